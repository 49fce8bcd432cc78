// lz4_frame_writer.hip -- the block-list LZ4 frame writer: frames the Java writer cannot write (achip_ctx_set_lz4frame_writer: a block-maximum size of 64 KiB,
// 256 KiB, 1 MiB or 4 MiB, block checksums, a content checksum, the content size), their independent blocks encoded side by side.  DESIGN 10f.
//
// The wavefront-per-frame kernel (lz4_compress_kernels.h: lz4frame_compress_kernel) stays what every frame at the default settings is written by; this unit runs
// for any other setting, and at the defaults under lz4frame.compress.variant 1.  Its shape is the Hadoop writer's (hadoop_streams.hip) over lists::WriterList:
//
//   plan      a lane per frame: ceil(srcLen / B) entries; the capacity is held against bound::lz4frame_list HERE, so a frame that is refused has not one byte
//             of its destination written
//   seal
//   encode    a persistent grid draws entries: a block through lz4_compress_block_mw into its worst-case place inside the frame's destination; the block
//             checksum, where asked for, right behind by the same wavefront (the block is in its cache; the compaction is one wavefront per FRAME and would
//             walk a frame's checksums one after the other)
//   compact   a wavefront per frame: header, then block by block the move to the left (a block that did not shrink: copied from the source instead), the size
//             field in front and the checksum behind -- both written AFTER the move, since a field of block k may lie inside block k - 1's worst-case place --,
//             the end mark, the content checksum
#include "lz4_compress_body.h"
#include "lz4_compress_mw.h"
#include "achip_launch.h"
#include "achip_lists.h"
#include "achip_bounds.h"
#include "achip_xxhash.h"

namespace achip {

namespace lz4fw {

// the frame descriptor a launch writes (wave-uniform kernel arguments)
struct Frame {
    int32_t blockMax;  // 65536 << (2 * (id - 4)), id = 4 .. 7
    int32_t blockChecksum, contentChecksum, contentSize;  // 0 / 1
};
__host__ __device__ inline int64_t header_bytes(const Frame& f) { return 7 + 8 * (int64_t)f.contentSize; }
__host__ __device__ inline int64_t slot_bytes(const Frame& f) { return 4 + 4 * (int64_t)f.blockChecksum + bound::lz4(f.blockMax); }  // a full block's worst-case place
__host__ __device__ inline int32_t bd_id(const Frame& f) { return f.blockMax == 65536 ? 4 : (f.blockMax == 262144 ? 5 : (f.blockMax == 1048576 ? 6 : 7)); }

// lists::WriterList (bSize: a kept block's compressed bytes, -1: stored) and, beside it, the block checksums
struct BlockList : lists::WriterList {
    uint32_t* bSum;
};

__global__ __launch_bounds__(64) void lz4f_list_plan_kernel(BatchArgs a, BlockList L, Frame f, int32_t capacity)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    const int32_t inLen = a.srcLen[stream];
    int32_t st = 0;
    int64_t blocks = 0;
    if (inLen < 0) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    else {
        blocks = ((int64_t)inLen + f.blockMax - 1) / f.blockMax;
        const int64_t need = bound::lz4frame_list(inLen, f.blockMax, f.blockChecksum, f.contentChecksum, f.contentSize);
        if (need > 0x7FFFFFFF) {
            st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
        }
        else if ((int64_t)a.dstCap[stream] < need) {
            st = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_LZ4F_MAX_OUTPUT);
        }
    }
    if (!lists::plan_entries(L, stream, st == 0 ? (int32_t)blocks : 0, capacity)) {  // (more blocks than the list holds in one call)
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_UNSUPPORTED);
    }
    L.sStatus[stream] = st;
}

}  // namespace lz4fw

#define LZ4K(name) name
#define LZ4K_PARAM
#define LZ4K_ACCEL false
#define LZ4K_VALUE 1
#include "lz4_frame_writer_kernels.h"
#undef LZ4K
#undef LZ4K_PARAM
#undef LZ4K_ACCEL
#undef LZ4K_VALUE
// the `_accel` twin, launched for an acceleration above 1
#define LZ4K(name) name##_accel
#define LZ4K_PARAM , int32_t accel
#define LZ4K_ACCEL true
#define LZ4K_VALUE accel
#include "lz4_frame_writer_kernels.h"
#undef LZ4K
#undef LZ4K_PARAM
#undef LZ4K_ACCEL
#undef LZ4K_VALUE

namespace lz4fw {

__global__ __launch_bounds__(64) void lz4f_list_compact_kernel(BatchArgs a, BlockList L, Frame f)
{
    const int lane = threadIdx.x;
    const int64_t worst = slot_bytes(f);
    const int32_t stream = blockIdx.x;  // a wavefront per frame
    const int32_t st = L.sStatus[stream];
    int64_t o = 0;
    if (st == 0) {
        const uint8_t* in = a.srcBase + a.srcOff[stream];
        uint8_t* out = a.dstBase + a.dstOff[stream];
        const int32_t inLen = a.srcLen[stream];
        const int32_t first = L.sFirst[stream], n = L.sCount[stream];
        const int64_t head = header_bytes(f);
        if (lane == 0) {  // (the header lies in front of every worst-case place)
            st4(out, 0x184D2204u);
            out[4] = (uint8_t)(0x60 | (f.blockChecksum << 4) | (f.contentSize << 3) | (f.contentChecksum << 2));  // version 01, independent blocks
            out[5] = (uint8_t)(bd_id(f) << 4);
            if (f.contentSize) {
                st8(out + 6, (uint64_t)(uint32_t)inLen);
            }
        }
        wave_mem_order();
        if (lane == 0) {
            out[head - 1] = (uint8_t)((xxh32_short(out + 4, (int32_t)head - 5) >> 8) & 0xFF);
        }
        o = head;
        for (int32_t k = 0; k < n; k++) {
            const int32_t size = L.bSize[first + k];
            const int64_t from = head + (int64_t)k * worst + 4;
            const int64_t pos = (int64_t)k * f.blockMax;
            const int32_t length = (int32_t)(inLen - pos < f.blockMax ? inLen - pos : f.blockMax);
            const int32_t payload = size >= 0 ? size : length;
            wave_mem_order();
            if (size < 0) {
                group_copy<64>(out + o + 4, in + pos, length, lane);  // stored: o + 4 + length (+ 4) never reaches block k + 1's place
            }
            else if (from != o + 4) {
                group_copy<64>(out + o + 4, out + from, size, lane);  // to the left; every lane loads before it stores
            }
            wave_mem_order();
            if (lane == 0) {  // (after the move: these fields may lie inside block k - 1's worst-case place)
                st4(out + o, size >= 0 ? (uint32_t)size : ((uint32_t)length | 0x80000000u));
                if (f.blockChecksum) {
                    st4(out + o + 4 + payload, L.bSum[first + k]);
                }
            }
            wave_mem_order();
            o += 4 + payload + 4 * f.blockChecksum;
        }
        uint32_t sum = 0;
        if (f.contentChecksum) {
            sum = quad_xxh32(in, inLen, 0u, lane & 3, lane - (lane & 3));
        }
        if (lane == 0) {
            st4(out + o, 0u);  // the end mark
            if (f.contentChecksum) {
                st4(out + o + 4, sum);
            }
        }
        o += 4 + 4 * f.contentChecksum;
    }
    if (lane == 0) {
        a.outLen[stream] = st == 0 ? (int32_t)o : 0;
        a.status[stream] = st;
        a.errOffset[stream] = 0;
    }
}

// achip_compress_bound_batch's line for this writer: bound::lz4frame_list per item
__global__ __launch_bounds__(256) void lz4f_list_bound_kernel(const int32_t* __restrict__ srcLen, int64_t* __restrict__ outSize, int32_t* __restrict__ status, int32_t n, Frame f)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const int32_t len = srcLen[i];
    const int64_t b = len < 0 ? -1 : bound::lz4frame_list(len, f.blockMax, f.blockChecksum, f.contentChecksum, f.contentSize);
    const bool bad = b < 0 || b > 0x7FFFFFFF;
    outSize[i] = bad ? 0 : b;
    status[i] = bad ? mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT) : 0;
}

}  // namespace lz4fw

namespace {
constexpr unsigned LZ4F_ENCODE_WORKGROUPS = 256 * 10;  // the 16 KiB table: ten wavefronts a CU; the 8 KiB form takes twice as many
lz4fw::Frame frame_of(const KernelSettings& ks) { return lz4fw::Frame{ks.lz4fBlockMaxSize, ks.lz4fBlockChecksum, ks.lz4fContentChecksum, ks.lz4fContentSize}; }
// the writer's scratch: the counter page, its list, the block checksums
void carve_lz4f_writer(lists::Carver& k, lz4fw::BlockList& L, int64_t nStreams)
{
    L.carve(k, k.take<int32_t>(lists::COUNTER_WORDS), nStreams, false);
    L.bSum = k.take<uint32_t>(lists::CAPACITY);
}
}  // namespace

int64_t lz4frame_list_compress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    lz4fw::BlockList L;
    carve_lz4f_writer(k, L, nStreams < 1 ? 1 : nStreams);
    return k.used();
}

hipError_t launch_lz4frame_list_compress(const BatchArgs& a, hipStream_t stream, void* scratch, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    lz4fw::BlockList L;
    carve_lz4f_writer(k, L, a.nBlocks);
    hipError_t e = hipMemsetAsync(L.counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const lz4fw::Frame f = frame_of(ks);
    const int32_t capacity = ks.lz4fListEntries > 0 && ks.lz4fListEntries < lists::CAPACITY ? ks.lz4fListEntries : lists::CAPACITY;
    const bool wide = f.blockMax > 65536;
    const unsigned full = wide ? LZ4F_ENCODE_WORKGROUPS : 2 * LZ4F_ENCODE_WORKGROUPS;
    const unsigned encodeGrid = ks.lz4fEncodeWorkgroups > 0 && (unsigned)ks.lz4fEncodeWorkgroups < full ? (unsigned)ks.lz4fEncodeWorkgroups : full;
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    const int32_t accel = ks.lz4Acceleration;
    hipLaunchKernelGGL(lz4fw::lz4f_list_plan_kernel, dim3(perStream), dim3(64), 0, stream, a, L, f, capacity);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, capacity);
    if (accel > 1) {
        if (wide) hipLaunchKernelGGL(lz4f_list_encode_kernel_accel<true>, dim3(encodeGrid), dim3(64), 0, stream, a, L, f, accel);
        else hipLaunchKernelGGL(lz4f_list_encode_kernel_accel<false>, dim3(encodeGrid), dim3(64), 0, stream, a, L, f, accel);
    }
    else {
        if (wide) hipLaunchKernelGGL(lz4f_list_encode_kernel<true>, dim3(encodeGrid), dim3(64), 0, stream, a, L, f);
        else hipLaunchKernelGGL(lz4f_list_encode_kernel<false>, dim3(encodeGrid), dim3(64), 0, stream, a, L, f);
    }
    hipLaunchKernelGGL(lz4fw::lz4f_list_compact_kernel, dim3((unsigned)a.nBlocks), dim3(64), 0, stream, a, L, f);
    return hipGetLastError();
}

hipError_t launch_lz4frame_list_bound(const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t nBlocks, hipStream_t stream, const KernelSettings& ks)
{
    if (nBlocks <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(lz4fw::lz4f_list_bound_kernel, dim3((unsigned)(((int64_t)nBlocks + 255) / 256)), dim3(256), 0, stream, srcLen, outSize, status, nBlocks, frame_of(ks));
    return hipGetLastError();
}

}  // namespace achip
