// pack_outputs.hip -- the compress side's counterpart of decoded_size.hip: what a batch needs for its compress call, found on the device
// (achip_compress_bound_batch), and the compaction of what that call left in its worst-case slots into one dense stream (achip_pack_outputs).
// DESIGN 10c has the contract.
//
//   bounds   a lane per item; the eight formulas are achip_bounds.h's, which the host functions achip_*_max_compressed_length call too.
//   scan     achip_plan.h's reduce / tile scan / scan over PackRoom: an item's length is outLen[i], or rawLen[i] where the raw arrays are given and
//            the compressed form is no smaller (an ORC writer's isOriginal chunk); an item with a status or a negative length takes no room.
//            The tile-scan's one thread also decides whether the bytes are copied: total[2] = packedBase given and total[0] <= packedCap.
//   copy     the dense stream is cut into tiles of PACK_TILE_BYTES of DESTINATION ADDRESS (so that a 16-byte store is aligned whatever packedBase
//            is); a workgroup takes tiles round-robin.  Two wavefronts find the tile's first and last item in packedOff[] by a 64-way search (a
//            probe per lane and a ballot: three rounds for a quarter of a million items); every lane then owns eight 16-byte chunks, 4 KiB apart, and
//            finds each chunk's item by a binary search between those two -- no step at all inside a multi-megabyte item, eleven steps of cached
//            reads among 1 600 twenty-byte ones, and a run of items without room is skipped by the search, never walked.  A chunk that lies
//            inside one item's bytes is one 16-byte load at whatever alignment the source has (gfx950 runs in unaligned-access mode) and one aligned
//            16-byte store, a chunk inside the zeros behind an item the store alone; all of a lane's loads are issued before its first store.  A
//            chunk that holds an item's head or tail, the start of its padding, or items shorter than a vector is gathered item by item from byte
//            loads into registers and stored once (16 bytes wide too, unless it is the stream's first or last chunk).
//            (Tried on the device and dropped, profiles/pack_rate.txt: a second path that copies a tile of few items item by item with the whole
//            workgroup, the item's arrays read once -- no faster on 64 KiB blocks, slower on short items.)
#include "achip_launch.h"
#include "achip_bounds.h"
#include "achip_plan.h"

namespace achip {

namespace pk {

constexpr int PACK_THREADS = 256, PACK_CHUNKS = 8;
static_assert(PACK_TILE_BYTES == (int64_t)PACK_THREADS * PACK_CHUNKS * 16, "a tile is eight 16-byte chunks per lane");

// ---------------------------------------------------------------------------------------------------------------------
// bounds
__device__ __forceinline__ int64_t compress_bound(int32_t op, int32_t n, int32_t hadoopBufferSize, int32_t snfBlockSize)
{
    switch (op) {
        case ACHIP_OP_LZ4_COMPRESS: return bound::lz4(n);
        case ACHIP_OP_SNAPPY_COMPRESS: return bound::snappy(n);
        case ACHIP_OP_ZSTD_COMPRESS: return bound::zstd(n);
        case ACHIP_OP_LZ4FRAME_COMPRESS: return bound::lz4frame(n);
        case ACHIP_OP_SNAPPYFRAMED_COMPRESS: return bound::snappyframed(n, snfBlockSize);
        case ACHIP_OP_LZ4HADOOP_COMPRESS: return bound::hadoop(false, n, hadoopBufferSize);
        case ACHIP_OP_SNAPPYHADOOP_COMPRESS: return bound::hadoop(true, n, hadoopBufferSize);
        case ACHIP_OP_ZSTDSTREAM_COMPRESS: return bound::zstdstream(n);
        case ACHIP_OP_LZO_COMPRESS: return bound::lzo(n);
        default: return -1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// scan
struct PackRoom {
    const int32_t* __restrict__ outLen;
    const int32_t* __restrict__ status;
    const int32_t* __restrict__ rawLen;  // null: no raw arrays
    int64_t* packedOff;
    int32_t* packedLen;
    int32_t* stored;  // null iff rawLen is
    int64_t packedCap;
    int32_t copy;  // packedBase was given
    __device__ __forceinline__ bool takes_raw(int64_t i, int32_t len) const { return rawLen != nullptr && rawLen[i] >= 0 && len >= rawLen[i]; }
    __device__ __forceinline__ int64_t room(int64_t i, int64_t n, int64_t mask, int32_t& len, int32_t& leftOut) const
    {
        len = 0;
        leftOut = 0;
        if (i >= n) {
            return 0;
        }
        const int32_t l = outLen[i];
        if (status[i] != 0 || l < 0) {
            leftOut = 1;
            return 0;
        }
        len = takes_raw(i, l) ? rawLen[i] : l;
        return ((int64_t)len + mask) & ~mask;
    }
    __device__ __forceinline__ void emit(int64_t i, int64_t at, int32_t len) const
    {
        packedOff[i] = at;
        packedLen[i] = len;
        if (stored != nullptr) {
            const int32_t l = outLen[i];
            stored[i] = (status[i] == 0 && l >= 0 && takes_raw(i, l)) ? 1 : 0;
        }
    }
    __device__ __forceinline__ void finish(int64_t* total) const { total[2] = (copy != 0 && total[0] <= packedCap) ? 1 : 0; }
};

// ---------------------------------------------------------------------------------------------------------------------
// copy
// The last item in [0, n) whose offset is <= x (offsets never decrease and off[0] = 0 <= x), by the whole wavefront: 64 probes a round.  Items without room share
// their successor's offset, so the answer is never one of a run of them unless nothing follows.  (uniform)
__device__ __forceinline__ int64_t wave_search(const int64_t* __restrict__ off, int64_t n, int64_t x, int lane)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t step = (hi - lo - 1 + 63) / 64;
        const int64_t p = lo + (int64_t)(lane + 1) * step;
        const bool le = p < hi && off[p] <= x;
        const int64_t cnt = __popcll(__ballot(le));
        const int64_t next = lo + (cnt + 1) * step;
        lo += cnt * step;
        hi = next < hi ? next : hi;
    }
    return lo;
}
// the same between two items, by one lane (off[first] <= x)
__device__ __forceinline__ int64_t lane_search(const int64_t* __restrict__ off, int64_t first, int64_t last, int64_t x)
{
    int64_t lo = first, hi = last + 1;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    return lo;
}
__device__ __forceinline__ const uint8_t* item_bytes(const uint8_t* __restrict__ srcBase, const int64_t* __restrict__ srcOff, const uint8_t* __restrict__ rawBase,
                                                     const int64_t* __restrict__ rawOff, const int32_t* __restrict__ stored, int64_t j)
{
    return (stored != nullptr && stored[j] != 0) ? rawBase + rawOff[j] : srcBase + srcOff[j];
}
// (the kernel and its helpers take PackCopy's members one by one: handed the struct, the compiler kept it in scratch memory and every pointer read from
// there made a flat load of what it pointed to -- 136 registers and 104 bytes of scratch a lane against 40-odd and none)
#define PACK_SOURCES srcBase, srcOff, rawBase, rawOff, stored
#define PACK_SOURCES_DECL                                                                                                                    \
    const uint8_t *__restrict__ srcBase, const int64_t *__restrict__ srcOff, const uint8_t *__restrict__ rawBase, const int64_t *__restrict__ rawOff, \
        const int32_t *__restrict__ stored
// A chunk that is not one item's bytes: dense bytes [from, to) of the 16 at d0 -- items' heads and tails, the zeros behind them, items shorter than a vector --
// gathered item by item into two registers and stored once.  An item's bytes are 16 byte loads at clamped (always valid) indices, so that they are issued
// together and waited for once: a loop of load-then-store per byte costs a memory round trip each.  wholeStore: [from, to) is the whole chunk.
__device__ __forceinline__ void copy_mixed_chunk(PACK_SOURCES_DECL, const int64_t* __restrict__ packedOff, const int32_t* __restrict__ packedLen, uint8_t* dst, int64_t mask,
                                                 int64_t first, int64_t last, int64_t d0, int64_t from, int64_t to, bool wholeStore)
{
    uint64_t lo64 = 0, hi64 = 0;
    int64_t j = first, pos = from;
    while (pos < to) {
        j = lane_search(packedOff, j, last, pos);
        const int64_t off = packedOff[j];
        const int64_t len = packedLen[j];
        const int64_t dataEnd = off + len, roomEnd = off + ((len + mask) & ~mask);
        const int64_t stop = roomEnd < to ? roomEnd : to;
        if (stop <= pos) {  // (offsets that are not a scan of these lengths: no progress to be made)
            break;
        }
        const int64_t bytesEnd = dataEnd < stop ? dataEnd : stop;
        if (pos < bytesEnd) {  // (len >= 1)
            const uint8_t* __restrict__ in = item_bytes(PACK_SOURCES, j);
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const int64_t p = d0 + b;
                int64_t idx = p - off;
                idx = idx < 0 ? 0 : (idx >= len ? len - 1 : idx);
                const uint64_t x = (p >= pos && p < bytesEnd) ? (uint64_t)in[idx] : 0;
                if (b < 8) {
                    lo64 |= x << (8 * b);
                }
                else {
                    hi64 |= x << (8 * (b - 8));
                }
            }
        }
        pos = stop;
    }
    uint8_t* const out = dst + d0;
    if (wholeStore) {
        const u32x4 v = {(uint32_t)lo64, (uint32_t)(lo64 >> 32), (uint32_t)hi64, (uint32_t)(hi64 >> 32)};
        *(u32x4*)__builtin_assume_aligned(out, 16) = v;
    }
    else {  // the stream's first and last chunk
#pragma unroll
        for (int b = 0; b < 16; b++) {
            if (d0 + b >= from && d0 + b < to) {
                out[b] = (uint8_t)((b < 8 ? lo64 >> (8 * b) : hi64 >> (8 * (b - 8))) & 0xFF);
            }
        }
    }
}

}  // namespace pk

__global__ __launch_bounds__(256) void compress_bound_kernel(int32_t op, const int32_t* __restrict__ srcLen, int64_t* __restrict__ outSize, int32_t* __restrict__ status, int32_t n,
                                                             int32_t hadoopBufferSize, int32_t snfBlockSize)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const int32_t len = srcLen[i];
    const int64_t b = len < 0 ? -1 : pk::compress_bound(op, len, hadoopBufferSize, snfBlockSize);
    const bool bad = b < 0 || b > 0x7FFFFFFF;
    outSize[i] = bad ? 0 : b;
    status[i] = bad ? mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT) : 0;
}

__global__ __launch_bounds__(256) void pack_copy_kernel(PACK_SOURCES_DECL, const int64_t* __restrict__ packedOff, const int32_t* __restrict__ packedLen,
                                                        const int64_t* __restrict__ totalDev, uint8_t* dst, int64_t packedCap, int64_t mask, int32_t n)
{
    using namespace pk;
    __shared__ int64_t bounds[2];
    const int64_t total = totalDev[0];
    if (total <= 0 || total > packedCap) {  // (uniform) nothing to copy, or the stream does not fit: not one byte is written
        return;
    }
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // positions are counted from the 16-byte boundary at or below packedBase: a = dense offset + shift, and dstA + a is aligned whenever a is
    const int64_t shift = (int64_t)((uintptr_t)dst & 15);
    uint8_t* const dstA = dst - shift;
    const int64_t aEnd = shift + total;
    const int64_t tiles = (aEnd + PACK_TILE_BYTES - 1) / PACK_TILE_BYTES;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform)
        const int64_t tileA = tile * PACK_TILE_BYTES;
        const int64_t lo = tileA > shift ? tileA : shift;
        const int64_t hi = tileA + PACK_TILE_BYTES < aEnd ? tileA + PACK_TILE_BYTES : aEnd;  // (lo < hi: shift < 16 and tileA < aEnd)
        __syncthreads();
        if (wave < 2) {  // (uniform per wavefront)
            const int64_t r = wave_search(packedOff, n, (wave == 0 ? lo : hi - 1) - shift, lane);
            if (lane == 0) {
                bounds[wave] = r;
            }
        }
        __syncthreads();
        const int64_t first = bounds[0], last = bounds[1];
        u32x4 v[PACK_CHUNKS];
        uint32_t whole = 0, bytewise = 0;
#pragma unroll
        for (int k = 0; k < PACK_CHUNKS; k++) {
            v[k] = u32x4{0, 0, 0, 0};
            const int64_t a0 = tileA + ((int64_t)k * PACK_THREADS + t) * 16;
            if (a0 + 16 <= lo || a0 >= hi) {
                continue;
            }
            if (a0 >= lo && a0 + 16 <= hi) {
                const int64_t d0 = a0 - shift;
                const int64_t j = lane_search(packedOff, first, last, d0);
                const int64_t off = packedOff[j];
                const int64_t len = packedLen[j];
                if (d0 + 16 <= off + len) {
                    v[k] = ld16(item_bytes(PACK_SOURCES, j) + (d0 - off));
                    whole |= 1u << k;
                    continue;
                }
                if (d0 >= off + len && d0 + 16 <= off + ((len + mask) & ~mask)) {  // all padding (large alignments): v[k] is zero
                    whole |= 1u << k;
                    continue;
                }
            }
            bytewise |= 1u << k;
        }
#pragma unroll
        for (int k = 0; k < PACK_CHUNKS; k++) {
            if ((whole >> k) & 1u) {
                uint8_t* const out = dstA + tileA + ((int64_t)k * PACK_THREADS + t) * 16;
                *(u32x4*)__builtin_assume_aligned(out, 16) = v[k];
            }
        }
        if (bytewise != 0) {
#pragma nounroll  // (one copy of the gather: eight cost 70 registers a lane and half the wavefronts a SIMD holds)
            for (int k = 0; k < PACK_CHUNKS; k++) {
                if ((bytewise >> k) & 1u) {
                    const int64_t a0 = tileA + ((int64_t)k * PACK_THREADS + t) * 16;
                    copy_mixed_chunk(PACK_SOURCES, packedOff, packedLen, dst, mask, first, last, a0 - shift, (a0 > lo ? a0 : lo) - shift, (a0 + 16 < hi ? a0 + 16 : hi) - shift, a0 >= lo && a0 + 16 <= hi);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// launchers
hipError_t launch_compress_bound(int32_t op, const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t nBlocks, int32_t hadoopBufferSize, hipStream_t stream, int32_t snfBlockSize)
{
    if (nBlocks <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(compress_bound_kernel, dim3((unsigned)(((int64_t)nBlocks + 255) / 256)), dim3(256), 0, stream, op, srcLen, outSize, status, nBlocks, hadoopBufferSize, snfBlockSize);
    return hipGetLastError();
}

int64_t pack_outputs_scratch_bytes(int32_t nBlocks) { return plan_scan_scratch_bytes(nBlocks); }

hipError_t launch_pack_outputs(const PackArgs& p, void* scratch, hipStream_t stream)
{
    if (p.nBlocks <= 0) {
        return hipSuccess;
    }
    const pk::PackRoom room{p.outLen, p.status, p.rawLen, p.packedOff, p.packedLen, p.stored, p.packedCap, p.packedBase != nullptr ? 1 : 0};
    hipError_t e = launch_plan_scan(room, p.nBlocks, p.align, p.total, scratch, stream);
    if (e != hipSuccess || p.packedBase == nullptr || p.packedCap <= 0) {
        return e;
    }
    // a stream that is copied has at most packedCap bytes: the tiles of that many, at most the 2 048 workgroups the chip holds at once (the rest round-robin)
    const int64_t tiles = (p.packedCap + 15 + PACK_TILE_BYTES - 1) / PACK_TILE_BYTES;
    hipLaunchKernelGGL(pack_copy_kernel, dim3((unsigned)(tiles < 2048 ? tiles : 2048)), dim3(pk::PACK_THREADS), 0, stream, p.srcBase, p.srcOff, p.rawBase, p.rawOff,
                       (const int32_t*)p.stored, (const int64_t*)p.packedOff, (const int32_t*)p.packedLen, (const int64_t*)p.total, p.packedBase, p.packedCap, (int64_t)p.align - 1, p.nBlocks);
    return hipGetLastError();
}

}  // namespace achip
