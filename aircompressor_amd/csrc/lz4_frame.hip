// lz4_frame.hip -- batched LZ4 frame container decode for gfx950.
//
// Replaces Lz4FrameCompression.decompress / decompressFrame / skipFrame (M/lz4/Lz4FrameCompression.java:145-343) over the
// HIP block decoder.  One wavefront per item (a buffer of concatenated frames), persistent grid: the frame walk is a
// serial chain (every block's output position and remaining capacity depend on the blocks before it), so the wavefront
// runs the Java loop itself -- same checks, same order, so status / detail / offset equal the Java exception -- and uses
// its 64 lanes inside each step: the block decoder of lz4_decode_body.h over LDS rings (64 lanes per block), 64 x 16-byte
// copies for stored blocks, XXH32 (achip_xxhash.h) for the header / block / content checksums.  Throughput comes from
// many frames per batch; a 4 MiB block is one wavefront's work.
#include "lz4_decode_body.h"
#include "lz4_frame_head.h"
#include "achip_launch.h"
#include "achip_lists.h"

namespace achip {

namespace lz4f {
constexpr int IN_RING = 2048, OUT_RING = 4096;
using FR = Rings<64, IN_RING, OUT_RING, 1>;

#define LZ4F_FAIL(detail, off)                            \
    {                                                     \
        eo = (int64_t)(off);                              \
        return mk_status(ACHIP_CLASS_MALFORMED, detail);  \
    }

// decompressFrame :184-322 ; wave-uniform.  Returns 0 or the status; pos / op advance.
//
// acceptLinked (achip_ctx_set_lz4frame_linked_blocks; a step beyond the Java reader, which refuses such frames): the blocks of a frame whose block-independence
// bit is clear may look back into this frame's content, out[outStart, o) -- compressed and stored blocks alike, never a frame before it or anything in front of
// the item.  A compressed block is told how much of it there is (at most the format's 65 535); the decoder reads it from memory (far matches, and once per
// block into its ring: Rings::prime_history).  Those bytes were stored by this wavefront -- the ring flushes of the block before, group_copy for a stored
// block -- and the wave_mem_order() behind either keeps the compiler from moving the next block's loads in front of them; the hardware performs a wavefront's
// vector memory operations in the order they were issued, which is all the far matches inside one block have ever relied on.  Nothing waits for another wavefront.
__device__ int32_t decompress_frame(const uint8_t* __restrict__ in, int32_t inLen, uint8_t* out, int32_t outCap, uint8_t* lds, int lane, bool acceptLinked, int32_t& pos, int32_t& op,
                                    int64_t& eo)
{
    const int32_t outStart = op;
    FrameHeader h;
    const int32_t hst = read_frame_header(in, inLen, pos, acceptLinked, h, eo);
    if (hst != 0) {
        return hst;
    }
    const int32_t blockMax = h.blockMax;
    const bool blockChecksum = h.blockChecksum, contentSize = h.contentSize, contentChecksum = h.contentChecksum;
    const int64_t expectedSize = h.expectedSize;
    int32_t p = h.firstBlock;

    int32_t o = outStart;
    for (;;) {
        if ((int64_t)p + 4 > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_MISSING_BLOCK_SIZE, p);
        const uint32_t header = ld4(in + p);
        p += 4;
        if (header == 0) {
            break;
        }
        const bool stored = (header & UNCOMPRESSED_FLAG) != 0;
        const int64_t blockLen = header & 0x7FFFFFFFu;
        if (blockLen > blockMax || (int64_t)p + blockLen > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_BLOCK_PAST_END, p);
        if (stored) {
            if ((int64_t)o + blockLen > outCap) LZ4F_FAIL(ACHIP_D_LZ4F_OUTPUT_TOO_SMALL, o);
            wave_mem_order();
            group_copy<64>(out + o, in + p, (int32_t)blockLen, lane);
            wave_mem_order();
            o += (int32_t)blockLen;
        }
        else {
            FR R;
            R.init(lds, lds + IN_RING, in + p, (int32_t)blockLen, out + o, lane);
            int32_t bst = 0, beo = 0, bop = 0;
            const int32_t history = !h.linked ? 0 : (o - outStart < 65535 ? o - outStart : 65535);
            lz4_block_decode<64, IN_RING, OUT_RING, 1, 0, true>(R, in + p, (int32_t)blockLen, outCap - o, bst, beo, bop, history);
            wave_mem_order();
            if (bst != 0) {
                if (bst == mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_LZ4_EMPTY_OUTPUT)) {
                    LZ4F_FAIL(ACHIP_D_LZ4F_OUTPUT_TOO_SMALL, o);  // the block codec returned -1 (:275-277)
                }
                eo = (int64_t)beo;  // the block codec's exception propagates; its offset is relative to the block
                return bst;
            }
            if (bop > blockMax) LZ4F_FAIL(ACHIP_D_LZ4F_BLOCK_EXCEEDS_MAX, p);
            o += bop;
        }
        if (blockChecksum) {
            const int64_t cpos = (int64_t)p + blockLen;
            if (cpos + 4 > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_MISSING_BLOCK_CHECKSUM, cpos);
            const uint32_t actual = quad_xxh32(in + p, (int32_t)blockLen, 0u, lane & 3, lane - (lane & 3));
            if (ld4(in + cpos) != actual) LZ4F_FAIL(ACHIP_D_LZ4F_BLOCK_CHECKSUM, cpos);
        }
        p += (int32_t)blockLen;
        if (blockChecksum) {
            p += 4;
        }
    }
    const int32_t contentLen = o - outStart;
    if (contentChecksum) {
        if ((int64_t)p + 4 > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_MISSING_CONTENT_CHECKSUM, p);
        const uint32_t actual = quad_xxh32(out + outStart, contentLen, 0u, lane & 3, lane - (lane & 3));
        if (ld4(in + p) != actual) LZ4F_FAIL(ACHIP_D_LZ4F_CONTENT_CHECKSUM, p);
        p += 4;
    }
    if (contentSize && (int64_t)contentLen != expectedSize) LZ4F_FAIL(ACHIP_D_LZ4F_CONTENT_SIZE, p);
    pos = p;
    op = o;
    return 0;
}

// decompress :145-177
__device__ int32_t decompress_item(const uint8_t* __restrict__ in, int32_t inLen, uint8_t* out, int32_t outCap, uint8_t* lds, int lane, bool acceptLinked, int32_t& opOut, int64_t& eo)
{
    eo = 0;
    opOut = 0;
    if (inLen < HEADER_SIZE) LZ4F_FAIL(ACHIP_D_LZ4F_TOO_SHORT, 0);
    int32_t pos = 0, op = 0;
    while (pos < inLen) {
        if ((int64_t)pos + 4 > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_TRUNC_MAGIC, pos);
        const uint32_t magic = ld4(in + pos);
        if (magic == MAGIC) {
            const int32_t r = decompress_frame(in, inLen, out, outCap, lds, lane, acceptLinked, pos, op, eo);
            if (r != 0) {
                return r;
            }
        }
        else if ((magic & SKIPPABLE_MASK) == SKIPPABLE_MAGIC) {  // skipFrame :327-343
            const int64_t spos = (int64_t)pos + 4;
            if (spos + 4 > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_TRUNC_SKIP_SIZE, spos);
            const int64_t frameEnd = spos + 4 + (int64_t)ld4(in + spos);
            if (frameEnd > inLen) LZ4F_FAIL(ACHIP_D_LZ4F_TRUNC_SKIP, spos);
            pos = (int32_t)frameEnd;
        }
        else {
            LZ4F_FAIL(ACHIP_D_LZ4F_BAD_MAGIC, pos);
        }
    }
    opOut = op;
    return 0;
}
#undef LZ4F_FAIL

}  // namespace lz4f

// ---- reader variants 1 and 2 (2: the default): the blocks of the regular frames as ONE batch for the block decoders, as hadoop_streams.hip
// does it for Hadoop streams.
//   walk   a lane per item: the item is exactly one frame, its header is in order, no block checksums; every compressed block becomes an
//          entry of a device-side batch, block k at output position k x blockMaxSize with at most a block's room.  That position is a GUESS
//          -- a block's length is not in the frame -- which holds for what every writer produces (all blocks but the last are full);
//   decode the batch through launch_listed_decode (achip_launch.h); the record arena of the two-pass decoder is sized after the host
//          has read back the number of blocks and their room;
//   fold   a wavefront per item walks the frame again: compressed blocks must have decoded, all but the last to a full block; stored blocks
//          are copied now; content checksum and content size are checked; anything else flags the item;
//   then the kernel above runs the flagged items, and every item of any other shape, from scratch (the Java loop: same status / offset).  A frame of linked blocks
//   is of another shape whatever the context accepts (frame_shape): its blocks are no batch of independent ones.
namespace lz4f {
struct BlockList : lists::ChunkBatch {  // (counters [2..3]: the entries' room, 64 bits; [8..11]: probe statistics)
    int32_t* sFirst;     // per item: first entry, -1 = not on this path
    int32_t* sSerial;    // per item: 1 = the wavefront-per-item kernel decodes it
    int32_t* cursor;     // the wavefront-per-item kernel's
    void carve(lists::Carver& k, int64_t nItems, bool listed)
    {
        cursor = k.take<int32_t>(lists::COUNTER_WORDS);
        if (listed) {
            sFirst = k.take<int32_t>(nItems);
            sSerial = k.take<int32_t>(nItems);
            ChunkBatch::carve(k, cursor + 16);
        }
    }
};

struct FrameShape {
    bool ok;
    int32_t firstBlock;      // position of the first block header
    int32_t blockMax;
    int32_t compressedBlocks;
    bool contentChecksum;
    int64_t expectedSize;    // -1: not announced
};

// the header of an item that holds exactly one frame of the shape the list path takes (decompressFrame :184-240 without its verdicts)
__device__ __forceinline__ FrameShape frame_shape(const uint8_t* __restrict__ in, int32_t inLen)
{
    FrameShape f;
    f.ok = false;
    f.firstBlock = 0;
    f.blockMax = 0;
    f.compressedBlocks = 0;
    f.contentChecksum = false;
    f.expectedSize = -1;
    if (inLen < HEADER_SIZE + 4 || ld4(in) != MAGIC) {
        return f;
    }
    const int flg = in[4], bd = in[5];
    if (((flg >> 6) & 3) != 1 || (flg & FLG_RESERVED_MASK) != 0 || (bd & BD_RESERVED_MASK) != 0 || (flg & FLG_BLOCK_INDEPENDENCE) == 0 || (flg & FLG_DICTIONARY_ID) != 0 ||
        (flg & FLG_BLOCK_CHECKSUM) != 0) {
        return f;
    }
    const int sizeId = (bd >> 4) & 7;
    if (sizeId < 4) {
        return f;
    }
    f.blockMax = 1 << (8 + 2 * sizeId);
    f.contentChecksum = (flg & FLG_CONTENT_CHECKSUM) != 0;
    int32_t p = 6;
    if ((flg & FLG_CONTENT_SIZE) != 0) {
        if (p + 8 + 1 > inLen) {
            return f;
        }
        f.expectedSize = (int64_t)ld8(in + p);
        p += 8;
    }
    if (p + 1 > inLen || in[p] != (int)((xxh32_short(in + 4, p - 4) >> 8) & 0xFF)) {
        return f;
    }
    f.firstBlock = p + 1;
    f.ok = true;
    return f;
}

// the blocks of such a frame: FILL = 0 counts the compressed ones and checks that the frame ends the item; FILL = 1 writes their entries
template <bool FILL>
__device__ __forceinline__ bool frame_blocks(const BatchArgs& a, int32_t item, FrameShape& f, const BlockList& L, int32_t firstEntry)
{
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[item];
    const int32_t inLen = a.srcLen[item];
    const int64_t outCap = a.dstCap[item];
    int64_t p = f.firstBlock;
    int64_t o = 0;
    int32_t n = 0;
    for (;;) {
        if (p + 4 > inLen) {
            return false;
        }
        const uint32_t header = ld4(in + p);
        p += 4;
        if (header == 0) {
            break;
        }
        const int64_t blockLen = header & 0x7FFFFFFFu;
        if (blockLen > f.blockMax || p + blockLen > inLen || o >= outCap) {
            return false;
        }
        if ((header & UNCOMPRESSED_FLAG) != 0) {
            if (o + blockLen > outCap) {
                return false;
            }
            // (a stored block shorter than a full one must be the last: fold sees to that through the positions)
            o += blockLen < f.blockMax ? blockLen : f.blockMax;
        }
        else {
            if (FILL) {
                const int32_t e = firstEntry + n;
                L.cSrcOff[e] = a.srcOff[item] + p;
                L.cSrcLen[e] = (int32_t)blockLen;
                L.cDstOff[e] = a.dstOff[item] + o;
                L.cDstCap[e] = (int32_t)(outCap - o < f.blockMax ? outCap - o : f.blockMax);
                L.cOutLen[e] = 0;
                L.cStatus[e] = -1;
                L.cErrOff[e] = 0;
            }
            n++;
            o += f.blockMax;  // the guess: this block is full (the last one may fall short: nothing follows it)
        }
        p += blockLen;
    }
    if (f.contentChecksum) {
        if (p + 4 > inLen) {
            return false;
        }
        p += 4;
    }
    f.compressedBlocks = n;
    return p == inLen;  // (frames or skippable frames behind it: the other kernel's)
}
}  // namespace lz4f

__global__ __launch_bounds__(64) void lz4frame_walk_kernel(BatchArgs a, lz4f::BlockList L)
{
    using namespace lz4f;
    const int32_t item = blockIdx.x * 64 + threadIdx.x;
    if (item >= a.nBlocks) {
        return;
    }
    L.sFirst[item] = -1;
    L.sSerial[item] = 1;
    FrameShape f = frame_shape(a.srcBase + a.srcOff[item], a.srcLen[item]);
    if (!f.ok || a.dstCap[item] <= 0 || !frame_blocks<false>(a, item, f, L, 0)) {
        return;
    }
    const int32_t first = atomicAdd(L.counters, f.compressedBlocks);
    if ((int64_t)first + f.compressedBlocks > lists::CAPACITY) {
        return;
    }
    frame_blocks<true>(a, item, f, L, first);
    long long room = 0;
    for (int32_t k = 0; k < f.compressedBlocks; k++) {
        room += L.cDstCap[first + k];
    }
    atomicAdd((unsigned long long*)(L.counters + 2), (unsigned long long)room);
    L.sFirst[item] = first;
    L.sSerial[item] = 0;
}

// a wavefront per item on the list path
__global__ __launch_bounds__(64) void lz4frame_fold_kernel(BatchArgs a, lz4f::BlockList L, int32_t decoded)
{
    using namespace lz4f;
    const int32_t item = blockIdx.x;
    if (L.sSerial[item] != 0) {
        return;
    }
    const int lane = threadIdx.x;
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[item];
    uint8_t* out = a.dstBase + a.dstOff[item];
    const FrameShape f = frame_shape(in, a.srcLen[item]);  // (the walk's findings again: wave-uniform)
    bool ok = decoded != 0;
    int64_t p = f.firstBlock, o = 0;
    int32_t e = L.sFirst[item];
    bool shortSeen = false;  // a block that fell short of a full one: nothing may follow it
    while (ok) {  // (uniform)
        const uint32_t header = ld4(in + p);
        p += 4;
        if (header == 0) {
            break;
        }
        const int64_t blockLen = header & 0x7FFFFFFFu;
        ok = !shortSeen;
        if (!ok) {
            break;
        }
        if ((header & UNCOMPRESSED_FLAG) != 0) {
            wave_sync();
            group_copy<64>(out + o, in + p, (int32_t)blockLen, lane);
            wave_sync();
            shortSeen = blockLen < f.blockMax;
            o += blockLen;
        }
        else {
            const int32_t got = L.cOutLen[e];
            ok = L.cStatus[e] == 0;
            shortSeen = got < f.blockMax;
            o += got;
            e++;
        }
        p += blockLen;
    }
    if (ok && f.contentChecksum) {
        wave_sync();
        const uint32_t actual = quad_xxh32(out, (int32_t)o, 0u, lane & 3, lane - (lane & 3));
        ok = ld4(in + p) == actual;
    }
    ok = ok && (f.expectedSize < 0 || o == f.expectedSize);
    if (lane == 0) {
        if (ok) {
            a.outLen[item] = (int32_t)o;
            a.status[item] = 0;
            a.errOffset[item] = 0;
        }
        else {
            L.sSerial[item] = 1;  // the Java loop decides what it means
        }
    }
}

// LISTED: only the items `list` flags (the list path's leftovers).  acceptLinked: KernelSettings::lz4fLinkedBlocks
template <bool LISTED>
__global__ __launch_bounds__(64) void lz4frame_decompress_kernel(BatchArgs a, int32_t* nextItem, const int32_t* __restrict__ list, int32_t acceptLinked)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[lz4f::IN_RING + lz4f::OUT_RING];
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            item = atomicAdd(nextItem, 1);
        }
        __syncthreads();
        const int32_t block = item;
        if (block >= a.nBlocks) {
            return;
        }
        if (LISTED && list[block] == 0) {
            continue;
        }
        int32_t op = 0;
        int64_t eo = 0;
        const int32_t st = lz4f::decompress_item(a.srcBase + a.srcOff[block], a.srcLen[block], a.dstBase + a.dstOff[block], a.dstCap[block], lds, lane, acceptLinked != 0, op, eo);
        if (lane == 0) {
            a.outLen[block] = st == 0 ? op : 0;
            a.status[block] = st;
            a.errOffset[block] = st == 0 ? 0 : eo;
        }
    }
}

int64_t lz4frame_decompress_scratch_bytes(int32_t nItems, int variant)
{
    lists::Carver k(nullptr);
    lz4f::BlockList().carve(k, nItems < 1 ? 1 : nItems, variant == 1 || variant == 2);
    return k.used();
}

// variant 0, or no `aux`: a wavefront per item; variants 1 and 2: the block list (above).  1: always the two-pass decoder.  2 (the default): the
// sequence-length probe of the block API's auto mode decides -- short sequences (text: 7.8 -> 13.4 GiB/s) take the two-pass decoder, and leave
// every item to the wavefront-per-item kernel when there is no arena for it; long ones the ring decoders, the lanes per block by how many blocks
// there are (profiles/r05_groupsweep.txt: 16 384 blocks of 256 KiB 890 GiB/s at 16 lanes, 1 024 of 4 MiB 85 at 64) -- the wavefront-per-item
// kernel, where these frames went until round 5, is a serial reader that was never the fast one: 149 GiB/s on 16 384 frames of 256 KiB.
hipError_t launch_lz4frame_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, int variant, const AuxScratch* aux, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    const bool listed = (variant == 1 || variant == 2) && aux != nullptr && aux->get != nullptr;
    lists::Carver k(scratch);
    lz4f::BlockList L;
    L.carve(k, a.nBlocks, listed);
    hipError_t e = hipMemsetAsync(L.cursor, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const int32_t maxWaves = 256 * 16;
    const unsigned grid = (unsigned)(a.nBlocks < maxWaves ? a.nBlocks : maxWaves);
    if (!listed) {
        hipLaunchKernelGGL(lz4frame_decompress_kernel<false>, dim3(grid), dim3(64), 0, stream, a, L.cursor, (const int32_t*)nullptr, (int32_t)ks.lz4fLinkedBlocks);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(lz4frame_walk_kernel, dim3((unsigned)((a.nBlocks + 63) / 64)), dim3(64), 0, stream, a, L);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, lists::CAPACITY);
    // the number of listed blocks and their room decide the record arena: the one synchronisation of the call
    const ListedWant want{true, variant == 2, false, 1, 2};
    bool decoded = false;
    e = launch_listed_decode(L.as_batch(a, lists::CAPACITY), 0, stream, L.counters, L.counters + 8, aux, ks, want, &decoded);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lz4frame_fold_kernel, dim3((unsigned)a.nBlocks), dim3(64), 0, stream, a, L, decoded ? 1 : 0);
    hipLaunchKernelGGL(lz4frame_decompress_kernel<true>, dim3(grid), dim3(64), 0, stream, a, L.cursor, (const int32_t*)L.sSerial, (int32_t)ks.lz4fLinkedBlocks);
    return hipGetLastError();
}

}  // namespace achip
