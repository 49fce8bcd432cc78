// achip_seqexec.h -- what the two passes of the record-based LZ77 decoders share (lz4_decompress_v7.hip, snappy_decompress_v5.hip):
// the 8-byte RECORD a parser writes per piece of work and the chunked arena the records live in, wave helpers, and the parser's view of
// its compressed stream (LaneFeed), how a sequence is cut into pieces (cut_piece), the lane parsers' record output (LaneRecordSink) and a block's
// write-back (finish_block).  The executor is achip_seqexec2.h.
//
//   parse    a lane per block walks the token grammar (serial by nature) and writes one record per piece
//            {literal length <= 16, match length <= 16, offset, header bytes skipped} into the arena -- no byte is copied;
//   execute  a WAVEFRONT per block runs 64 records at a time.
// With a wavefront per block only a few thousand blocks are open at a time (the lane-per-block decoders keep 131072+ open: 8x more memory
// traffic than bytes decoded on text), input and record streams are read coalesced, and the output is written in stream order.
//
// Cross-lane operations are only used in wave-uniform control flow and lanes exchange data through memory only across wave_sync():
// the kernels built on this header run unchanged under tools/hostemu (fibers) on a CPU.
#pragma once
#include <stddef.h>

#include "achip_device.h"

namespace achip {

namespace sx {

// ---- records --------------------------------------------------------------------------------------------------------------------
// bits  0..16  literal length   (the parsers emit pieces: <= 16)
// bits 17..33  match length     (likewise <= 16; 0 = none)
// bits 34..49  offset           (1..65535)
// bits 50..63  skip             compressed bytes between the end of the previous record's literals and this record's literals
//                               (tokens, length extensions, offsets; <= 16383, longer gaps are split)
constexpr int MAX_LEN = (1 << 17) - 1;
constexpr int MAX_SKIP = (1 << 14) - 1;
__device__ __forceinline__ uint64_t rec_pack(uint32_t lit, uint32_t ml, uint32_t off, uint32_t skip)
{
    return (uint64_t)lit | ((uint64_t)ml << 17) | ((uint64_t)off << 34) | ((uint64_t)skip << 50);
}
__device__ __forceinline__ int32_t rec_lit(uint64_t r) { return (int32_t)(r & 0x1FFFF); }
__device__ __forceinline__ int32_t rec_ml(uint64_t r) { return (int32_t)((r >> 17) & 0x1FFFF); }
__device__ __forceinline__ int32_t rec_off(uint64_t r) { return (int32_t)((r >> 34) & 0xFFFF); }
__device__ __forceinline__ int32_t rec_skip(uint64_t r) { return (int32_t)(r >> 50); }

// ---- arena: chunks of 512 slots (4 KiB); slots 0..503 hold records (an all-zero record does nothing), slot 504 the index of the
// block's next chunk ----
constexpr int CHUNK_SLOTS = 512;
constexpr int CHUNK_RECS = 504;  // (a multiple of 8: the parser writes records in 64-byte pieces; the link sits in slot 504)

struct BlockMeta {  // per block, written by the parser
    int32_t firstChunk;
    int32_t count;  // records to execute (0: nothing -- failed, empty or handed to the fallback decoder)
};

struct ArenaHeader {  // leads the scratch
    int32_t nextChunk;  // allocation cursor
    int32_t maxChunks;
    int32_t fallbackBlocks;  // blocks whose records did not fit: decoded by the ring decoder afterwards
    int32_t pad[61];
};
static_assert(offsetof(ArenaHeader, fallbackBlocks) == 4 * stats::ARENA_FALLBACK_BLOCKS, "achip_ctx_get_stat reads the word by that index (achip_stats.h)");

// the two-pass decoders' scratch: [header, 4 KiB][meta n x 8][only n x 4][arena, 4 KiB aligned]
struct TwoPassLayout {
    ArenaHeader* hdr;
    BlockMeta* meta;
    int32_t* only;      // per block: 1 = its records did not fit, the ring decoder takes it
    uint64_t* arena;
    int32_t maxChunks;  // what of `scratchBytes` lies behind the fixed part, in chunks (one to spare: the executor's unconditional record loads)
    static int64_t fixed(int32_t nBlocks) { return 4096 + (((int64_t)nBlocks * 12 + 4095) & ~4095LL); }
    TwoPassLayout(void* scratch, int64_t scratchBytes, int32_t nBlocks)
    {
        uint8_t* s = (uint8_t*)scratch;
        hdr = (ArenaHeader*)s;
        meta = (BlockMeta*)(s + 4096);
        only = (int32_t*)(s + 4096 + (int64_t)nBlocks * 8);
        arena = (uint64_t*)(s + fixed(nBlocks));
        const int64_t chunks = (scratchBytes - fixed(nBlocks)) / (CHUNK_SLOTS * 8) - 1;
        maxChunks = (int32_t)(chunks > 0x7FFFFFFF ? 0x7FFFFFFF : chunks);
    }
};

// ---- wave helpers (DPP on the device, shuffles under tools/hostemu) ---------------------------------------------------------------
__device__ __forceinline__ int32_t wave_scan_incl(int32_t x, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t t;
    t = __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);  // row_shr:1
    x += t;
    t = __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);  // row_shr:2
    x += t;
    t = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);  // row_shr:4
    x += t;
    t = __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);  // row_shr:8
    x += t;
    const int32_t r0 = __builtin_amdgcn_readlane(x, 15), r1 = __builtin_amdgcn_readlane(x, 31), r2 = __builtin_amdgcn_readlane(x, 47);
    return x + (lane >= 16 ? r0 : 0) + (lane >= 32 ? r1 : 0) + (lane >= 48 ? r2 : 0);
#else
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t t = __shfl_up(x, d);
        if (lane >= d) x += t;
    }
    return x;
#endif
}
__device__ __forceinline__ int32_t wave_bcast(int32_t v, int srcLane) { return __builtin_amdgcn_readlane(v, srcLane); }
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int srcLane)  // (uniform srcLane)
{
    return ((uint64_t)(uint32_t)wave_bcast((int32_t)(v >> 32), srcLane) << 32) | (uint32_t)wave_bcast((int32_t)(uint32_t)v, srcLane);
}
__device__ __forceinline__ const uint8_t* wave_bcast_ptr(const uint8_t* p, int srcLane)
{
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)wave_bcast((int32_t)(uint32_t)v, srcLane), hi = (uint32_t)wave_bcast((int32_t)(v >> 32), srcLane);
    return (const uint8_t*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// ---- the parser's view of its compressed stream: a byte-addressable LDS ring per lane, fed by loads that are in flight for NS trips -----
// RING bytes of the stream are resident per lane, contiguous in LDS (the first 16 bytes once more behind the ring, so that any resident
// 16 bytes [v, v + 16) can be read at ring + (v % RING) without a wrap case), fed with aligned 32-byte granules.
// The point of the structure is WHEN the loads are waited for.  A wavefront's vector memory operations complete in order and are waited
// for by count, so a lane that refilled "when it ran dry, one piece ahead" made the whole wavefront wait for the load some other lane
// had issued a moment ago: one memory latency per trip (measured: 2.1 us per trip of ~200 instructions).  Here every trip has ONE place
// where granules are requested (`issue`, slot = trip mod NS) and ONE place where the granule requested NS trips earlier enters the ring
// (`land`, same slot): the loop is unrolled, the slots are distinct registers, and the wait the compiler places before `land` lets the
// NS - 1 younger requests stay in flight.  A lane whose bytes are not resident yet sits the trip out.
// "Virtual" positions count from the 32-byte aligned address at or before the stream's first byte.
template <int NS>
struct LaneFeed {
    static constexpr int RING = 128;
    static constexpr int GRAN = 32;
    static constexpr int STRIDE = RING + 16;  // (a multiple of 16: the granules are written as aligned 16-byte pieces)
    uint8_t* ring;
    const uint8_t* inAligned;
    const uint8_t* safe;  // what a lane that wants nothing loads from (the load itself is unconditional, see issue)
    int32_t inBase;    // virtual position of the stream's first byte (0..31)
    int32_t lastV;     // virtual position of the last 16-byte piece that holds a byte of the stream
    int32_t loadedV;   // (a multiple of 32) the ring holds virtual [.., loadedV)
    int32_t issueV;    // the next granule to request; loadedV + 32 * (granules in flight)
    u32x4 ga[NS], gb[NS];
    uint32_t validBits;  // bit s: slot s holds a granule of this lane (flags live in vector registers: no lane-mask bookkeeping at branches)

    // `anywhere`: an address (16-byte aligned, 16 bytes) that can always be read
    __device__ __forceinline__ void init(uint8_t* lds, int lane, const uint8_t* in, int32_t inLimit, const void* anywhere)
    {
        ring = lds + lane * STRIDE;
        inBase = (int32_t)((uintptr_t)in & (GRAN - 1));
        // (an empty payload has no byte of its own to anchor the granule loads at: `in` may be the first byte BEHIND the item, and on a
        // 32-byte boundary the piece at `in` then lies outside everything the caller handed over -- such a stream reads `anywhere`)
        inAligned = inLimit > 0 ? in - inBase : (const uint8_t*)anywhere;
        lastV = inLimit > 0 ? ((inLimit + inBase - 1) & ~15) : 0;
        safe = (const uint8_t*)anywhere;
        loadedV = 0;
        issueV = 0;
        validBits = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            ga[s] = u32x4{0, 0, 0, 0};
            gb[s] = u32x4{0, 0, 0, 0};
        }
    }
    // the granule requested NS trips ago enters the ring
    template <int SLOT>
    __device__ __forceinline__ void land()
    {
        const uint32_t have = (validBits >> SLOT) & 1u;
        const int32_t slot = loadedV & (RING - 1);
        if (have != 0) {  // (only stores inside the branch: no state to merge behind it)
            *(u32x4*)(ring + slot) = ga[SLOT];
            *(u32x4*)(ring + slot + 16) = gb[SLOT];
            if (slot == 0) {
                *(u32x4*)(ring + RING) = ga[SLOT];
            }
        }
        loadedV += have != 0 ? GRAN : 0;
        validBits &= ~(1u << SLOT);
    }
    // Requests the next granule if the ring has room for it behind virtual position v (everything below v is consumed).  The load
    // instructions are executed by every lane on every trip -- lanes that want nothing read `safe`, all the same address -- so that the
    // compiler can count: with a request on every trip, "all but the NS - 1 youngest have completed" is what `land` has to wait for.  (A
    // request under a branch makes that count unknown and every wait a wait for everything.)  A 16-byte piece is read whole even where
    // the stream starts or ends inside it: the bytes around the stream lie in the same aligned 16 bytes, hence on the same page, and no
    // parse decision looks at them (positions at or beyond the stream's end only ever reach the general path, which reads the stream
    // itself).  Pieces entirely beyond the end repeat the last one.
    template <int SLOT>
    __device__ __forceinline__ void issue(int32_t v, bool active)
    {
        const bool want = active && issueV + GRAN - RING <= v;
        const int32_t a0 = issueV < lastV ? issueV : lastV;
        const int32_t a1 = issueV + 16 < lastV ? issueV + 16 : lastV;
        const uint8_t* p0 = want ? inAligned + a0 : safe;
        const uint8_t* p1 = want ? inAligned + a1 : safe;
        ga[SLOT] = *(const u32x4*)p0;
        gb[SLOT] = *(const u32x4*)p1;
        validBits |= want ? (1u << SLOT) : 0u;
        issueV += want ? GRAN : 0;
    }
    // the stream continues at virtual position v, beyond everything requested so far: what is in flight is dropped
    __device__ __forceinline__ void restart(int32_t v, bool doIt = true)
    {
        loadedV = doIt ? (v & ~(GRAN - 1)) : loadedV;
        issueV = doIt ? loadedV : issueV;
        validBits = doIt ? 0u : validBits;
    }
    __device__ __forceinline__ bool resident(int32_t v, int32_t n) const { return v + n <= loadedV; }
    __device__ __forceinline__ uint32_t rd32(int32_t v) const
    {
        uint32_t x;
        __builtin_memcpy(&x, ring + (v & (RING - 1)), 4);
        return x;
    }
};

// largest multiple of off (1..65535) that is <= x (off <= x <= 65535)
__device__ __forceinline__ int32_t largest_multiple(int32_t off, int32_t x)
{
    int32_t m = (int32_t)((float)x / (float)off);  // within one of the quotient (both below 2^24: exact operands)
    m -= m * off > x ? 1 : 0;
    m += (m + 1) * off <= x ? 1 : 0;
    return m * off;
}

// ---- pieces: a sequence (lit literal bytes, then ml match bytes at offset off) is cut into records of at most 16 literal + 16 match bytes.
// Pieces 0 .. litFull - 1 are 16 literal bytes each, piece litFull holds the rest of the literals (1..16, or 0 when there are none) and
// the match's first 16 bytes, the pieces behind it 16 match bytes each.  A match's later pieces name the largest multiple of its offset
// that stays inside the match's periodic source region [start - offset, ..): the same bytes, but never the output of the piece before
// (no chains of dependent pieces). ----
__device__ __forceinline__ int32_t lit_full(int32_t lit) { return lit > 16 ? (lit + 15) / 16 - 1 : 0; }
__device__ __forceinline__ int32_t piece_count(int32_t lit, int32_t ml) { return lit_full(lit) + 1 + (ml > 16 ? (ml - 16 + 15) / 16 : 0); }
// piece k (< piece_count) of the sequence: pl literal bytes, pm match bytes at offset o.  (off > 0 wherever o is used -- pm > 0 --: the
// guard only keeps the division defined for a sequence without a match)
__device__ __forceinline__ void cut_piece(int32_t lit, int32_t ml, int32_t off, int32_t litFull, int32_t k, int32_t& pl, int32_t& pm, int32_t& o)
{
    o = off;
    if (k < litFull) {
        pl = 16;
        pm = 0;
    }
    else if (k == litFull) {
        pl = lit - 16 * litFull;
        pm = ml < 16 ? ml : 16;
    }
    else {
        const int32_t m = k - litFull;  // match pieces before this one
        pl = 0;
        pm = ml - 16 * m < 16 ? ml - 16 * m : 16;
        const int32_t xm = 16 * m + off;
        o = largest_multiple(off > 0 ? off : 1, xm < 65535 ? xm : 65535);
    }
}
// ... as a record; skip0: the compressed bytes in front of the sequence's literals (the first piece carries them)
__device__ __forceinline__ uint64_t piece_record(int32_t lit, int32_t ml, int32_t off, int32_t litFull, int32_t k, int32_t skip0)
{
    int32_t pl, pm, o;
    cut_piece(lit, ml, off, litFull, k, pl, pm, o);
    return rec_pack((uint32_t)pl, (uint32_t)pm, pm > 0 ? (uint32_t)o : 0u, k == 0 ? (uint32_t)skip0 : 0u);
}

// What the lanes of a lane-per-block parser that request nothing read (LaneFeed's `anywhere`): one address per WAVEFRONT (one request per
// load instruction, hot in this CU's L1) -- the start of the first non-empty stream of the wavefront, `fallback` when all are empty; a
// single address for the whole grid would queue every wavefront of the chip at one L2 channel.
__device__ __forceinline__ const uint8_t* idle_address(const uint8_t* srcBase, const uint8_t* in, int32_t inLimit, const void* fallback)
{
    const unsigned long long nonEmpty = __ballot(inLimit > 0);
    const uint8_t* anywhere = (const uint8_t*)fallback;
    if (nonEmpty != 0) {  // (uniform)
        // (an offset from the batch's base travels, not a pointer: the loads stay global_load, not flat_load)
        anywhere = srcBase + (int64_t)shfl_u64((uint64_t)((in - srcBase) - (int64_t)((uintptr_t)in & 31)), __builtin_ctzll(nonEmpty));
    }
    return anywhere;
}

// ---- the record output of a lane-per-block parser: exactly one record per lane and trip (an empty one when there is nothing to say),
// eight trips to a 64-byte piece, kept in registers; the pieces go to 4 KiB chunks of the arena ----
struct LaneRecordSink {
    int32_t firstChunk, chunk, fill, count;
    __device__ __forceinline__ void init()
    {
        firstChunk = -1;
        chunk = -1;
        fill = CHUNK_RECS;
        count = 0;
    }
    // the group of eight leaves: a chunk for every lane that needs one (one atomic per wavefront), then one 64-byte piece per lane.
    // Called by the whole wavefront; groupAny: the group holds a record of this lane.
    __device__ __forceinline__ void flush(ArenaHeader* hdr, uint64_t* arena, int32_t maxChunks, int lane, const uint64_t (&rec)[8], int32_t groupAny, int32_t& fallback,
                                          int32_t& finished)
    {
        const bool flush = groupAny != 0 && fallback == 0;
        const bool need = flush && fill == CHUNK_RECS;
        const unsigned long long nm = __ballot(need);
        if (nm != 0) {  // (uniform)
            int32_t base = 0;
            if (lane == __builtin_ctzll(nm)) {
                base = atomicAdd(&hdr->nextChunk, (int32_t)__popcll(nm));
            }
            base = wave_bcast(base, __builtin_ctzll(nm));
            if (need) {
                const int32_t c = base + (int32_t)__popcll(nm & ((1ull << lane) - 1));
                if (c >= maxChunks) {  // the arena is exhausted: the ring decoder takes the block
                    fallback = 1;
                    finished = 1;
                }
                else {
                    if (chunk >= 0) {
                        arena[(int64_t)chunk * CHUNK_SLOTS + CHUNK_RECS] = (uint64_t)(uint32_t)c;  // link
                    }
                    else {
                        firstChunk = c;
                    }
                    chunk = c;
                    fill = 0;
                }
            }
        }
        if (flush && fallback == 0) {
            uint8_t* const dst = (uint8_t*)(arena + (int64_t)chunk * CHUNK_SLOTS + fill);
#pragma unroll
            for (int k = 0; k < 8; k += 2) {
                st16(dst + 8 * k, u32x4{(uint32_t)rec[k], (uint32_t)(rec[k] >> 32), (uint32_t)rec[k + 1], (uint32_t)(rec[k + 1] >> 32)});
            }
            fill += 8;
            count += 8;
        }
    }
};

// A parsed block's results, by the one lane that holds them: a block whose records did not fit (or cannot be expressed) goes to the ring
// decoder (`only`), any other gets its record chain and -- the parse pass decides them -- output length, status and error offset.
__device__ __forceinline__ void finish_block(const BatchArgs& a, ArenaHeader* hdr, BlockMeta* meta, int32_t* only, int64_t block, bool fallback, int32_t firstChunk, int32_t count,
                                             int32_t st, int32_t eo, int32_t op)
{
    if (fallback) {
        only[block] = 1;
        meta[block].firstChunk = 0;
        meta[block].count = 0;
        atomicAdd(&hdr->fallbackBlocks, 1);
    }
    else {
        only[block] = 0;
        meta[block].firstChunk = firstChunk < 0 ? 0 : firstChunk;
        meta[block].count = st == 0 ? count : 0;
        a.outLen[block] = st == 0 ? op : 0;
        a.status[block] = st;
        a.errOffset[block] = (int64_t)eo;
    }
}

}  // namespace sx
}  // namespace achip
