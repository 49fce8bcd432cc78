// achip_enc_wave.h -- what the window encoders of one wavefront share (lz4_compress_mw.h, snappy_compress_mw.h, zstd_dfast_mw.h and the batch-probe
// bodies they grew out of): lane reads, lane masks and "match any".  Codec-specific helpers stay with their encoder.
#pragma once
#include "achip_device.h"

namespace achip {

__device__ __forceinline__ uint32_t rl32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, int src) { return ((uint64_t)rl32((uint32_t)(v >> 32), src) << 32) | rl32((uint32_t)v, src); }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
}
// bits [lo, hi) of a 64-bit mask (0 <= lo, hi <= 64; empty when hi <= lo)
__device__ __forceinline__ uint64_t bits(int lo, int hi)
{
    const uint64_t upTo = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
    const uint64_t below = lo >= 64 ? ~0ull : ((1ull << lo) - 1ull);
    return upTo & ~below;
}
// The same for WAVE-UNIFORM lo <= hi with hi - lo <= 63 (the masks of the LZ4 and Snappy replays), in one scalar instruction: `bits` compiles to a
// dozen (two 64-bit shifts with their >= 64 cases, subtractions, selects), twice per sequence, in kernels whose time IS their scalar instructions -- 6.0e10
// of them against 2.1e10 vector instructions per launch on the corpus batch, one scalar unit per CU (profiles/r06_counters_lz4_compress_corpus.txt).
__device__ __forceinline__ uint64_t sbits(int lo, int hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t m;
    asm("s_bfm_b64 %0, %1, %2" : "=s"(m) : "s"(hi - lo), "s"(lo));
    return m;
#else
    return bits(lo, hi);
#endif
}

// ---- wave-wide "match any": for every lane, the mask of lanes whose `key` (low `keyBits` bits) equals its own --------
// A ballot + a select/and per bit; used to replay the hash-table updates of a batch of probes, or of a window, in program order.
__device__ __forceinline__ unsigned long long wave_match_any(uint32_t key, int keyBits, unsigned long long active)
{
    unsigned long long eq = active;
    for (int b = 0; b < keyBits; b++) {
        const bool bit = (key >> b) & 1u;
        const unsigned long long m = __ballot(bit);
        eq &= bit ? m : ~m;
    }
    return eq;
}

// ---- the window replays of LZ4 and Snappy (lz4_compress_mw.h has the scheme): lane l holds the 8 bytes `x` at `pos` = base + l, x4 its low word ----

// the window's load: the 8 bytes at `pos` where the block (`limit` bytes) has them, their hash, the table's entry of that hash as the window finds it, and
// the lanes of the window with the same hash
struct WindowLoad {
    uint64_t x;
    int32_t h;
    int32_t tc;
    unsigned long long same;
    bool canLoad;
};
template <typename TableT, typename Hash>
__device__ __forceinline__ WindowLoad window_load(const uint8_t* in, int32_t pos, int32_t limit, const TableT* table, int hashBits, Hash hash)
{
    const bool canLoad = pos + 8 <= limit;
    uint64_t x = 0;
    int32_t h = 0;
    int32_t tc = 0;
    if (canLoad) {
        x = ld8(in + pos);
        h = hash(x);
        tc = (int32_t)table[h];
    }
    const unsigned long long loadMask = __ballot(canLoad);
    return {x, h, tc, wave_match_any((uint32_t)h, hashBits, loadMask) & loadMask, canLoad};
}

// literal bytes [from, to) of the window, stored at out + at straight from the lanes' registers (a literal byte is the low byte of its lane's word)
__device__ __forceinline__ void window_store_literals(uint8_t* out, int32_t at, int32_t from, int32_t to, int32_t pos, uint32_t x4)
{
    if (pos >= from && pos < to) {
        out[at + (pos - from)] = (uint8_t)x4;
    }
}

// `count` from a0 against b0 up to `limit` when the first 8 bytes of both sides (a8, b8) are in registers: memory only for what lies behind 8 equal bytes
__device__ __forceinline__ int32_t window_count8(const uint8_t* in, uint64_t a8, uint64_t b8, int32_t a0, int32_t b0, int32_t limit, int lane)
{
    const int32_t limitLen = limit - a0;
    const uint64_t d = a8 ^ b8;
    int32_t eq = d == 0 ? 8 : (int32_t)(__builtin_ctzll(d) >> 3);
    eq = eq < limitLen ? eq : limitLen;
    if (eq == 8 && limitLen > 8) {
        return 8 + wave_count(in, a0 + 8, b0 + 8, limit, lane);
    }
    return eq;
}

// the end of a window: the table takes the latest inserted lane (mask M) of every hash (`same`: the lanes with this lane's hash h)
template <typename TableT>
__device__ __forceinline__ void window_commit_table(TableT* table, int32_t h, int32_t pos, bool canLoad, unsigned long long same, unsigned long long M, int lane)
{
    const unsigned long long later = same & M & ~((2ull << lane) - 1ull);
    if (canLoad && ((M >> lane) & 1ull) != 0 && later == 0) {
        table[h] = (TableT)pos;
    }
}

}  // namespace achip
