// achip_xxh_stream.h -- hasher states that live in device memory between calls (xxhash_stream.hip): the records, the launchers, and the
// pieces of XXH3 / XXH64 / XXH32 that resume from a record.  The one-shot routines' mechanisms are used as they are (achip_xxh3.h:
// stripe_part, stripe_sum, scramble, short_hash, LaneKey); what is added here is what a resumed stream needs -- a LaneKey read from the
// record's seeded secret instead of a kernel argument, a span of stripes that begins and ends anywhere in a 1 KiB block, and eight
// bytes read across the seam between two buffers.  (The Zstd stream writer keeps its own Xxh64Stream in achip_xxhash.h, seed 0 and a
// wavefront per stream: untouched.)
#pragma once
#include "achip_xxh3.h"

namespace achip {

constexpr int32_t HASH_XXH32 = 0, HASH_XXH64 = 1, HASH_XXH3_64 = 2, HASH_XXH3_128 = 3;

// ---- the records (opaque to callers: achip_hash_state_size; each a multiple of 16 bytes) ----
struct Xxh32State {
    uint32_t v[4];
    uint64_t total;
    uint32_t seed;
    int32_t bufLen;   // 0..15
    uint8_t buf[16];  // the pending stripe
};
struct Xxh64State {
    uint64_t v[4];
    uint64_t total;
    uint64_t seed;
    int32_t bufLen;  // 0..31
    int32_t pad0;
    uint8_t buf[32];
    uint64_t pad1;
};
// XXH3-64 and XXH3-128 share the record and the update; only the digest differs
struct Xxh3State {
    uint64_t acc[8];
    uint64_t total;
    uint64_t seed;
    int32_t bufLen;       // 0..256: bytes absorbed and not yet consumed (at least one once anything was consumed: the stream's last stripe is never consumed early)
    int32_t stripes;      // 0..15: stripes consumed of the stream's current 1 KiB block
    uint8_t buf[256];
    uint8_t last[64];     // the 64 bytes of the stream in front of buf (valid once anything was consumed): the last stripe when bufLen < 64
    uint8_t secret[192];  // the seeded secret (word 2i + seed, word 2i+1 - seed)
    uint64_t pad;
};
static_assert(sizeof(Xxh32State) == 48 && sizeof(Xxh64State) == 96 && sizeof(Xxh3State) == 608, "record sizes are part of the launch arithmetic");

constexpr int32_t XXH3_BUF = 256;
constexpr int32_t XXH3_LANE_MAX = 256;  // pieces up to here are absorbed by one lane (at most 8 stripes complete), longer ones by a wavefront

inline int64_t hash_state_size(int32_t algo)
{
    return algo == HASH_XXH32 ? (int64_t)sizeof(Xxh32State) : (algo == HASH_XXH64 ? (int64_t)sizeof(Xxh64State) : ((algo == HASH_XXH3_64 || algo == HASH_XXH3_128) ? (int64_t)sizeof(Xxh3State) : -1));
}
hipError_t launch_hash_states_reset(int32_t algo, void* states, int32_t n, uint64_t seed, hipStream_t stream);
hipError_t launch_hash_states_update(int32_t algo, void* states, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, hipStream_t stream);
hipError_t launch_hash_states_digest(int32_t algo, const void* states, int64_t* out, int32_t n, hipStream_t stream);

namespace xxs {

// 8 / 4 bytes at offset `off` of the bytes a[0, aLen) followed by b[...]
__device__ __forceinline__ uint64_t ld8_seam(const uint8_t* a, int32_t aLen, const uint8_t* b, int32_t off)
{
    if (off + 8 <= aLen) return ld8(a + off);
    if (off >= aLen) return ld8(b + (off - aLen));
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)(off + i < aLen ? a[off + i] : b[off + i - aLen]) << (8 * i);
    return v;
}
__device__ __forceinline__ uint32_t ld4_seam(const uint8_t* a, int32_t aLen, const uint8_t* b, int32_t off)
{
    if (off + 4 <= aLen) return ld4(a + off);
    if (off >= aLen) return ld4(b + (off - aLen));
    uint32_t v = 0;
    for (int i = 0; i < 4; i++) v |= (uint32_t)(off + i < aLen ? a[off + i] : b[off + i - aLen]) << (8 * i);
    return v;
}
// n bytes by the calling lane (exact: nothing outside [src, src + n) / [dst, dst + n) is touched)
__device__ __forceinline__ void lane_copy(uint8_t* dst, const uint8_t* src, int32_t n)
{
    int32_t i = 0;
    for (; i + 8 <= n; i += 8) st8(dst + i, ld8(src + i));
    for (; i < n; i++) dst[i] = src[i];
}

// ---- XXH3 by ONE lane (short pieces, the digest): the eight accumulators in registers ----
__device__ __forceinline__ void lane_stripe_words(uint64_t (&acc)[8], const uint64_t (&x)[8], const uint8_t* key)
{
#pragma unroll
    for (int j = 0; j < 4; j++) xxh3::stripe_part(x[2 * j], x[2 * j + 1], xxh3::rd64(key + 16 * j), xxh3::rd64(key + 16 * j + 8), acc[2 * j], acc[2 * j + 1]);
}
__device__ __forceinline__ void lane_stripe(uint64_t (&acc)[8], const uint8_t* p, const uint8_t* key)
{
    uint64_t x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = ld8(p + 8 * j);
    lane_stripe_words(acc, x, key);
}
// nStripes stripes at p, the first being stripe `sib` of its block; a block's sixteenth stripe is followed by the scramble
__device__ __forceinline__ void lane_consume(uint64_t (&acc)[8], int32_t& sib, const uint8_t* p, int32_t nStripes, const uint8_t* secret)
{
    for (int32_t k = 0; k < nStripes; k++) {
        lane_stripe(acc, p + 64 * k, secret + 8 * sib);
        if (++sib == 16) {
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] = xxh3::scramble(acc[j], xxh3::rd64(secret + 128 + 8 * j));
            sib = 0;
        }
    }
}

// ---- XXH3 by a WAVEFRONT: lane L owns words 2(L%4), 2(L%4)+1 of stripe L/4 of the BLOCK, wherever in the block a span begins ----
// the lane's block and scramble words from the record's secret (the words LaneKey names k0, k1, s0, s1; the digest is a lane's and reads
// the last-stripe and merge words itself)
__device__ __forceinline__ xxh3::LaneKey lane_key_of(const uint8_t* secret, int lane)
{
    const int w = 2 * (lane & 3), s = lane >> 2;
    xxh3::LaneKey k;
    k.k0 = xxh3::rd64(secret + 8 * (s + w));
    k.k1 = xxh3::rd64(secret + 8 * (s + w + 1));
    k.s0 = xxh3::rd64(secret + 8 * (16 + w));
    k.s1 = xxh3::rd64(secret + 8 * (17 + w));
    k.l0 = k.l1 = k.m0 = k.m1 = k.h0 = k.h1 = 0;
    return k;
}
// `blocks` whole blocks at p (p + 16 * lane is the lane's column), each followed by its scramble: the loop of long_hash_wave, four blocks'
// loads in flight while the four before them are summed
__device__ __forceinline__ void wave_blocks(const uint8_t* __restrict__ lp, int32_t blocks, const xxh3::LaneKey& k, uint64_t& a0, uint64_t& a1)
{
    constexpr int UNROLL = 4;
    int32_t b = 0;
    uint64_t x[UNROLL][2];
    if (blocks >= UNROLL) {
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            x[u][0] = ld8(lp + ((int64_t)u << 10));
            x[u][1] = ld8(lp + ((int64_t)u << 10) + 8);
        }
    }
    for (; b + UNROLL <= blocks; b += UNROLL) {
        const bool more = b + 2 * UNROLL <= blocks;
        uint64_t y[UNROLL][2];
        if (more) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                y[u][0] = ld8(lp + ((int64_t)(b + UNROLL + u) << 10));
                y[u][1] = ld8(lp + ((int64_t)(b + UNROLL + u) << 10) + 8);
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            uint64_t c0 = 0, c1 = 0;
            xxh3::stripe_part(x[u][0], x[u][1], k.k0, k.k1, c0, c1);
            a0 = xxh3::scramble(a0 + xxh3::stripe_sum(c0), k.s0);
            a1 = xxh3::scramble(a1 + xxh3::stripe_sum(c1), k.s1);
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                x[u][0] = y[u][0];
                x[u][1] = y[u][1];
            }
        }
    }
    for (; b < blocks; b++) {
        uint64_t c0 = 0, c1 = 0;
        xxh3::stripe_part(ld8(lp + ((int64_t)b << 10)), ld8(lp + ((int64_t)b << 10) + 8), k.k0, k.k1, c0, c1);
        a0 = xxh3::scramble(a0 + xxh3::stripe_sum(c0), k.s0);
        a1 = xxh3::scramble(a1 + xxh3::stripe_sum(c1), k.s1);
    }
}
// nStripes stripes at p, the first being stripe `sib` of the stream's block (wave-uniform arguments): the rest of that block with the lanes
// outside it masked, whole blocks, and the head of the block the span ends in
__device__ __forceinline__ void wave_span(const uint8_t* __restrict__ p, int64_t nStripes, int32_t& sib, const xxh3::LaneKey& k, int lane, uint64_t& a0, uint64_t& a1)
{
    while (nStripes > 0) {
        if (sib == 0 && nStripes >= 16) {
            const int64_t blocks = nStripes >> 4;
            wave_blocks(p + 16 * lane, (int32_t)blocks, k, a0, a1);
            p += blocks << 10;
            nStripes -= blocks << 4;
            continue;
        }
        const int32_t take = nStripes < 16 - sib ? (int32_t)nStripes : 16 - sib;
        const int32_t s = lane >> 2;
        uint64_t c0 = 0, c1 = 0;
        if (s >= sib && s < sib + take) {
            const uint8_t* q = p + 64 * (s - sib) + 16 * (lane & 3);
            xxh3::stripe_part(ld8(q), ld8(q + 8), k.k0, k.k1, c0, c1);
        }
        a0 += xxh3::stripe_sum(c0);
        a1 += xxh3::stripe_sum(c1);
        sib += take;
        if (sib == 16) {
            a0 = xxh3::scramble(a0, k.s0);
            a1 = xxh3::scramble(a1, k.s1);
            sib = 0;
        }
        p += 64 * take;
        nStripes -= take;
    }
}

}  // namespace xxs

}  // namespace achip
