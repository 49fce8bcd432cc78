// achip_xxh3.h -- XXH3-64 / XXH3-128 (xxHash 0.8) on the device; used by xxhash3.hip (the batched hashers).
//
// Two roles.  A buffer of at most 240 bytes is hashed by ONE lane (xxh3_short: the 0 / 1-3 / 4-8 / 9-16 / 17-128 / 129-240 classes, the
// default secret and the seed as they are).  A longer buffer is hashed by a WAVEFRONT (xxh3_long_wave): within a 1 KiB block a stripe's
// contribution to the eight accumulators does not depend on the accumulators, so lane L loads 16 contiguous bytes of the block (words
// 2(L%4), 2(L%4)+1 of stripe L/4 -- the wavefront reads the block in one coalesced load), computes what they add to accumulators
// 2(L%4) and 2(L%4)+1 (XXH3 adds word i to accumulator i^1: both of a word pair stay on its lane), and the 16 stripes are summed over
// lane rotations by 4 and 8 within a row of 16 (DPP) and lane-xor 16 and 32.  Every lane then holds the two accumulators of its class L%4 and scrambles them itself: only the scramble
// between blocks is serial.  The long path reads its secret words from an Xxh3Key the host derives once per call (the seeded custom
// secret, with the unaligned words of the last stripe and of the merges already picked out).
#pragma once
#include "achip_device.h"

namespace achip {

namespace xxh3 {
constexpr uint64_t P32_1 = 0x9E3779B1u, P32_2 = 0x85EBCA77u, P32_3 = 0xC2B2AE3Du;
constexpr uint64_t P64_1 = 0x9E3779B185EBCA87ULL, P64_2 = 0xC2B2AE3D27D4EB4FULL, P64_3 = 0x165667B19E3779F9ULL, P64_4 = 0x85EBCA77C2B2AE63ULL,
                   P64_5 = 0x27D4EB2F165667C5ULL;
constexpr uint64_t MX1 = 0x165667919E3779F9ULL, MX2 = 0x9FB21C651E98DF25ULL;
constexpr int32_t SHORT_MAX = 240;  // longer inputs take the wavefront path

// the default secret (192 bytes), for the host (key derivation) and the device (short inputs)
#define ACHIP_XXH3_SECRET_BYTES                                                                                                            \
    {0xb8, 0xfe, 0x6c, 0x39, 0x23, 0xa4, 0x4b, 0xbe, 0x7c, 0x01, 0x81, 0x2c, 0xf7, 0x21, 0xad, 0x1c, 0xde, 0xd4, 0x6d, 0xe9, 0x83, 0x90, 0x97, 0xdb, \
     0x72, 0x40, 0xa4, 0xa4, 0xb7, 0xb3, 0x67, 0x1f, 0xcb, 0x79, 0xe6, 0x4e, 0xcc, 0xc0, 0xe5, 0x78, 0x82, 0x5a, 0xd0, 0x7d, 0xcc, 0xff, 0x72, 0x21, \
     0xb8, 0x08, 0x46, 0x74, 0xf7, 0x43, 0x24, 0x8e, 0xe0, 0x35, 0x90, 0xe6, 0x81, 0x3a, 0x26, 0x4c, 0x3c, 0x28, 0x52, 0xbb, 0x91, 0xc3, 0x00, 0xcb, \
     0x88, 0xd0, 0x65, 0x8b, 0x1b, 0x53, 0x2e, 0xa3, 0x71, 0x64, 0x48, 0x97, 0xa2, 0x0d, 0xf9, 0x4e, 0x38, 0x19, 0xef, 0x46, 0xa9, 0xde, 0xac, 0xd8, \
     0xa8, 0xfa, 0x76, 0x3f, 0xe3, 0x9c, 0x34, 0x3f, 0xf9, 0xdc, 0xbb, 0xc7, 0xc7, 0x0b, 0x4f, 0x1d, 0x8a, 0x51, 0xe0, 0x4b, 0xcd, 0xb4, 0x59, 0x31, \
     0xc8, 0x9f, 0x7e, 0xc9, 0xd9, 0x78, 0x73, 0x64, 0xea, 0xc5, 0xac, 0x83, 0x34, 0xd3, 0xeb, 0xc3, 0xc5, 0x81, 0xa0, 0xff, 0xfa, 0x13, 0x63, 0xeb, \
     0x17, 0x0d, 0xdd, 0x51, 0xb7, 0xf0, 0xda, 0x49, 0xd3, 0x16, 0x55, 0x26, 0x29, 0xd4, 0x68, 0x9e, 0x2b, 0x16, 0xbe, 0x58, 0x7d, 0x47, 0xa1, 0xfc, \
     0x8f, 0xf8, 0xb8, 0xd1, 0x7a, 0xd0, 0x31, 0xce, 0x45, 0xcb, 0x3a, 0x8f, 0x95, 0x16, 0x04, 0x28, 0xaf, 0xd7, 0xfb, 0xca, 0xbb, 0x4b, 0x40, 0x7e}

// The long path's secret words, derived on the host once per call from the seed (the custom secret: word 2i + seed, word 2i+1 - seed;
// seed 0 gives the default secret).  w: the 24 aligned words (stripe n of a block uses w[n..n+7], the scramble w[16..23]); last: the
// words at byte 121 (the last stripe); merge / merge128: the words at bytes 11 and 117 (the 64-bit merge, the 128-bit high half).
struct Key {
    uint64_t w[24];
    uint64_t last[8];
    uint64_t merge[8];
    uint64_t merge128[8];
};

__host__ __device__ __forceinline__ uint64_t rd64(const uint8_t* p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__host__ __device__ __forceinline__ uint32_t rd32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

inline void derive_key(uint64_t seed, Key* k)
{
    static const uint8_t kSecret[192] = ACHIP_XXH3_SECRET_BYTES;
    uint8_t s[192];
    for (int i = 0; i < 24; i++) {
        const uint64_t v = rd64(kSecret + 8 * i) + ((i & 1) ? 0 - seed : seed);
        __builtin_memcpy(s + 8 * i, &v, 8);
    }
    for (int i = 0; i < 24; i++) k->w[i] = rd64(s + 8 * i);
    for (int i = 0; i < 8; i++) {
        k->last[i] = rd64(s + 121 + 8 * i);
        k->merge[i] = rd64(s + 11 + 8 * i);
        k->merge128[i] = rd64(s + 117 + 8 * i);
    }
}

__device__ __forceinline__ uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
__device__ __forceinline__ uint64_t fold64(uint64_t a, uint64_t b) { return (a * b) ^ mulhi64(a, b); }
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t xxh64_avalanche(uint64_t h)
{
    h ^= h >> 33;
    h *= P64_2;
    h ^= h >> 29;
    h *= P64_3;
    return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t avalanche(uint64_t h)
{
    h ^= h >> 37;
    h *= MX1;
    return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t mix16(const uint8_t* p, const uint8_t* s, uint64_t seed)
{
    return fold64(ld8(p) ^ (rd64(s) + seed), ld8(p + 8) ^ (rd64(s + 8) - seed));
}
// XXH128_mix32B
__device__ __forceinline__ void mix32(uint64_t& lo, uint64_t& hi, const uint8_t* p1, const uint8_t* p2, const uint8_t* s, uint64_t seed)
{
    lo += mix16(p1, s, seed);
    lo ^= ld8(p2) + ld8(p2 + 8);
    hi += mix16(p2, s + 16, seed);
    hi ^= ld8(p1) + ld8(p1 + 8);
}

// XXH3 of [p, p + len), len <= 240, by the calling lane; `secret` is the default secret.  Returns the 64-bit hash in lo (WIDE = false)
// or the 128-bit hash in lo / hi (WIDE = true).
template <bool WIDE>
__device__ __forceinline__ void short_hash(const uint8_t* __restrict__ p, int32_t len, uint64_t seed, const uint8_t* __restrict__ secret, uint64_t& lo, uint64_t& hi)
{
    const uint64_t n = (uint64_t)len;
    if (len > 16) {
        if (!WIDE) {
            uint64_t acc = n * P64_1;
            if (len <= 128) {
                if (len > 32) {
                    if (len > 64) {
                        if (len > 96) {
                            acc += mix16(p + 48, secret + 96, seed) + mix16(p + len - 64, secret + 112, seed);
                        }
                        acc += mix16(p + 32, secret + 64, seed) + mix16(p + len - 48, secret + 80, seed);
                    }
                    acc += mix16(p + 16, secret + 32, seed) + mix16(p + len - 32, secret + 48, seed);
                }
                acc += mix16(p, secret, seed) + mix16(p + len - 16, secret + 16, seed);
                lo = avalanche(acc);
                return;
            }
            for (int i = 0; i < 8; i++) acc += mix16(p + 16 * i, secret + 16 * i, seed);
            acc = avalanche(acc);
            const int rounds = len >> 4;
            for (int i = 8; i < rounds; i++) acc += mix16(p + 16 * i, secret + 16 * (i - 8) + 3, seed);
            lo = avalanche(acc + mix16(p + len - 16, secret + 136 - 17, seed));
            return;
        }
        uint64_t a = n * P64_1, b = 0;
        if (len <= 128) {
            if (len > 32) {
                if (len > 64) {
                    if (len > 96) mix32(a, b, p + 48, p + len - 64, secret + 96, seed);
                    mix32(a, b, p + 32, p + len - 48, secret + 64, seed);
                }
                mix32(a, b, p + 16, p + len - 32, secret + 32, seed);
            }
            mix32(a, b, p, p + len - 16, secret, seed);
        }
        else {
            for (int i = 0; i < 4; i++) mix32(a, b, p + 32 * i, p + 32 * i + 16, secret + 32 * i, seed);
            a = avalanche(a);
            b = avalanche(b);
            const int rounds = len >> 5;
            for (int i = 4; i < rounds; i++) mix32(a, b, p + 32 * i, p + 32 * i + 16, secret + 3 + 32 * (i - 4), seed);
            mix32(a, b, p + len - 16, p + len - 32, secret + 136 - 17 - 16, 0 - seed);
        }
        lo = avalanche(a + b);
        hi = 0 - avalanche(a * P64_1 + b * P64_4 + (n - seed) * P64_2);
        return;
    }
    if (len > 8) {
        if (!WIDE) {
            const uint64_t x = ld8(p) ^ ((rd64(secret + 24) ^ rd64(secret + 32)) + seed);
            const uint64_t y = ld8(p + len - 8) ^ ((rd64(secret + 40) ^ rd64(secret + 48)) - seed);
            lo = avalanche(n + __builtin_bswap64(x) + y + fold64(x, y));
            return;
        }
        const uint64_t bl = (rd64(secret + 32) ^ rd64(secret + 40)) - seed, bh = (rd64(secret + 48) ^ rd64(secret + 56)) + seed;
        uint64_t y = ld8(p + len - 8);
        const uint64_t x = ld8(p) ^ y ^ bl;
        uint64_t mlo = x * P64_1, mhi = mulhi64(x, P64_1);
        mlo += (n - 1) << 54;
        y ^= bh;
        mhi += y + (uint64_t)(uint32_t)y * (P32_2 - 1);
        mlo ^= __builtin_bswap64(mhi);
        lo = avalanche(mlo * P64_2);
        hi = avalanche(mulhi64(mlo, P64_2) + mhi * P64_2);
        return;
    }
    if (len >= 4) {
        const uint64_t sd = seed ^ ((uint64_t)__builtin_bswap32((uint32_t)seed) << 32);
        const uint64_t first = ld4(p), last = ld4(p + len - 4);
        if (!WIDE) {
            uint64_t h = (last + (first << 32)) ^ ((rd64(secret + 8) ^ rd64(secret + 16)) - sd);
            h ^= rotl64(h, 49) ^ rotl64(h, 24);
            h *= MX2;
            h ^= (h >> 35) + n;
            h *= MX2;
            lo = h ^ (h >> 28);
            return;
        }
        const uint64_t x = (first + (last << 32)) ^ ((rd64(secret + 16) ^ rd64(secret + 24)) + sd);
        const uint64_t m = P64_1 + (n << 2);
        uint64_t mlo = x * m, mhi = mulhi64(x, m);
        mhi += mlo << 1;
        mlo ^= mhi >> 3;
        mlo ^= mlo >> 35;
        mlo *= MX2;
        lo = mlo ^ (mlo >> 28);
        hi = avalanche(mhi);
        return;
    }
    if (len > 0) {
        const uint32_t c = ((uint32_t)p[0] << 16) | ((uint32_t)p[len >> 1] << 24) | (uint32_t)p[len - 1] | ((uint32_t)len << 8);
        lo = xxh64_avalanche((uint64_t)c ^ ((uint64_t)(rd32(secret) ^ rd32(secret + 4)) + seed));
        if (WIDE) {
            const uint32_t ch = __builtin_bswap32(c);
            hi = xxh64_avalanche((uint64_t)((ch << 13) | (ch >> 19)) ^ ((uint64_t)(rd32(secret + 8) ^ rd32(secret + 12)) - seed));
        }
        return;
    }
    if (!WIDE) {
        lo = xxh64_avalanche(seed ^ rd64(secret + 56) ^ rd64(secret + 64));
        return;
    }
    lo = xxh64_avalanche(seed ^ rd64(secret + 64) ^ rd64(secret + 72));
    hi = xxh64_avalanche(seed ^ rd64(secret + 80) ^ rd64(secret + 88));
}

// a lane's words of the long path: the secret words of its word pair in every block, in the scramble, the last stripe and the merges
struct LaneKey {
    uint64_t k0, k1, s0, s1, l0, l1, m0, m1, h0, h1;
};
template <int N>
__device__ __forceinline__ uint64_t pick(const uint64_t (&w)[N], int idx)
{
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < N; j++) v = j == idx ? w[j] : v;  // (w is wave-uniform: selects, no indexed access to the kernel argument)
    return v;
}
__device__ __forceinline__ LaneKey lane_key(const Key& key, int lane)
{
    const int w = 2 * (lane & 3), s = lane >> 2;
    LaneKey k;
    k.k0 = pick(key.w, s + w);
    k.k1 = pick(key.w, s + w + 1);
    k.s0 = pick(key.w, 16 + w);
    k.s1 = pick(key.w, 17 + w);
    k.l0 = pick(key.last, w);
    k.l1 = pick(key.last, w + 1);
    k.m0 = pick(key.merge, w);
    k.m1 = pick(key.merge, w + 1);
    k.h0 = pick(key.merge128, w);
    k.h1 = pick(key.merge128, w + 1);
    return k;
}

// what the lane's 16 bytes (words x0, x1 of a stripe, keys k0, k1) add to its two accumulators
__device__ __forceinline__ void stripe_part(uint64_t x0, uint64_t x1, uint64_t k0, uint64_t k1, uint64_t& c0, uint64_t& c1)
{
    const uint64_t d0 = x0 ^ k0, d1 = x1 ^ k1;
    c0 += x1 + (uint64_t)(uint32_t)d0 * (d0 >> 32);
    c1 += x0 + (uint64_t)(uint32_t)d1 * (d1 >> 32);
}
// c + the value N lanes along the row of 16 (a DPP row rotation on the device: a VALU operand, no LDS round trip)
template <int N>
__device__ __forceinline__ uint64_t add_row_rotated(uint64_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)c, 0x120 + N, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(c >> 32), 0x120 + N, 0xF, 0xF, false);
    return c + (((uint64_t)hi << 32) | lo);
#else
    const int lane = (int)(threadIdx.x & 63);
    return c + (uint64_t)__shfl((unsigned long long)c, (lane & ~15) | ((lane + N) & 15));
#endif
}
// the sum over the 16 stripes: lanes of the same class L % 4 (rotations by 4 and 8 within the row, then lane-xor 16 and 32)
__device__ __forceinline__ uint64_t stripe_sum(uint64_t c)
{
    c = add_row_rotated<4>(c);
    c = add_row_rotated<8>(c);
    c += (uint64_t)__shfl_xor((unsigned long long)c, 16);
    c += (uint64_t)__shfl_xor((unsigned long long)c, 32);
    return c;
}
__device__ __forceinline__ uint64_t scramble(uint64_t a, uint64_t key)
{
    a ^= a >> 47;
    a ^= key;
    return a * P32_1;
}

// XXH3 of [p, p + len), len > 240, by the whole wavefront (uniform control flow; every lane returns the hash)
template <bool WIDE>
__device__ __forceinline__ void long_hash_wave(const uint8_t* __restrict__ p, int32_t len, const LaneKey& k, int lane, uint64_t& lo, uint64_t& hi)
{
    constexpr int UNROLL = 4;  // blocks whose loads are in flight together
    const int q = lane & 3;
    uint64_t a0 = q == 0 ? P32_3 : (q == 1 ? P64_2 : (q == 2 ? P64_4 : P64_5));
    uint64_t a1 = q == 0 ? P64_1 : (q == 1 ? P64_3 : (q == 2 ? P32_2 : P32_1));
    const int32_t blocks = (len - 1) >> 10;
    const uint8_t* lp = p + 16 * lane;
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
        // the next UNROLL blocks' loads go out before this group is summed (software pipelining: 2 x UNROLL KiB in flight)
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
            stripe_part(x[u][0], x[u][1], k.k0, k.k1, c0, c1);
            a0 = scramble(a0 + stripe_sum(c0), k.s0);
            a1 = scramble(a1 + stripe_sum(c1), k.s1);
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
        stripe_part(ld8(lp + ((int64_t)b << 10)), ld8(lp + ((int64_t)b << 10) + 8), k.k0, k.k1, c0, c1);
        a0 = scramble(a0 + stripe_sum(c0), k.s0);
        a1 = scramble(a1 + stripe_sum(c1), k.s1);
    }
    // the last (partial) block's whole stripes and the last 64 bytes (lanes 0..3), summed together: no scramble between them
    uint64_t c0 = 0, c1 = 0;
    const int32_t rest = ((len - 1) & 1023) >> 6;
    if ((lane >> 2) < rest) {
        stripe_part(ld8(lp + ((int64_t)blocks << 10)), ld8(lp + ((int64_t)blocks << 10) + 8), k.k0, k.k1, c0, c1);
    }
    if (lane < 4) {
        const uint8_t* t = p + len - 64 + 16 * lane;
        stripe_part(ld8(t), ld8(t + 8), k.l0, k.l1, c0, c1);
    }
    a0 += stripe_sum(c0);
    a1 += stripe_sum(c1);
    // merge: class q folds accumulators 2q, 2q+1; the four classes are summed over lane-xor 1 and 2
    uint64_t m = fold64(a0 ^ k.m0, a1 ^ k.m1);
    m += (uint64_t)__shfl_xor((unsigned long long)m, 1);
    m += (uint64_t)__shfl_xor((unsigned long long)m, 2);
    lo = avalanche((uint64_t)len * P64_1 + m);
    if (WIDE) {
        uint64_t h = fold64(a0 ^ k.h0, a1 ^ k.h1);
        h += (uint64_t)__shfl_xor((unsigned long long)h, 1);
        h += (uint64_t)__shfl_xor((unsigned long long)h, 2);
        hi = avalanche(~((uint64_t)len * P64_2) + h);
    }
}

}  // namespace xxh3

}  // namespace achip
