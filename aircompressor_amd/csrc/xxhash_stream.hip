// xxhash_stream.hip -- streaming XXH32 / XXH64 / XXH3-64 / XXH3-128 for gfx950: a batch of hasher states in device memory, and reset /
// update / digest kernels that resume from them (the reference's create(seed) / update / digest / reset of XxHash64Hasher.java:91-169,
// XxHash32Hasher.java, XxHash3Hasher.java, XxHash3Hasher128.java, for many streams per call).  The records are in achip_xxh_stream.h.
//
//   reset   a lane per state.
//   update  state i absorbs srcBase[srcOff[i] .. + srcLen[i]); srcLen[i] <= 0 leaves the state alone.
//           XXH64 / XXH32: a QUAD per state, as in the one-shot kernels (xxhash.hip) -- lane s owns accumulator s and reads word s of every
//             stripe, so the quad reads a stripe's 32 / 16 contiguous bytes per step, four steps in flight.  One kernel: a quad is the right shape for
//             short and long pieces alike (the accumulators are four serial chains; more lanes would idle).
//           XXH3: two kernels per call, each skipping the other's items, since the host does not see the lengths.  A piece of at most
//             XXH3_LANE_MAX bytes is a LANE's: it appends to the record's buffer, or completes at most eight stripes itself.  A longer piece
//             is a WAVEFRONT's (wavefront w looks after states [w*group, w*group + group), group from nStates alone): it tops the buffer up to
//             a stripe boundary and consumes it, runs to the next 1 KiB boundary of the STREAM, takes whole blocks a lane per 16 bytes, then
//             the whole stripes that remain, and keeps the tail (1..64 bytes: the stream's last stripe is never consumed before the digest).
//   digest  a lane per state; reads the record, never writes it.
// Roofline: HBM (read-once); algorithmic bytes = the pieces' lengths (+ the records, read and written once per update).
#include "achip_xxh_stream.h"
#include "achip_xxhash.h"

namespace achip {

namespace {

__constant__ uint8_t kStreamSecret[192] = ACHIP_XXH3_SECRET_BYTES;

struct UpdateArgs {
    uint8_t* __restrict__ states;
    const uint8_t* __restrict__ srcBase;
    const int64_t* __restrict__ srcOff;
    const int32_t* __restrict__ srcLen;
    int32_t n;
};

// ---- XXH64 / XXH32: what differs between the two (word size, rotations, primes, the tail's steps) ----
struct T64 {
    typedef uint64_t U;
    typedef Xxh64State State;
    static constexpr U P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL, P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
    static __device__ __forceinline__ U rotl(U x, int r) { return (x << r) | (x >> (64 - r)); }
    static __device__ __forceinline__ U mix(U cur, U v) { return rotl(cur + v * P2, 31) * P1; }
    static __device__ __forceinline__ U ld(const uint8_t* p) { return ld8(p); }
    static __device__ __forceinline__ U ld_seam(const uint8_t* a, int32_t aLen, const uint8_t* b, int32_t off) { return xxs::ld8_seam(a, aLen, b, off); }
};
struct T32 {
    typedef uint32_t U;
    typedef Xxh32State State;
    static constexpr U P1 = 0x9E3779B1u, P2 = 0x85EBCA77u, P3 = 0xC2B2AE3Du, P4 = 0x27D4EB2Fu, P5 = 0x165667B1u;
    static __device__ __forceinline__ U rotl(U x, int r) { return (x << r) | (x >> (32 - r)); }
    static __device__ __forceinline__ U mix(U cur, U v) { return rotl(cur + v * P2, 13) * P1; }
    static __device__ __forceinline__ U ld(const uint8_t* p) { return ld4(p); }
    static __device__ __forceinline__ U ld_seam(const uint8_t* a, int32_t aLen, const uint8_t* b, int32_t off) { return xxs::ld4_seam(a, aLen, b, off); }
};

template <class T>
__global__ __launch_bounds__(256) void quad_reset_kernel(uint8_t* __restrict__ states, int32_t n, typename T::U seed)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    typename T::State* st = (typename T::State*)(states + i * (int64_t)sizeof(typename T::State));
    st->v[0] = seed + T::P1 + T::P2;
    st->v[1] = seed + T::P2;
    st->v[2] = seed;
    st->v[3] = seed - T::P1;
    st->total = 0;
    st->seed = seed;
    st->bufLen = 0;
}

// lane s of the quad: accumulator s, word s of every stripe
template <class T>
__global__ __launch_bounds__(64) void quad_update_kernel(UpdateArgs a)
{
    typedef typename T::U U;
    constexpr int32_t W = (int32_t)sizeof(U), STRIPE = 4 * W;
    const int lane = threadIdx.x;
    const int s = lane & 3;
    const int64_t i = (int64_t)blockIdx.x * 16 + (lane >> 2);
    if (i >= a.n) {
        return;  // whole quads leave together
    }
    const int32_t n = a.srcLen[i];
    if (n <= 0) {
        return;
    }
    typename T::State* st = (typename T::State*)(a.states + i * (int64_t)sizeof(typename T::State));
    const uint8_t* __restrict__ p = a.srcBase + a.srcOff[i];
    const int32_t b = st->bufLen;
    if ((int64_t)b + n < STRIPE) {  // the pending stripe stays incomplete
        for (int32_t k = s; k < n; k += 4) {
            st->buf[b + k] = p[k];
        }
        quad_sync();  // (every lane of the quad has read bufLen)
        if (s == 0) {
            st->bufLen = b + n;
            st->total += (uint64_t)n;
        }
        return;
    }
    U v = st->v[s];
    int32_t at = 0;
    if (b > 0) {  // the pending stripe, completed by the piece's head: the lane's word of it lies in the buffer, in the piece or across
        v = T::mix(v, T::ld_seam(st->buf, b, p, W * s));
        at = STRIPE - b;
    }
    const int32_t stripes = (n - at) / STRIPE;
    const uint8_t* q = p + at + W * s;
    int32_t k = 0;
    for (; k + 4 <= stripes; k += 4) {
        const U x0 = T::ld(q + (int64_t)k * STRIPE), x1 = T::ld(q + (int64_t)(k + 1) * STRIPE), x2 = T::ld(q + (int64_t)(k + 2) * STRIPE), x3 = T::ld(q + (int64_t)(k + 3) * STRIPE);
        v = T::mix(v, x0);
        v = T::mix(v, x1);
        v = T::mix(v, x2);
        v = T::mix(v, x3);
    }
    for (; k < stripes; k++) {
        v = T::mix(v, T::ld(q + (int64_t)k * STRIPE));
    }
    at += stripes * STRIPE;
    quad_sync();  // (every lane of the quad has read the old pending bytes)
    for (int32_t j = s; j < n - at; j += 4) {
        st->buf[j] = p[at + j];
    }
    st->v[s] = v;
    if (s == 0) {
        st->bufLen = n - at;
        st->total += (uint64_t)n;
    }
}

__device__ __forceinline__ uint64_t digest_one(const Xxh64State* st)
{
    typedef T64 T;
    uint64_t hash;
    if (st->total >= 32) {
        const uint64_t v1 = st->v[0], v2 = st->v[1], v3 = st->v[2], v4 = st->v[3];
        hash = T::rotl(v1, 1) + T::rotl(v2, 7) + T::rotl(v3, 12) + T::rotl(v4, 18);
        hash = (hash ^ T::mix(0, v1)) * T::P1 + T::P4;
        hash = (hash ^ T::mix(0, v2)) * T::P1 + T::P4;
        hash = (hash ^ T::mix(0, v3)) * T::P1 + T::P4;
        hash = (hash ^ T::mix(0, v4)) * T::P1 + T::P4;
    }
    else {
        hash = st->seed + T::P5;
    }
    hash += st->total;
    const uint8_t* t = st->buf;
    const int32_t len = st->bufLen;
    int32_t index = 0;
    while (index <= len - 8) {
        hash = T::rotl(hash ^ T::mix(0, ld8(t + index)), 27) * T::P1 + T::P4;
        index += 8;
    }
    if (index <= len - 4) {
        hash = T::rotl(hash ^ ((uint64_t)ld4(t + index) * T::P1), 23) * T::P2 + T::P3;
        index += 4;
    }
    while (index < len) {
        hash = T::rotl(hash ^ ((uint64_t)t[index] * T::P5), 11) * T::P1;
        index++;
    }
    hash ^= hash >> 33;
    hash *= T::P2;
    hash ^= hash >> 29;
    hash *= T::P3;
    hash ^= hash >> 32;
    return hash;
}
__device__ __forceinline__ uint64_t digest_one(const Xxh32State* st)
{
    typedef T32 T;
    uint32_t hash;
    if (st->total >= 16) {
        hash = T::rotl(st->v[0], 1) + T::rotl(st->v[1], 7) + T::rotl(st->v[2], 12) + T::rotl(st->v[3], 18);
    }
    else {
        hash = st->seed + T::P5;
    }
    hash += (uint32_t)st->total;
    const uint8_t* t = st->buf;
    const int32_t len = st->bufLen;
    int32_t index = 0;
    while (index <= len - 4) {
        hash = T::rotl(hash + ld4(t + index) * T::P3, 17) * T::P4;
        index += 4;
    }
    while (index < len) {
        hash = T::rotl(hash + (uint32_t)t[index] * T::P5, 11) * T::P1;
        index++;
    }
    hash ^= hash >> 15;
    hash *= T::P2;
    hash ^= hash >> 13;
    hash *= T::P3;
    hash ^= hash >> 16;
    return (uint64_t)hash;  // (zero-extended)
}

template <class T>
__global__ __launch_bounds__(256) void quad_digest_kernel(const uint8_t* __restrict__ states, int32_t n, int64_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    out[i] = (int64_t)digest_one((const typename T::State*)(states + i * (int64_t)sizeof(typename T::State)));
}

// ---- XXH3 ----
__global__ __launch_bounds__(256) void xxh3_reset_kernel(uint8_t* __restrict__ states, int32_t n, uint64_t seed)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    Xxh3State* st = (Xxh3State*)(states + i * (int64_t)sizeof(Xxh3State));
    st->acc[0] = xxh3::P32_3;
    st->acc[1] = xxh3::P64_1;
    st->acc[2] = xxh3::P64_2;
    st->acc[3] = xxh3::P64_3;
    st->acc[4] = xxh3::P64_4;
    st->acc[5] = xxh3::P32_2;
    st->acc[6] = xxh3::P64_5;
    st->acc[7] = xxh3::P32_1;
    st->total = 0;
    st->seed = seed;
    st->bufLen = 0;
    st->stripes = 0;
    for (int w = 0; w < 24; w++) {
        st8(st->secret + 8 * w, xxh3::rd64(kStreamSecret + 8 * w) + ((w & 1) ? 0 - seed : seed));
    }
}

__global__ __launch_bounds__(256) void xxh3_update_lane_kernel(UpdateArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) {
        return;
    }
    const int32_t n = a.srcLen[i];
    if (n <= 0 || n > XXH3_LANE_MAX) {
        return;
    }
    Xxh3State* st = (Xxh3State*)(a.states + i * (int64_t)sizeof(Xxh3State));
    const uint8_t* __restrict__ p = a.srcBase + a.srcOff[i];
    const int32_t b = st->bufLen;
    st->total += (uint64_t)n;
    if (b + n <= XXH3_BUF) {
        xxs::lane_copy(st->buf + b, p, n);
        st->bufLen = b + n;
        return;
    }
    // (b >= 1 and b + n > 256 from here on) top the buffer up to a stripe boundary, consume it, then the piece's whole stripes short of its
    // last byte; 1..64 bytes stay
    uint64_t acc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = st->acc[j];
    int32_t sib = st->stripes;
    const int32_t t = (0 - b) & 63;
    xxs::lane_copy(st->buf + b, p, t);
    const int32_t filled = b + t;
    xxs::lane_consume(acc, sib, st->buf, filled >> 6, st->secret);
    const int32_t m = n - t;
    const int32_t cm = ((m - 1) >> 6) << 6;
    xxs::lane_consume(acc, sib, p + t, cm >> 6, st->secret);
    xxs::lane_copy(st->last, cm >= 64 ? p + t + cm - 64 : st->buf + filled - 64, 64);
    xxs::lane_copy(st->buf, p + t + cm, m - cm);
#pragma unroll
    for (int j = 0; j < 8; j++) st->acc[j] = acc[j];
    st->stripes = sib;
    st->bufLen = m - cm;
}

// one piece longer than XXH3_LANE_MAX by the whole wavefront (uniform control flow)
__device__ __forceinline__ void xxh3_update_wave(Xxh3State* st, const uint8_t* __restrict__ p, int32_t n, int lane)
{
    const int q = lane & 3;
    const int32_t b = uni(st->bufLen);
    int32_t sib = uni(st->stripes);
    uint64_t a0 = st->acc[2 * q], a1 = st->acc[2 * q + 1];
    const xxh3::LaneKey k = xxs::lane_key_of(st->secret, lane);
    const int32_t t = (0 - b) & 63;
    if (lane < t) {
        st->buf[b + lane] = p[lane];
    }
    wave_sync();
    xxs::wave_span(st->buf, (b + t) >> 6, sib, k, lane, a0, a1);
    const int32_t m = n - t;  // (> 192: at least two whole stripes of the piece are consumed below, so `last` comes from the piece)
    const int32_t cm = ((m - 1) >> 6) << 6;
    xxs::wave_span(p + t, cm >> 6, sib, k, lane, a0, a1);
    wave_sync();  // (the buffer has been read)
    st->last[lane] = p[t + cm - 64 + lane];
    if (lane < m - cm) {
        st->buf[lane] = p[t + cm + lane];
    }
    if (lane < 4) {
        st->acc[2 * q] = a0;
        st->acc[2 * q + 1] = a1;
    }
    if (lane == 0) {
        st->bufLen = m - cm;
        st->stripes = sib;
        st->total += (uint64_t)n;
    }
}

__global__ __launch_bounds__(256) void xxh3_update_wave_kernel(UpdateArgs a, int32_t group)
{
    const int lane = threadIdx.x & 63;
    const int64_t first = (((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6) * group;
    if (first >= a.n) {
        return;  // (whole wavefronts)
    }
    const int32_t count = a.n - first < group ? (int32_t)(a.n - first) : group;
    const int32_t myLen = lane < count ? a.srcLen[first + lane] : 0;
    uint64_t todo = __ballot(myLen > XXH3_LANE_MAX);
    while (todo != 0) {
        const int j = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t i = first + j;
        const int32_t len = __builtin_amdgcn_readlane(myLen, j);
        xxh3_update_wave((Xxh3State*)(a.states + i * (int64_t)sizeof(Xxh3State)), a.srcBase + a.srcOff[i], len, lane);
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void xxh3_digest_kernel(const uint8_t* __restrict__ states, int32_t n, int64_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    const Xxh3State* st = (const Xxh3State*)(states + i * (int64_t)sizeof(Xxh3State));
    const uint64_t total = st->total;
    uint64_t lo = 0, hi = 0;
    if (total <= (uint64_t)xxh3::SHORT_MAX) {  // (nothing was consumed: the stream is buf[0, total))
        xxh3::short_hash<WIDE>(st->buf, (int32_t)total, st->seed, kStreamSecret, lo, hi);
    }
    else {
        uint64_t acc[8];
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] = st->acc[j];
        int32_t sib = st->stripes;
        const int32_t b = st->bufLen;
        const uint8_t* sec = st->secret;
        // the buffer's whole stripes short of its last byte, then the stream's last 64 bytes (from `last` and the buffer when the buffer is short)
        xxs::lane_consume(acc, sib, st->buf, b >= 64 ? (b - 1) >> 6 : 0, sec);
        uint64_t x[8];
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = b >= 64 ? ld8(st->buf + b - 64 + 8 * j) : xxs::ld8_seam(st->last + b, 64 - b, st->buf, 8 * j);
        xxs::lane_stripe_words(acc, x, sec + 121);
        uint64_t m = total * xxh3::P64_1;
#pragma unroll
        for (int j = 0; j < 4; j++) m += xxh3::fold64(acc[2 * j] ^ xxh3::rd64(sec + 11 + 16 * j), acc[2 * j + 1] ^ xxh3::rd64(sec + 11 + 16 * j + 8));
        lo = xxh3::avalanche(m);
        if (WIDE) {
            uint64_t h = ~(total * xxh3::P64_2);
#pragma unroll
            for (int j = 0; j < 4; j++) h += xxh3::fold64(acc[2 * j] ^ xxh3::rd64(sec + 117 + 16 * j), acc[2 * j + 1] ^ xxh3::rd64(sec + 117 + 16 * j + 8));
            hi = xxh3::avalanche(h);
        }
    }
    if (WIDE) {
        out[2 * i] = (int64_t)lo;
        out[2 * i + 1] = (int64_t)hi;
    }
    else {
        out[i] = (int64_t)lo;
    }
}

// states a wavefront of the XXH3 wave kernel looks after: as xxh3_group of the one-shot kernels (about 8 192 wavefronts or more, at most 64 states each)
int32_t stream_group(int32_t n)
{
    const int32_t g = n / 8192;
    return g < 1 ? 1 : (g > 64 ? 64 : g);
}

dim3 lanes_grid(int32_t n) { return dim3((unsigned)(((int64_t)n + 255) / 256)); }
dim3 quads_grid(int32_t n) { return dim3((unsigned)(((int64_t)n + 15) / 16)); }

}  // namespace

hipError_t launch_hash_states_reset(int32_t algo, void* states, int32_t n, uint64_t seed, hipStream_t stream)
{
    if (n <= 0) {
        return hipSuccess;
    }
    switch (algo) {
    case HASH_XXH32: hipLaunchKernelGGL(quad_reset_kernel<T32>, lanes_grid(n), dim3(256), 0, stream, (uint8_t*)states, n, (uint32_t)seed); break;
    case HASH_XXH64: hipLaunchKernelGGL(quad_reset_kernel<T64>, lanes_grid(n), dim3(256), 0, stream, (uint8_t*)states, n, seed); break;
    default: hipLaunchKernelGGL(xxh3_reset_kernel, lanes_grid(n), dim3(256), 0, stream, (uint8_t*)states, n, seed); break;
    }
    return hipGetLastError();
}

hipError_t launch_hash_states_update(int32_t algo, void* states, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, hipStream_t stream)
{
    if (n <= 0) {
        return hipSuccess;
    }
    UpdateArgs a{(uint8_t*)states, (const uint8_t*)srcBase, srcOff, srcLen, n};
    if (algo == HASH_XXH32) {
        hipLaunchKernelGGL(quad_update_kernel<T32>, quads_grid(n), dim3(64), 0, stream, a);
        return hipGetLastError();
    }
    if (algo == HASH_XXH64) {
        hipLaunchKernelGGL(quad_update_kernel<T64>, quads_grid(n), dim3(64), 0, stream, a);
        return hipGetLastError();
    }
    const int32_t group = stream_group(n);
    const int64_t waves = ((int64_t)n + group - 1) / group;
    hipLaunchKernelGGL(xxh3_update_wave_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, a, group);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(xxh3_update_lane_kernel, lanes_grid(n), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_hash_states_digest(int32_t algo, const void* states, int64_t* out, int32_t n, hipStream_t stream)
{
    if (n <= 0) {
        return hipSuccess;
    }
    const uint8_t* s = (const uint8_t*)states;
    switch (algo) {
    case HASH_XXH32: hipLaunchKernelGGL(quad_digest_kernel<T32>, lanes_grid(n), dim3(256), 0, stream, s, n, out); break;
    case HASH_XXH64: hipLaunchKernelGGL(quad_digest_kernel<T64>, lanes_grid(n), dim3(256), 0, stream, s, n, out); break;
    case HASH_XXH3_64: hipLaunchKernelGGL(xxh3_digest_kernel<false>, lanes_grid(n), dim3(256), 0, stream, s, n, out); break;
    default: hipLaunchKernelGGL(xxh3_digest_kernel<true>, lanes_grid(n), dim3(256), 0, stream, s, n, out); break;
    }
    return hipGetLastError();
}

}  // namespace achip
