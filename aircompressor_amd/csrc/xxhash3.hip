// xxhash3.hip -- batched XXH3-64 / XXH3-128 for gfx950 (the reference's XxHash3Native.hash / hash128 with a seed, for many buffers per call).
//
// A batch mixes sizes and the host does not see the device-resident lengths, so one call is two kernels on the stream, each skipping the
// other's buffers (achip_xxh3.h has the two roles):
//   * xxh3_long_kernel: a wavefront per buffer longer than 240 bytes.  Wavefront w looks after buffers [w*group, w*group + group): its lanes
//     read those lengths, a ballot picks the long ones, and the wavefront hashes them one after the other.  `group` grows with the batch
//     (the host picks it from nBuffers alone) so that a batch of millions of short buffers does not launch a wavefront per buffer, while a
//     batch of a few thousand long ones still gives every buffer its own wavefront.
//   * xxh3_short_kernel: a lane per buffer of at most 240 bytes.
// Roofline: HBM (read-once); algorithmic bytes = the buffer lengths.
#include "achip_xxh3.h"
#include "achip_launch.h"

namespace achip {

namespace {

__constant__ uint8_t kXxh3Secret[192] = ACHIP_XXH3_SECRET_BYTES;

struct Xxh3Args {
    const uint8_t* __restrict__ srcBase;
    const int64_t* __restrict__ srcOff;
    const int32_t* __restrict__ srcLen;
    int64_t* __restrict__ out;  // one word per buffer (64-bit), two (low, high) for the 128-bit hash
    int32_t n;
};

template <bool WIDE>
__device__ __forceinline__ void put(int64_t* __restrict__ out, int64_t i, uint64_t lo, uint64_t hi)
{
    if (WIDE) {
        out[2 * i] = (int64_t)lo;
        out[2 * i + 1] = (int64_t)hi;
    }
    else {
        out[i] = (int64_t)lo;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void xxh3_short_kernel(Xxh3Args a, uint64_t seed)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) {
        return;
    }
    int32_t len = a.srcLen[i];
    len = len < 0 ? 0 : len;  // (a negative length hashes as empty)
    if (len > xxh3::SHORT_MAX) {
        return;
    }
    uint64_t lo = 0, hi = 0;
    xxh3::short_hash<WIDE>(a.srcBase + a.srcOff[i], len, seed, kXxh3Secret, lo, hi);
    put<WIDE>(a.out, i, lo, hi);
}

template <bool WIDE>
__global__ __launch_bounds__(256) void xxh3_long_kernel(Xxh3Args a, xxh3::Key key, int32_t group)
{
    const int lane = threadIdx.x & 63;
    const int64_t first = (((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6) * group;
    if (first >= a.n) {
        return;  // (whole wavefronts)
    }
    const int32_t count = a.n - first < group ? (int32_t)(a.n - first) : group;
    const int32_t myLen = lane < count ? a.srcLen[first + lane] : 0;
    uint64_t todo = __ballot(myLen > xxh3::SHORT_MAX);
    if (todo == 0) {
        return;
    }
    const xxh3::LaneKey k = xxh3::lane_key(key, lane);
    while (todo != 0) {
        const int j = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t i = first + j;
        const int32_t len = __builtin_amdgcn_readlane(myLen, j);
        uint64_t lo = 0, hi = 0;
        xxh3::long_hash_wave<WIDE>(a.srcBase + a.srcOff[i], len, k, lane, lo, hi);
        if (lane == 0) {
            put<WIDE>(a.out, i, lo, hi);
        }
    }
}

// buffers a long-path wavefront looks after: about 8 192 wavefronts or more (32 a CU), at most 64 buffers each
int32_t xxh3_group(int32_t n)
{
    const int32_t g = n / 8192;
    return g < 1 ? 1 : (g > 64 ? 64 : g);
}

}  // namespace

hipError_t launch_xxh3_batch(const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, uint64_t seed, bool wide, int64_t* out, hipStream_t stream)
{
    if (n <= 0) {
        return hipSuccess;
    }
    Xxh3Args a{(const uint8_t*)srcBase, srcOff, srcLen, out, n};
    xxh3::Key key;
    xxh3::derive_key(seed, &key);
    const int32_t group = xxh3_group(n);
    const int64_t waves = ((int64_t)n + group - 1) / group;
    const dim3 longGrid((unsigned)((waves + 3) / 4)), shortGrid((unsigned)(((int64_t)n + 255) / 256));
    if (wide) {
        hipLaunchKernelGGL(xxh3_long_kernel<true>, longGrid, dim3(256), 0, stream, a, key, group);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(xxh3_short_kernel<true>, shortGrid, dim3(256), 0, stream, a, seed);
    }
    else {
        hipLaunchKernelGGL(xxh3_long_kernel<false>, longGrid, dim3(256), 0, stream, a, key, group);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(xxh3_short_kernel<false>, shortGrid, dim3(256), 0, stream, a, seed);
    }
    return hipGetLastError();
}

}  // namespace achip
