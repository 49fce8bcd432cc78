// achip_plan.h -- the exclusive scan of per-item room that both planners run: achip_plan_outputs over decoded sizes (decoded_size.hip) and achip_pack_outputs
// over the lengths a compress call left (pack_outputs.hip).  Reduce per tile, scan of the tile sums by one workgroup, scan per tile: three launches, no
// workgroup waits for another.  What an item takes is a functor's business:
//   int64_t room(int64_t i, int64_t n, int64_t mask, int32_t& len, int32_t& leftOut) const   item i's length, and its room = the length rounded up (0, 0 for i >= n;
//                                                                                             a left-out item takes none and sets leftOut)
//   void emit(int64_t i, int64_t at, int32_t len) const                                       item i starts at `at`
//   void finish(int64_t* total) const                                                         one thread, behind total[0] = the bytes, total[1] = the items left out
#pragma once
#include "achip_device.h"

namespace achip {
namespace ds {
constexpr int PLAN_THREADS = 256, PLAN_PER_THREAD = 4, PLAN_TILE = PLAN_THREADS * PLAN_PER_THREAD;

__device__ __forceinline__ int64_t wave_scan_incl64(int64_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t t = __shfl_up(v, d);
        if (lane >= d) {
            v += t;
        }
    }
    return v;
}
// inclusive scan over the workgroup's threads; total = the sum of all (waveSums: PLAN_THREADS / 64 words of LDS)
__device__ __forceinline__ int64_t block_scan_incl64(int64_t v, int64_t* waveSums, int64_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t incl = wave_scan_incl64(v, lane);
    __syncthreads();
    if (lane == 63) {
        waveSums[wave] = incl;
    }
    __syncthreads();
    int64_t before = 0;
    total = 0;
    for (int k = 0; k < PLAN_THREADS / 64; k++) {
        const int64_t w = waveSums[k];
        before += k < wave ? w : 0;
        total += w;
    }
    return incl + before;
}
}  // namespace ds

template <class F>
__global__ __launch_bounds__(256) void plan_reduce_kernel(F f, int32_t n, int64_t mask, int64_t* tileRoom, int64_t* tileLeftOut)
{
    using namespace ds;
    __shared__ int64_t waveSums[PLAN_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * PLAN_TILE + (int64_t)threadIdx.x * PLAN_PER_THREAD;
    int64_t room = 0, left = 0;
    for (int k = 0; k < PLAN_PER_THREAD; k++) {
        int32_t len, leftOut;
        room += f.room(base + k, n, mask, len, leftOut);
        left += leftOut;
    }
    int64_t roomTotal = 0, leftTotal = 0;
    block_scan_incl64(room, waveSums, roomTotal);
    block_scan_incl64(left, waveSums, leftTotal);
    if (threadIdx.x == 0) {
        tileRoom[blockIdx.x] = roomTotal;
        tileLeftOut[blockIdx.x] = leftTotal;
    }
}

// one workgroup: tileRoom[] becomes its exclusive scan; total[0] = the bytes the output needs, total[1] = the items left out
template <class F>
__global__ __launch_bounds__(256) void plan_tiles_kernel(F f, int64_t* tileRoom, const int64_t* __restrict__ tileLeftOut, int32_t tiles, int64_t* total)
{
    using namespace ds;
    __shared__ int64_t waveSums[PLAN_THREADS / 64];
    int64_t base = 0, left = 0;
    for (int32_t t0 = 0; t0 < tiles; t0 += PLAN_THREADS) {  // (uniform)
        const int32_t t = t0 + (int32_t)threadIdx.x;
        const int64_t room = t < tiles ? tileRoom[t] : 0;
        left += t < tiles ? tileLeftOut[t] : 0;
        int64_t sum = 0;
        const int64_t incl = block_scan_incl64(room, waveSums, sum);
        if (t < tiles) {
            tileRoom[t] = base + incl - room;
        }
        base += sum;
    }
    int64_t leftTotal = 0;
    block_scan_incl64(left, waveSums, leftTotal);
    if (threadIdx.x == 0) {
        total[0] = base;
        total[1] = leftTotal;
        f.finish(total);
    }
}

template <class F>
__global__ __launch_bounds__(256) void plan_scan_kernel(F f, int32_t n, int64_t mask, const int64_t* __restrict__ tileBase)
{
    using namespace ds;
    __shared__ int64_t waveSums[PLAN_THREADS / 64];
    const int64_t first = (int64_t)blockIdx.x * PLAN_TILE + (int64_t)threadIdx.x * PLAN_PER_THREAD;
    int64_t room[PLAN_PER_THREAD];
    int32_t len[PLAN_PER_THREAD];
    int64_t mine = 0;
    for (int k = 0; k < PLAN_PER_THREAD; k++) {
        int32_t leftOut;
        room[k] = f.room(first + k, n, mask, len[k], leftOut);
        mine += room[k];
    }
    int64_t sum = 0;
    int64_t at = tileBase[blockIdx.x] + block_scan_incl64(mine, waveSums, sum) - mine;
    for (int k = 0; k < PLAN_PER_THREAD; k++) {
        if (first + k < n) {
            f.emit(first + k, at, len[k]);
        }
        at += room[k];
    }
}

inline int32_t plan_tile_count(int32_t n) { return (int32_t)(((int64_t)n + ds::PLAN_TILE - 1) / ds::PLAN_TILE); }
inline int64_t plan_scan_scratch_bytes(int32_t n) { return 2 * (int64_t)plan_tile_count(n) * (int64_t)sizeof(int64_t); }

// the three launches; scratch: plan_scan_scratch_bytes(n) bytes
template <class F>
hipError_t launch_plan_scan(const F& f, int32_t n, int32_t align, int64_t* total, void* scratch, hipStream_t stream)
{
    const int32_t tiles = plan_tile_count(n);
    int64_t* tileRoom = (int64_t*)scratch;
    int64_t* tileLeftOut = tileRoom + tiles;
    const int64_t mask = (int64_t)align - 1;
    hipLaunchKernelGGL((plan_reduce_kernel<F>), dim3((unsigned)tiles), dim3(ds::PLAN_THREADS), 0, stream, f, n, mask, tileRoom, tileLeftOut);
    hipLaunchKernelGGL((plan_tiles_kernel<F>), dim3(1), dim3(ds::PLAN_THREADS), 0, stream, f, tileRoom, (const int64_t*)tileLeftOut, tiles, total);
    hipLaunchKernelGGL((plan_scan_kernel<F>), dim3((unsigned)tiles), dim3(ds::PLAN_THREADS), 0, stream, f, n, mask, (const int64_t*)tileRoom);
    return hipGetLastError();
}

}  // namespace achip
