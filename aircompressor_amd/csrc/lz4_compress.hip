// lz4_compress.hip -- batched LZ4 block encode for gfx950, bit-exact with the Java encoder.
//
// Replaces Lz4RawCompressor.compress + hash/count/emitLiteral/emitMatch/emitLastLiteral/
// encodeRunLength/computeTableSize (M/lz4/Lz4RawCompressor.java:50-312).
//
// One wavefront per block.  The greedy parse is inherently serial per block (which
// positions enter the hash table depends on the parse so far, :113-183), so the parse
// state is wave-uniform and the 64 lanes help inside each step:
//   * hash table (4096 entries, positions relative to the block) lives in LDS -- u16
//     entries for blocks <= 64 KiB (8 KiB per wave => 20 waves / CU), i32 otherwise;
//   * `count` compares 64 x 8 bytes per step and resolves the first mismatch with a
//     ballot (:240-267);
//   * literal runs are copied 64 x 16 bytes per step.
// PROBE_BATCH > 1 additionally evaluates the next PROBE_BATCH probe positions of the
// skip-accelerated search loop (:113-138) in parallel, resolving same-hash collisions
// inside the batch so the table evolves exactly as in program order.
#include "lz4_compress_body.h"
#include "lz4_compress_mw.h"
#include "achip_launch.h"

namespace achip {

namespace lz4t {
constexpr int LDS_WAVES = 5;
constexpr int MEM_WAVES_MAX = 2;
constexpr int WORKGROUPS = 256 * 4;
}  // namespace lz4t

namespace lz4f {
constexpr int32_t BLOCK_MAX_4MB = 4 * 1024 * 1024;
constexpr int64_t SLAB_BYTES = ((int64_t)BLOCK_MAX_4MB + BLOCK_MAX_4MB / 255 + 16 + 255) & ~(int64_t)255;
constexpr int32_t MAX_WAVES = 2304;  // 9 wavefronts per CU (16 KB of LDS each) x 256 CUs; round 3 ran 512 (2 per CU): 5 GiB/s where the 64 KiB block encoder makes 28
constexpr int32_t MIN_WAVES = 256;
}  // namespace lz4f

#define LZ4K(name) name
#define LZ4K_PARAM
#define LZ4K_ACCEL false
#define LZ4K_VALUE 1
#include "lz4_compress_kernels.h"
#undef LZ4K
#undef LZ4K_PARAM
#undef LZ4K_ACCEL
#undef LZ4K_VALUE
// the `_accel` twins, launched for an acceleration above 1
#define LZ4K(name) name##_accel
#define LZ4K_PARAM , int32_t accel
#define LZ4K_ACCEL true
#define LZ4K_VALUE accel
#include "lz4_compress_kernels.h"
#undef LZ4K
#undef LZ4K_PARAM
#undef LZ4K_ACCEL
#undef LZ4K_VALUE

// one 4 MiB slab per resident wavefront: `items` items never need more wavefronts than that (9.7 GB for a batch that fills the chip, on a
// 288 GB device; `least`: what the launch can still work with when the device cannot give that)
int64_t lz4frame_compress_scratch_bytes(int32_t items, bool least)
{
    int64_t waves = items < lz4f::MAX_WAVES ? (items > 0 ? items : 1) : lz4f::MAX_WAVES;
    if (least && waves > lz4f::MIN_WAVES) waves = lz4f::MIN_WAVES;
    return 4096 + waves * lz4f::SLAB_BYTES;
}

// A kernel of either set (lz4_compress_kernels.h): the `_accel` twin with the acceleration behind the other arguments for an acceleration above 1, else the kernel
// as it was.  LZ4K_BOTH(name, <T>) names the two.
#define LZ4K_BOTH(name, ...) name __VA_ARGS__, name##_accel __VA_ARGS__
template <typename Plain, typename Accel, typename... Args>
static void launch_lz4k(Plain plain, Accel twin, int32_t acceleration, dim3 grid, dim3 block, hipStream_t stream, Args... args)
{
    if (acceleration > 1) {
        hipLaunchKernelGGL(twin, grid, block, 0, stream, args..., acceleration);
    }
    else {
        hipLaunchKernelGGL(plain, grid, block, 0, stream, args...);
    }
}

hipError_t launch_lz4frame_compress(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int32_t acceleration)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    int32_t* counter = (int32_t*)scratch;
    hipError_t e = hipMemsetAsync(counter, 0, 64, stream);
    if (e != hipSuccess) return e;
    int64_t waves = (scratchBytes - 4096) / lz4f::SLAB_BYTES;  // a slab per wavefront
    if (waves < 1) return hipErrorUnknown;  // (the caller sizes the scratch: never)
    if (waves > lz4f::MAX_WAVES) waves = lz4f::MAX_WAVES;
    const unsigned grid = (unsigned)(a.nBlocks < waves ? a.nBlocks : waves);
    launch_lz4k(LZ4K_BOTH(lz4frame_compress_kernel), acceleration, dim3(grid), dim3(64), stream, a, (uint8_t*)scratch + 4096, counter);
    return hipGetLastError();
}

// the two-tier kernel: from batches that fill the LDS tier on (fewer blocks: a wavefront per block, all tables in LDS); ks.lz4MemWaves, ks.lz4TierMinBlocks
int64_t lz4_compress_scratch_bytes() { return 4096 + (int64_t)lz4t::WORKGROUPS * lz4t::MEM_WAVES_MAX * lz4c::MAX_TABLE_SIZE * 2; }

hipError_t launch_lz4_compress(const BatchArgs& a, hipStream_t stream, int variant, int maxSrcLenHint, void* scratch, int64_t scratchBytes, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    // maxSrcLenHint: 0 = unknown, else the caller's promise about the largest srcLen in the batch: when it is <= 64 KiB the launch of
    // the wide-table kernel is skipped (a block that breaks the promise gets an INVALID_ARGUMENT status, not silence)
    const int32_t both = maxSrcLenHint == 0 || maxSrcLenHint > 65536;
    const int32_t accel = ks.lz4Acceleration;
    const dim3 grid((unsigned)a.nBlocks), wave(64);
    // blocks up to 64 KiB: the narrow table
    if (variant == 4 && ks.lz4MemWaves > 0 && a.nBlocks >= ks.lz4TierMinBlocks && scratch != nullptr && scratchBytes >= lz4_compress_scratch_bytes()) {
        int32_t* counter = (int32_t*)scratch;
        const hipError_t e = hipMemsetAsync(counter, 0, 64, stream);
        if (e != hipSuccess) return e;
        const unsigned perGroup = (unsigned)(lz4t::LDS_WAVES + ks.lz4MemWaves);
        unsigned groups = ks.lz4TierWorkgroups > 0 ? (unsigned)ks.lz4TierWorkgroups : (unsigned)lz4t::WORKGROUPS;
        groups = groups > (unsigned)lz4t::WORKGROUPS ? (unsigned)lz4t::WORKGROUPS : groups;
        const unsigned need = ((unsigned)a.nBlocks + perGroup - 1) / perGroup;
        launch_lz4k(LZ4K_BOTH(lz4_compress_tiers_kernel), accel, dim3(need < groups ? need : groups), dim3(64 * perGroup), stream, a, both, (uint16_t*)((uint8_t*)scratch + 4096), counter);
    }
    else if (variant == 4) {
        launch_lz4k(LZ4K_BOTH(lz4_compress_mw_kernel, <uint16_t>), accel, grid, wave, stream, a, both);
    }
    else if (variant == 0) {
        launch_lz4k(LZ4K_BOTH(lz4_compress_kernel, <uint16_t>), accel, grid, wave, stream, a, both);
    }
    else {
        launch_lz4k(LZ4K_BOTH(lz4_compress_batch_kernel, <uint16_t>), accel, grid, wave, stream, a, both);
    }
    if (both) {  // blocks beyond 64 KiB: the wide table
        if (variant == 4) {
            launch_lz4k(LZ4K_BOTH(lz4_compress_mw_kernel, <int32_t>), accel, grid, wave, stream, a, both);
        }
        else if (variant == 0) {
            launch_lz4k(LZ4K_BOTH(lz4_compress_kernel, <int32_t>), accel, grid, wave, stream, a, both);
        }
        else {
            launch_lz4k(LZ4K_BOTH(lz4_compress_batch_kernel, <int32_t>), accel, grid, wave, stream, a, both);
        }
    }
    return hipGetLastError();
}

}  // namespace achip
