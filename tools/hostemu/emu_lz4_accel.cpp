// tools/hostemu/emu_lz4_accel.cpp -- the `_accel` kernels of lz4_compress.hip (the LZ4 encoders with the search schedule of Lz4Compressor.create(acceleration)) on
// the CPU, every memory access a soft order point like emu_enc.cpp (the same build flags: tools/hostemu/build.sh lz4_accel).  Driven by check_lz4_accel.py.
#define HOSTEMU_ACCESS_LOCKSTEP 1
#define HOSTEMU_ORDER_IS_RENDEZVOUS 1
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/lz4_compress.hip"
#include <vector>
// frame: 0 = block encoder (variant 0 / 1 / 4; memWaves 0 = a wavefront per block, 1 / 2 = the two-tier kernel with a grid of two workgroups), 1 = the frame writer
extern "C" int emu_lz4_accel(int frame, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap,
                             int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n, int32_t variant, int32_t memWaves, int32_t maxSrcLenHint, int32_t acceleration)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 0};
    std::vector<uint8_t> scratch;
    if (frame) {
        scratch.assign((size_t)achip::lz4frame_compress_scratch_bytes(n < 4 ? n : 4, false), 0xCD);  // (a slab per wavefront: the emulator runs them one after the other)
        return (int)achip::launch_lz4frame_compress(a, nullptr, scratch.data(), (int64_t)scratch.size(), acceleration);
    }
    scratch.assign((size_t)achip::lz4_compress_scratch_bytes(), 0xCD);
    achip::KernelSettings ks;
    ks.lz4TierWorkgroups = 2;
    ks.lz4TierMinBlocks = 1;
    ks.lz4MemWaves = memWaves;
    ks.lz4Acceleration = acceleration;
    return (int)achip::launch_lz4_compress(a, nullptr, variant, maxSrcLenHint, scratch.data(), (int64_t)scratch.size(), ks);
}
