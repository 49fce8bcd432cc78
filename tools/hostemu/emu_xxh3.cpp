// tools/hostemu/emu_xxh3.cpp -- the XXH3 kernels (xxhash3.hip) under the fiber emulator: the lane-per-buffer short kernel and the
// wavefront-per-buffer long kernel, whose cross-lane sums (__shfl_xor) and ballot are rendezvous of the wave here.  Driven by check_xxh3.py.
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/xxhash3.hip"
extern "C" int emu_xxh3_batch(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, uint64_t seed, int32_t wide, int64_t* out)
{
    return (int)achip::launch_xxh3_batch(srcBase, srcOff, srcLen, n, seed, wide != 0, out, nullptr);
}
