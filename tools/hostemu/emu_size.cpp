// tools/hostemu/emu_size.cpp -- the sizing kernels and the output planner (decoded_size.hip) under the fiber emulator: the lane-per-block and wavefront-per-block
// LZ4 walks (the window chain's lane reads, scans and ballots are rendezvous of the wave here), the Snappy preamble, the Zstd walk (its table builds meet at
// workgroup barriers), the containers' list / size / fold, the planner's workgroup scans.  Driven by check_size.py.
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/decoded_size.hip"
#include <vector>
extern "C" int emu_decoded_size(int32_t op, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t* outSize, int32_t* status, int64_t* errOffset, int32_t n)
{
    std::vector<uint8_t> scratch((size_t)achip::decoded_size_scratch_bytes(op, n) + 16, 0xCD);
    const achip::SizeArgs s{srcBase, srcOff, srcLen, outSize, status, errOffset, n};
    return (int)achip::launch_decoded_size(op, s, nullptr, scratch.data());
}
// LZ4 frames with achip_ctx_set_lz4frame_linked_blocks(accept) (check_lz4_linked.py)
extern "C" int emu_lz4frame_size_linked(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t* outSize, int32_t* status, int64_t* errOffset, int32_t n, int32_t accept)
{
    std::vector<uint8_t> scratch((size_t)achip::decoded_size_scratch_bytes(ACHIP_OP_LZ4FRAME_DECOMPRESS, n) + 16, 0xCD);
    achip::SizeArgs s{srcBase, srcOff, srcLen, outSize, status, errOffset, n};
    s.lz4fLinked = accept;
    return (int)achip::launch_decoded_size(ACHIP_OP_LZ4FRAME_DECOMPRESS, s, nullptr, scratch.data());
}
// the LZ4 walk in the shape the launcher would not pick for this count: shape 1 a lane per block, 2 a wavefront per block
extern "C" int emu_lz4_size_shape(int32_t shape, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t* outSize, int32_t* status, int64_t* errOffset, int32_t n)
{
    const achip::SizeArgs s{srcBase, srcOff, srcLen, outSize, status, errOffset, n};
    if (shape == 1) {
        hipLaunchKernelGGL(achip::lz4_size_lane_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, s);
    }
    else {
        hipLaunchKernelGGL(achip::lz4_size_wave_kernel, dim3((unsigned)n), dim3(64), 0, nullptr, s);
    }
    return 0;
}
extern "C" int emu_plan_outputs(const int64_t* outSize, const int32_t* status, int32_t n, int32_t align, int64_t* dstOff, int32_t* dstCap, int64_t* total)
{
    std::vector<uint8_t> scratch((size_t)achip::plan_outputs_scratch_bytes(n) + 16, 0xCD);
    return (int)achip::launch_plan_outputs(outSize, status, n, align, dstOff, dstCap, total, scratch.data(), nullptr);
}
