// tools/hostemu/emu_pack.cpp -- the bound kernel, the pack scan and the dense copy (pack_outputs.hip) under the fiber emulator: the scan's workgroup barriers,
// the copy's 64-way search (a ballot: a rendezvous of the wave here) and its per-lane chunk work.  Driven by check_pack.py.
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/pack_outputs.hip"
#include <vector>
extern "C" long long emu_pack_tile_bytes() { return achip::PACK_TILE_BYTES; }
extern "C" int emu_compress_bound(int32_t op, const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t n, int32_t hadoopBufferSize)
{
    return (int)achip::launch_compress_bound(op, srcLen, outSize, status, n, hadoopBufferSize, nullptr, achip::KernelSettings().snfBlockSize);
}
extern "C" int emu_pack_outputs(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* outLen, const int32_t* status, const uint8_t* rawBase, const int64_t* rawOff,
                                const int32_t* rawLen, int32_t n, int32_t align, uint8_t* packedBase, int64_t packedCap, int64_t* packedOff, int32_t* packedLen, int32_t* stored,
                                int64_t* total)
{
    std::vector<uint8_t> scratch((size_t)achip::pack_outputs_scratch_bytes(n) + 16, 0xCD);
    const achip::PackArgs p{srcBase, srcOff, outLen, status, rawBase, rawOff, rawLen, n, align, packedBase, packedCap, packedOff, packedLen, stored, total};
    return (int)achip::launch_pack_outputs(p, scratch.data(), nullptr);
}
