// tools/hostemu/emu_serial.cpp -- the wavefront-per-item kernels under the fiber emulator: the LZ4 frame reader (lz4_frame.hip variant 0), the
// x-snappy-framed and Hadoop stream readers' wavefront-per-stream kernels (variant 0), the one-kernel Zstd decoder.  They run one item per
// wavefront in wave-uniform control flow over Rings<64, ...>: wave_mem_order() is a rendezvous of the wave here (HOSTEMU_ORDER_IS_RENDEZVOUS),
// the rings' lockstep points are rendezvous of the 64-lane group.  A library of its own: the other emulated kernels need wave_mem_order()
// to stay what it is on the device.
#define HOSTEMU_RINGS_LOCKSTEP 1
#define HOSTEMU_ORDER_IS_RENDEZVOUS 1
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/lz4_frame.hip"
#include "../../aircompressor_amd/csrc/snappy_frame.hip"
#include "../../aircompressor_amd/csrc/hadoop_streams.hip"
#include "../../aircompressor_amd/csrc/zstd_decompress.hip"
#include <vector>
// the list paths' decode and the Zstd pipeline (not part of this library: the wavefront-per-item kernels only).  Qualified definitions: each must
// match its declaration in achip_launch.h
hipError_t achip::launch_listed_decode(const BatchArgs&, int, hipStream_t, const int32_t*, int32_t*, const AuxScratch*, const KernelSettings&, const ListedWant&, bool*) { return hipSuccess; }
int64_t achip::zstd_decompress_pipe_scratch_bytes(int32_t, int32_t) { return 0; }
hipError_t achip::launch_zstd_decompress_pipe(const BatchArgs&, hipStream_t, void*, void*, int32_t, const ZstdMbProvider*, const KernelSettings&) { return hipSuccess; }
void* achip::zstd_decompress_pipe_general_scratch(void* scratch, int32_t, int32_t) { return scratch; }

extern "C" int emu_lz4frame_serial(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap,
                                   int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 16};
    static std::vector<uint8_t> scratch;
    scratch.assign(4096, 0);
    return achip::launch_lz4frame_decompress(a, nullptr, scratch.data(), 0, nullptr, achip::KernelSettings());
}

// the same with achip_ctx_set_lz4frame_linked_blocks(accept) (check_lz4_linked.py)
extern "C" int emu_lz4frame_serial_linked(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap,
                                          int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n, int32_t accept)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 16};
    static std::vector<uint8_t> scratch;
    scratch.assign(4096, 0);
    achip::KernelSettings ks;
    if (!achip::set_lz4f_linked_blocks(ks, accept)) return -1;
    return achip::launch_lz4frame_decompress(a, nullptr, scratch.data(), 0, nullptr, ks);
}

// op 8: x-snappy-framed streams, 10 / 12: Hadoop LZ4 / Snappy block streams, 4: Zstd frames -- each through its wavefront-per-item kernel
extern "C" int emu_serial(int op, int bufferSize, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff,
                          const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 16};
    static std::vector<uint8_t> scratch;
    if (op == 6) {
        scratch.assign(4096, 0);
        return achip::launch_lz4frame_decompress(a, nullptr, scratch.data(), 0, nullptr, achip::KernelSettings());
    }
    if (op == 8) {
        scratch.assign((size_t)achip::snappyframed_decompress_scratch_bytes(n), 0xCD);
        return achip::launch_snappyframed_decompress(a, nullptr, scratch.data(), 0, nullptr, achip::KernelSettings());
    }
    if (op == 10 || op == 12) {
        scratch.assign((size_t)achip::hadoop_decompress_scratch_bytes(n, bufferSize), 0xCD);
        return achip::launch_hadoop_decompress(a, nullptr, scratch.data(), op == 12, bufferSize, 0, nullptr, achip::KernelSettings());
    }
    if (op == 4) {
        scratch.assign((size_t)achip::zstd_decompress_general_scratch_bytes() + 4096, 0xCD);
        return achip::launch_zstd_decompress(a, nullptr, scratch.data(), (int64_t)scratch.size(), 0, 0, nullptr, achip::KernelSettings());
    }
    return -1;
}
