// tools/hostemu/emu_lz4f_writer.cpp -- the block-list LZ4 frame writer of lz4_frame_writer.hip (plan, seal, encode, compact) with the settings of
// achip_ctx_set_lz4frame_writer on the CPU, every memory access an order point and wave_mem_order() a rendezvous like emu_enc.cpp: the block encoder changes its hash
// table in place and is exact only under the device's lockstep.  Driven by check_lz4f_writer.py.
#define HOSTEMU_ACCESS_LOCKSTEP 1
#define HOSTEMU_ORDER_IS_RENDEZVOUS 1
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/lz4_frame_writer.hip"
#include <vector>

// listEntries: the entries the block list is sealed at (0: the product's 2^20) -- a frame of more blocks is refused
extern "C" int emu_lz4f_write(int32_t listEntries, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize, int32_t acceleration,
                              const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen,
                              int32_t* status, int64_t* errOffset, int32_t n)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 0};
    achip::KernelSettings ks;
    if (achip::set_lz4f_writer(ks, blockMaxSize, blockChecksum, contentChecksum, contentSize) != achip::Lz4fRefusal::None) {
        fprintf(stderr, "hostemu: LZ4 frame writer settings refused\n");
        abort();
    }
    ks.lz4fCompressVariant = 1;   // (the block list at the default settings too)
    ks.lz4fEncodeWorkgroups = 2;  // (the persistent grid: the emulator runs its wavefronts one after the other)
    ks.lz4fListEntries = listEntries;
    ks.lz4Acceleration = acceleration;
    std::vector<uint8_t> scratch((size_t)achip::lz4frame_list_compress_scratch_bytes(n), 0xCD);
    return (int)achip::launch_lz4frame_list_compress(a, nullptr, scratch.data(), ks);
}
