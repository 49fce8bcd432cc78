// tools/hostemu/emu_lzo.cpp -- the LZO kernels on the CPU, two libraries from one unit (emulib.py: group lzo).  Driven by check_lzo.py.
//   LZO_ENCODER   lzo_compress.hip, built like the other encoder units (emu_enc.cpp): the 64 lanes run the same serial code and change the hash table in
//                 place, which is exact only under the device's lockstep -- every memory access of the kernel source is a soft order point.
//   otherwise     lzo_decompress.hip with the record executor it parses for (emu.cpp holds lz4_decompress_v7.hip) and the sizing kernel of decoded_size.hip,
//                 under the soft order point: lzo_parse2_kernel's lanes go their own ways, lzo_decompress_wave_kernel and the executor run a wavefront in
//                 uniform control flow.
#ifdef LZO_ENCODER
#define HOSTEMU_ACCESS_LOCKSTEP 1
#define HOSTEMU_ORDER_IS_RENDEZVOUS 1
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/lzo_compress.hip"
extern "C" int emu_lzo_encode(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap,
                              int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 0};
    return (int)achip::launch_lzo_compress(a, nullptr);
}
#else
#define HOSTEMU_ORDER_IS_SOFT 1
#include "emu.cpp"
#include "../../aircompressor_amd/csrc/lzo_decompress.hip"
#include "../../aircompressor_amd/csrc/decoded_size.hip"
// variant 1: the two passes (maxChunks > 0: an arena of that many chunks, so that items are handed over), 2: a wavefront per item.  *fallbackBlocks: the items
// the parser handed to the wavefront decoder.
extern "C" int emu_lzo_decode(int variant, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap,
                              int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n, int32_t maxChunks, int32_t* fallbackBlocks)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 0};
    *fallbackBlocks = 0;
    if (variant == 2) {
        return (int)achip::launch_lzo_decompress_wave(a, nullptr);
    }
    static GuardedScratch scratch;
    const int64_t bytes = achip::twopass_scratch_bytes(n, achip::LZ4_RECORD_BYTES_PER_BLOCK) - (60LL << 20);  // (4 of the product's 64 MiB of slack: enough for the long-run item)
    scratch.assign(bytes);
    const int r = scratch.check("the LZO two passes", (int)achip::launch_lzo_decompress_twopass(a, nullptr, scratch.v.data(), bytes, maxChunks));
    *fallbackBlocks = ((const achip::sx::ArenaHeader*)scratch.v.data())->fallbackBlocks;
    return r;
}
extern "C" int emu_lzo_size(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t* outSize, int32_t* status, int64_t* errOffset, int32_t n)
{
    const achip::SizeArgs s{srcBase, srcOff, srcLen, outSize, status, errOffset, n};
    return (int)achip::launch_decoded_size(ACHIP_OP_LZO_DECOMPRESS, s, nullptr, nullptr);
}
#endif
