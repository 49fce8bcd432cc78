// lz4_frame_head.h -- the LZ4 frame format's constants and the frame header as Lz4FrameCompression.decompressFrame reads it
// (M/lz4/Lz4FrameCompression.java:184-232), for the reader (lz4_frame.hip) and the size query (decoded_size.hip): one statement of the header's verdicts.
#pragma once
#include "achip_xxhash.h"

namespace achip {
namespace lz4f {
constexpr uint32_t MAGIC = 0x184D2204u, SKIPPABLE_MAGIC = 0x184D2A50u, SKIPPABLE_MASK = 0xFFFFFFF0u;
constexpr int FLG_BLOCK_INDEPENDENCE = 1 << 5, FLG_BLOCK_CHECKSUM = 1 << 4, FLG_CONTENT_SIZE = 1 << 3, FLG_CONTENT_CHECKSUM = 1 << 2, FLG_DICTIONARY_ID = 1;
constexpr int FLG_RESERVED_MASK = 0x02, BD_RESERVED_MASK = 0x8F;
constexpr int HEADER_SIZE = 7;
constexpr uint32_t UNCOMPRESSED_FLAG = 0x80000000u;

struct FrameHeader {
    int32_t blockMax;  // 64 KiB, 256 KiB, 1 MiB, 4 MiB (Lz4FrameFormat.java:58-67)
    bool blockChecksum, contentSize, contentChecksum;
    bool linked;           // the block-independence bit is clear: a block's matches may reach into the frame's content in front of it (acceptLinked readers only)
    int64_t expectedSize;  // -1: the frame does not announce its content size
    int32_t firstBlock;    // position of the first block's length
};

// The header of the frame whose magic stands at frameStart (the caller has read it): 0, or the status of the reader's exception with its offset in eo.
// acceptLinked (achip_ctx_set_lz4frame_linked_blocks; nothing in the reference): a clear block-independence bit is recorded in h.linked where the Java reader throws.
__device__ __forceinline__ int32_t read_frame_header(const uint8_t* __restrict__ in, int32_t inLen, int32_t frameStart, bool acceptLinked, FrameHeader& h, int64_t& eo)
{
#define LZ4F_HEAD_FAIL(detail, off)                      \
    {                                                    \
        eo = (int64_t)(off);                             \
        return mk_status(ACHIP_CLASS_MALFORMED, detail); \
    }
    const int32_t dstart = frameStart + 4;
    if (dstart + 2 > inLen) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_TRUNC_HEADER, dstart);
    const int flg = in[dstart], bd = in[dstart + 1];
    const int version = (flg >> 6) & 3;
    if (version != 1) LZ4F_HEAD_FAIL(version == 0 ? ACHIP_D_LZ4F_VERSION_0 : (version == 2 ? ACHIP_D_LZ4F_VERSION_2 : ACHIP_D_LZ4F_VERSION_3), dstart);
    if ((flg & FLG_RESERVED_MASK) != 0 || (bd & BD_RESERVED_MASK) != 0) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_RESERVED_BITS, dstart);
    h.blockChecksum = (flg & FLG_BLOCK_CHECKSUM) != 0;
    h.contentSize = (flg & FLG_CONTENT_SIZE) != 0;
    h.contentChecksum = (flg & FLG_CONTENT_CHECKSUM) != 0;
    h.linked = (flg & FLG_BLOCK_INDEPENDENCE) == 0;
    if (h.linked && !acceptLinked) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_LINKED_BLOCKS, dstart);
    if ((flg & FLG_DICTIONARY_ID) != 0) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_DICTIONARY, dstart);
    const int sizeId = (bd >> 4) & 7;
    if (sizeId < 4) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_BLOCK_MAX_SIZE, dstart + 1);
    h.blockMax = 1 << (8 + 2 * sizeId);
    int32_t p = dstart + 2;
    if ((int64_t)p + (h.contentSize ? 8 : 0) + 1 > inLen) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_TRUNC_HEADER, p);
    h.expectedSize = -1;
    if (h.contentSize) {
        h.expectedSize = (int64_t)ld8(in + p);
        p += 8;
    }
    const int expectedHc = in[p];
    const int actualHc = (int)((xxh32_short(in + dstart, p - dstart) >> 8) & 0xFF);
    if (expectedHc != actualHc) LZ4F_HEAD_FAIL(ACHIP_D_LZ4F_HEADER_CHECKSUM, p);
    h.firstBlock = p + 1;
    return 0;
#undef LZ4F_HEAD_FAIL
}
}  // namespace lz4f
}  // namespace achip
