// achip_zstd_frame.h -- what the HOST reads of a Zstd frame, stated once: the frame header (readFrameHeader, M/zstd/ZstdFrameDecompressor.java:865-947),
// the three-byte block header (:156-181), and the two decisions of the incremental reader (abi_zstd_stream.cpp) that are functions of those -- how far a
// frame's decoder must be able to look back, and which whole blocks of the buffered input make the next step.  achip_zstd_decompressed_size and
// achip_zstd_decompress_bound (abi_context.cpp) and achip_zstdstream_decompress_feed read frames through these; so does tools/hostemu/check_zstd.py --stream.
// Plain C++17: no HIP, no device (tests/test_host_plan.py compiles it alone).  The device's own frame parsing is zstd_dec_common.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/aircompressor_hip.h"

namespace achip {
namespace zframe __attribute__((visibility("hidden"))) {  // (inline code of the host units: not the library's interface)

constexpr uint32_t kMagic = 0xFD2FB528u, kMagicV07 = 0xFD2FB527u;
constexpr int32_t kMaxBlock = 131072;  // MAX_BLOCK_SIZE :278

// the four magic bytes: 0, or the detail they are refused with (verifyMagic :949-962)
inline int32_t magic_detail(const uint8_t* p)
{
    const uint32_t magic = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return magic == kMagic ? 0 : (magic == kMagicV07 ? ACHIP_D_ZSTD_V07_MAGIC : ACHIP_D_ZSTD_BAD_MAGIC);
}

struct FrameHeader {
    enum State { OK, NEED_MORE, FAILED };
    State state = NEED_MORE;
    int32_t detail = 0;         // FAILED: why
    int64_t offset = 0;         // FAILED / NEED_MORE: where, counted from the descriptor byte
    int32_t headerSize = 0;     // descriptor byte included, magic not
    bool singleSegment = false, hasChecksum = false;
    int64_t windowSize = -1;    // -1: no window descriptor (a single-segment frame)
    int64_t contentSize = -1;   // -1: not set
    bool contentBeyondInt64 = false;  // an 8-byte content size >= 2^63 (reads negative in Java: "not set"); contentSize is -1 then
};

// The header behind the magic: p[0] is the frame descriptor, `have` bytes lie there.
inline FrameHeader read_frame_header(const uint8_t* p, int64_t have)
{
    FrameHeader h;
    if (have < 1) return h;
    const int32_t fhd = p[0];
    h.singleSegment = (fhd & 0x20) != 0;
    h.hasChecksum = (fhd & 0x04) != 0;
    const int32_t dictDesc = fhd & 3, csDesc = fhd >> 6;
    h.headerSize = 1 + (h.singleSegment ? 0 : 1) + (dictDesc == 0 ? 0 : (1 << (dictDesc - 1))) + (csDesc == 0 ? (h.singleSegment ? 1 : 0) : (1 << csDesc));
    h.offset = 1;
    if (have < h.headerSize) return h;
    int32_t at = 1;
    if (!h.singleSegment) {
        const int32_t wd = p[at++];
        const int64_t base = 1LL << (10 + (wd >> 3));
        h.windowSize = base + (base / 8) * (wd & 7);
    }
    h.offset = at;
    if (dictDesc != 0) {
        h.state = FrameHeader::FAILED;
        h.detail = ACHIP_D_ZSTD_DICTIONARY;
        h.offset = at + (1 << (dictDesc - 1));
        return h;
    }
    const int n = csDesc == 0 ? (h.singleSegment ? 1 : 0) : (1 << csDesc);
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint64_t)p[at + i] << (8 * i);
    if (n > 0) h.contentSize = (int64_t)v + (csDesc == 1 ? 256 : 0);
    if (csDesc == 3 && v > (uint64_t)INT64_MAX) {
        h.contentSize = -1;
        h.contentBeyondInt64 = true;
    }
    h.state = FrameHeader::OK;
    return h;
}

struct BlockHeader {
    int32_t type;    // 0 RAW, 1 RLE, 2 compressed, 3 reserved
    int32_t size;    // the size field: what a RAW / RLE block decodes to, what a compressed block stores
    bool last;
    int64_t stored;  // bytes behind the header (an RLE block stores one)
};
inline BlockHeader read_block_header(const uint8_t* p)
{
    const int32_t h = p[0] | (p[1] << 8) | (p[2] << 16);
    const int32_t type = (h >> 1) & 3, size = h >> 3;
    return BlockHeader{type, size, (h & 1) != 0, type == 1 ? 1 : (int64_t)size};
}

// How far back the decoder of a frame must be able to look (FrameHeader.computeRequiredOutputBufferLookBackSize), and what the incremental reader does with large
// windows:
//  * a window descriptor above 8 MiB (MAX_WINDOW_SIZE): Java fails the frame's first COMPRESSED block ("Window size too large", ZstdFrameDecompressor
//    .java:303) and copies RAW / RLE blocks as they come -- so does the reader (windowBeyondJava, checked where the blocks are listed: list_step);
//  * a single-segment frame (no descriptor: Java's windowSize is -1 and the check above passes) of any content size: Java decodes it in a buffer
//    that never grows beyond 8 MiB + a block (ZstdIncrementalFrameDecompressor.java:318-336) -- the reader keeps min(content size, maxWindow) behind
//    the position, i.e. it decodes every such stream the Java reader decodes, to the same bytes, and in addition accepts offsets between
//    Java's buffer and maxWindow that Java refuses;
//  * output is handed out block by block, where Java holds a window's worth back: an error in a later block is reported after bytes the
//    Java reader would not have delivered yet (tests/test_gpu_zstd_stream.py: "everything the reference delivered is a prefix").
struct FrameWindow {
    int64_t lookBack;       // < 0: refused (ACHIP_D_ZSTD_WINDOW_TOO_LARGE at the frame header)
    bool windowBeyondJava;
};
inline FrameWindow frame_window(const FrameHeader& h, int64_t maxWindow)
{
    const int64_t w = h.windowSize, c = h.contentSize;
    int64_t lookBack = c < 0 ? w : (w < 0 ? c : std::min(w, c));
    if (h.singleSegment && lookBack > maxWindow) lookBack = maxWindow;
    if (lookBack < 0 || lookBack > maxWindow) lookBack = w >= 0 && w <= maxWindow ? w : -1;
    return FrameWindow{lookBack, !h.singleSegment && w > (8LL << 20)};
}

// A block of a step: its three header bytes as the step's stand-in frame will carry them (type and size; the stand-in frame sets the "last" bit itself), its payload
// at p + dataPos, and what it accounts for of the STREAM's bytes (a RAW / RLE block beyond 128 KiB is handed over as several).
struct StepBlock {
    int32_t header;
    size_t dataPos;
    int64_t dataLen;
    int64_t streamBytes;
};
struct Step {
    enum Broken { NONE, BLOCK_TYPE, WINDOW };
    std::vector<StepBlock> blocks;
    int64_t bytes = 0;      // of p, block headers included (the checksum word not)
    bool closing = false;   // the frame's last block is among them
    uint32_t expected = 0;  // closing, a frame with checksum: the checksum word
    Broken broken = NONE;   // the block behind the listed ones cannot be decoded (at p + bytes; its error offset is behind its header: + 3)
};
// The whole blocks that lie in [p, p + have), up to a step of maxBlocks.
inline Step list_step(const uint8_t* p, int64_t have, bool hasChecksum, bool windowBeyondJava, int32_t maxBlocks)
{
    Step s;
    int64_t at = 0;
    while ((int32_t)s.blocks.size() < maxBlocks) {
        if (have - at < 3) break;
        const BlockHeader b = read_block_header(p + at);
        if (b.type == 3 || (b.type == 2 && b.size > kMaxBlock)) {
            // ("Invalid block type" :264; a compressed block beyond Block_Maximum_Size -- "Expected match length table to be present" or worse in Java -- would outgrow a step's room)
            s.broken = Step::BLOCK_TYPE;
            break;
        }
        if (b.type == 2 && windowBeyondJava) {  // ("Window size too large (not yet supported)" :303: the frame's first compressed block)
            s.broken = Step::WINDOW;
            break;
        }
        if (have - at < 3 + b.stored) break;
        if (b.last && hasChecksum) {
            if (have - at < 3 + b.stored + 4) break;  // (the frame's last block goes with its checksum word)
            const uint8_t* c = p + at + 3 + b.stored;
            s.expected = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
        }
        // A RAW or RLE block may say any size up to 2^21 - 1: ZstdIncrementalFrameDecompressor.java:204-226 copies / fills that many bytes (no encoder writes such a
        // block, the format forbids it, the Java reader does not check).  Here it becomes blocks of at most 128 KiB each -- the same bytes, and such blocks touch
        // neither tables nor repeat offsets -- so that a step's room holds them; a step that has no room left for all of them ends in front of the block.
        const int32_t parts = b.type == 2 || b.size <= kMaxBlock ? 1 : (b.size + kMaxBlock - 1) / kMaxBlock;
        if ((int32_t)s.blocks.size() + parts > maxBlocks) {
            break;  // (at most 16 parts: an empty step of 32 always has room)
        }
        for (int32_t k = 0; k < parts; k++) {
            const int32_t partSize = parts == 1 ? b.size : std::min(kMaxBlock, b.size - kMaxBlock * k);
            StepBlock sb;
            sb.header = (b.type << 1) | (partSize << 3);
            sb.dataPos = (size_t)at + 3 + (b.type == 0 ? (size_t)kMaxBlock * (size_t)k : 0);
            sb.dataLen = b.type == 1 ? 1 : partSize;
            sb.streamBytes = (k == 0 ? 3 : 0) + (b.type == 1 ? (k == 0 ? 1 : 0) : partSize);
            s.blocks.push_back(sb);
        }
        at += 3 + b.stored;
        if (b.last) {
            s.closing = true;
            break;
        }
    }
    s.bytes = at;
    return s;
}

}  // namespace zframe
}  // namespace achip
