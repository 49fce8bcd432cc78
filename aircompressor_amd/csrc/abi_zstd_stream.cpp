// abi_zstd_stream.cpp -- the two incremental Zstd streams of the C ABI: a reader that decodes one long stream a step at a time, and a writer that is
// ZstdOutputStream on the device.  What the reader decides from the bytes alone -- frame header, block headers, which blocks make a step -- is achip_zstd_frame.h's.
#include "achip_host.h"

#include "achip_zstd_frame.h"

using namespace achip::host;
using achip::zframe::StepBlock;

extern "C" {

// ---- one long Zstd stream, decoded a step at a time in bounded memory ----------------------------------------------------
// What ZstdInputStream does over ZstdIncrementalFrameDecompressor (M/zstd/ZstdIncrementalFrameDecompressor.java:44-72: the states; :216-234: the
// window kept behind the output): input arrives in pieces, output leaves in pieces, a frame may be any length, frames may follow each other.
// The host walks magic / frame header / block headers (three bytes each) and hands the device STEPS of whole blocks -- up to kStepBlocks, i.e.
// 4 MiB of output -- which the pipeline's multi-block stages decode with tables, repeat offsets, window and running checksum carried from step
// to step (zstd_decompress_pipe.hip: launch_zstd_stream_step).  Memory per open stream: the window (at most kMaxWindow) twice + a step of
// output on the device, a step of input and of output on the host, the stages' scratch for one step: ~45 MB at the 8 MiB window of the Java
// writer, whatever the stream's length.
namespace {
struct achip_zstd_dstream {
    static constexpr int32_t kStepBlocks = 32;
    static constexpr int32_t kStepBytes = kStepBlocks * 131072;
    static constexpr int64_t kMaxWindow = 128LL << 20;  // (window descriptors beyond 2^27: refused -- the Java frame decoder stops at 8 MiB, :303)
    ~achip_zstd_dstream() { (void)hipSetDevice(ctx->device); }  // (the members free what they hold)
    bool frameDone = false;  // a frame has been read to its end: from then on the stream may end quietly between frames (the Java decoder's INITIAL state is not a stopping point)
    enum Phase { MAGIC = 0, HEADER = 1, BLOCKS = 2, FAILED = 3 };
    achip_ctx* ctx = nullptr;
    int phase = MAGIC;
    std::vector<uint8_t> pending;  // input accepted, not decoded yet
    size_t pendingAt = 0;          // ... from here on
    int64_t streamPos = 0;         // stream offset of pending[pendingAt]
    // the frame under way
    int64_t lookBack = 0;          // FrameHeader.computeRequiredOutputBufferLookBackSize
    bool hasChecksum = false;
    bool windowBeyondJava = false; // the frame's window descriptor says more than 8 MiB: its first compressed block fails as in Java (:303), RAW / RLE blocks pass
    // output decoded, not delivered yet
    PinnedBuffer<uint8_t> hostOut;  // kStepBytes
    int64_t outLen = 0, outAt = 0;
    int32_t failStatus = 0;
    int64_t failOffset = 0;
    // device
    DeviceBuffer<uint8_t> hist;    // [0, window) history (ending at `window`) | [window, window + kStepBytes) a step's output | [.., + window) room to move the history
    int64_t window = 0;            // bytes of history room
    int64_t histLen = 0;           // history bytes held (at hist + window - histLen)
    DeviceBuffer<uint8_t> dSrc;    // 6 + kStepBytes + 4 * kStepBlocks + 64
    PinnedBuffer<uint8_t> hostSrc;  // the same
    DeviceBuffer<> carry;
    DeviceBuffer<> scratch;
    int64_t scratchBytes = 0;
};

constexpr int64_t kStepSrcBytes = 6 + (int64_t)achip_zstd_dstream::kStepBytes + 4 * achip_zstd_dstream::kStepBlocks + 64;

int32_t dstream_fail(achip_zstd_dstream* z, int detail, int64_t offset)
{
    z->phase = achip_zstd_dstream::FAILED;
    z->failStatus = ACHIP_STATUS(ACHIP_CLASS_MALFORMED, detail);
    z->failOffset = offset;
    return z->failStatus;
}

// the history room for a frame whose decoder must be able to look `lookBack` bytes back (grown, never shrunk)
int32_t dstream_window(achip_zstd_dstream* z, int64_t lookBack)
{
    const int64_t want = std::max<int64_t>((lookBack + 255) & ~255LL, 1 << 16);
    if (want > z->window) {
        if (z->hist) {
            HIP_TRY(hipStreamSynchronize(z->ctx->stream.get()));
            z->window = 0;
            HIP_TRY(z->hist.reset());
        }
        HIP_TRY(z->hist.alloc((size_t)(2 * want + achip_zstd_dstream::kStepBytes + 256)));
        z->window = want;
    }
    z->histLen = 0;
    return 0;
}

// Decodes a step: the blocks list_step (achip_zstd_frame.h) found whole at pending[pendingAt ...].
int32_t dstream_step(achip_zstd_dstream* z, const std::vector<StepBlock>& list, bool closing, uint32_t expected)
{
    achip_ctx* ctx = z->ctx;
    const int32_t blocks = (int32_t)list.size();
    // the step as a frame of its own: magic, a descriptor that says "single segment, one byte of content size, no checksum", the size byte, the blocks
    uint8_t* h = z->hostSrc.get();
    const uint8_t head[6] = {0x28, 0xB5, 0x2F, 0xFD, 0x20, 0x00};
    memcpy(h, head, 6);
    int64_t at = 6;
    for (int32_t i = 0; i < blocks; i++) {
        const StepBlock& b = list[(size_t)i];
        const int32_t hd = (b.header & ~1) | (i == blocks - 1 ? 1 : 0);  // the step's last block closes the stand-in frame
        h[at] = (uint8_t)hd;
        h[at + 1] = (uint8_t)(hd >> 8);
        h[at + 2] = (uint8_t)(hd >> 16);
        memcpy(h + at + 3, z->pending.data() + z->pendingAt + b.dataPos, (size_t)b.dataLen);
        at += 3 + b.dataLen;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(z->dSrc.get(), h, (size_t)at, hipMemcpyHostToDevice, ctx->stream.get()));
    int32_t result[3] = {0, 0, -1};
    // positions count from the oldest history byte kept: the step writes from histLen on
    uint8_t* dOut = z->hist.get() + (z->window - z->histLen);
    HIP_TRY(achip::launch_zstd_stream_step(ctx->stream.get(), z->scratch.get(), z->scratchBytes, z->carry.get(), z->dSrc.get(), (int32_t)at, blocks, dOut, (int32_t)z->histLen,
                                           (int32_t)(z->histLen + achip_zstd_dstream::kStepBytes), closing ? 1 : 0, z->hasChecksum ? 1 : 0, expected, result, ctx->kernel));
    const int32_t good = result[0], produced = result[1];
    if (produced > 0) {
        HIP_TRY(hipMemcpyAsync(z->hostOut.get(), z->hist.get() + z->window, (size_t)produced, hipMemcpyDeviceToHost, ctx->stream.get()));
        // the history for the next step: the last min(window, histLen + produced) bytes, ending where the step's output begins
        const int64_t keep = std::min<int64_t>(z->lookBack, z->histLen + produced);
        uint8_t* from = z->hist.get() + z->window + produced - keep;
        uint8_t* to = z->hist.get() + z->window - keep;
        if (produced >= keep) {
            HIP_TRY(hipMemcpyAsync(to, from, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream.get()));
        }
        else {  // (the ranges overlap: by way of the room behind the step's output)
            uint8_t* tmp = z->hist.get() + z->window + achip_zstd_dstream::kStepBytes;
            HIP_TRY(hipMemcpyAsync(tmp, from, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream.get()));
            HIP_TRY(hipMemcpyAsync(to, tmp, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream.get()));
        }
        z->histLen = keep;
        HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    }
    z->outLen = produced;
    z->outAt = 0;
    if (good < blocks) {
        // the stream is damaged in block `good`: what lies in front of it is delivered first (the next calls), then the stream fails
        int64_t off = z->streamPos;
        for (int32_t i = 0; i < good; i++) off += list[(size_t)i].streamBytes;
        dstream_fail(z, ACHIP_D_ZSTD_CORRUPTED, off);
        return 0;
    }
    if (closing && z->hasChecksum && result[2] != 1) {
        int64_t off = z->streamPos;
        for (int32_t i = 0; i < blocks; i++) off += list[(size_t)i].streamBytes;
        dstream_fail(z, ACHIP_D_ZSTD_BAD_CHECKSUM, off + 4);  // (ZstdIncrementalFrameDecompressor.java:318-320: behind the checksum word)
        return 0;
    }
    return 0;
}
}  // namespace

void* achip_zstdstream_decompress_begin(achip_ctx* ctx)
{
    if (!ctx) {
        g_lastError = "ctx is null";
        return nullptr;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        g_lastError = "hipSetDevice failed";
        return nullptr;
    }
    achip_zstd_dstream* z = new achip_zstd_dstream();
    z->ctx = ctx;
    z->scratchBytes = achip::zstd_stream_step_scratch_bytes(achip_zstd_dstream::kStepBlocks);
    bool ok = z->hostOut.alloc((size_t)achip_zstd_dstream::kStepBytes) == hipSuccess;
    ok = ok && z->hostSrc.alloc((size_t)kStepSrcBytes) == hipSuccess;
    ok = ok && z->dSrc.alloc((size_t)kStepSrcBytes) == hipSuccess;
    ok = ok && z->carry.alloc((size_t)achip::zstd_stream_carry_bytes()) == hipSuccess;
    ok = ok && z->scratch.alloc((size_t)z->scratchBytes) == hipSuccess;
    if (!ok) {
        g_lastError = "out of memory for a Zstd stream's buffers";
        delete z;
        return nullptr;
    }
    return z;
}

int32_t achip_zstdstream_decompress_end(achip_ctx* ctx, void* state)
{
    (void)ctx;
    delete (achip_zstd_dstream*)state;
    return 0;
}

int32_t achip_zstdstream_decompress_at_stopping_point(void* state)
{
    const achip_zstd_dstream* z = (const achip_zstd_dstream*)state;
    if (!z) return 0;
    // (state == READ_FRAME_MAGIC, whatever lies buffered: fewer than four bytes behind the last frame end the stream quietly -- ZstdInputStream.java:81-86,
    //  ZstdIncrementalFrameDecompressor.isAtStoppingPoint)
    return z->phase == achip_zstd_dstream::MAGIC && z->frameDone && z->outAt == z->outLen ? 1 : 0;
}

int32_t achip_zstdstream_decompress_feed(achip_ctx* ctx, void* state, const void* src, int64_t srcLen, void* dst, int64_t dstCap, int64_t* consumed, int64_t* produced,
                                         int64_t* errOffset)
{
    achip_zstd_dstream* z = (achip_zstd_dstream*)state;
    if (!ctx || !z || z->ctx != ctx) return bad_argument("stream state");
    if (srcLen < 0 || dstCap < 0 || (srcLen > 0 && !src) || (dstCap > 0 && !dst) || !consumed || !produced) return bad_argument("buffers");
    *consumed = 0;
    *produced = 0;
    if (errOffset) *errOffset = 0;
    const uint8_t* in = (const uint8_t*)src;
    uint8_t* out = (uint8_t*)dst;
    // what the stream may hold back of the caller's input: a step of blocks with their headers, the frame's checksum, the next frame's header
    const size_t holdLimit = (size_t)kStepSrcBytes + 64;
    for (;;) {
        // ---- decoded bytes first ----
        if (z->outAt < z->outLen) {
            const int64_t n = std::min<int64_t>(z->outLen - z->outAt, dstCap - *produced);
            if (n > 0) {
                memcpy(out + *produced, z->hostOut.get() + z->outAt, (size_t)n);
                z->outAt += n;
                *produced += n;
            }
            if (z->outAt < z->outLen) {
                return 0;  // (the caller's buffer is full)
            }
        }
        if (z->phase == achip_zstd_dstream::FAILED) {
            if (errOffset) *errOffset = z->failOffset;
            return *produced > 0 ? 0 : z->failStatus;  // (bytes in front of the damage go out first: the NEXT call fails)
        }
        // ---- take input ----
        if (z->pendingAt > 0 && (z->pendingAt == z->pending.size() || z->pendingAt >= (size_t)(1 << 20))) {
            z->pending.erase(z->pending.begin(), z->pending.begin() + (ptrdiff_t)z->pendingAt);
            z->pendingAt = 0;
        }
        {
            const size_t held = z->pending.size() - z->pendingAt;
            const int64_t take = std::min<int64_t>(srcLen - *consumed, held < holdLimit ? (int64_t)(holdLimit - held) : 0);
            if (take > 0) {
                z->pending.insert(z->pending.end(), in + *consumed, in + *consumed + take);
                *consumed += take;
            }
        }
        const uint8_t* p = z->pending.data() + z->pendingAt;
        const int64_t have = (int64_t)(z->pending.size() - z->pendingAt);
        auto failed = [&](int detail, int64_t offset) -> int32_t {  // (bytes in front of the damage go out first: the NEXT call fails)
            const int32_t st = dstream_fail(z, detail, offset);
            if (errOffset) *errOffset = z->failOffset;
            return *produced > 0 ? 0 : st;
        };
        auto advance = [&](int64_t n) {
            z->pendingAt += (size_t)n;
            z->streamPos += n;
        };
        if (z->phase == achip_zstd_dstream::MAGIC) {
            if (have < 4) {
                return 0;  // (more input, or the end of the stream: achip_zstdstream_decompress_at_stopping_point)
            }
            if (const int32_t detail = achip::zframe::magic_detail(p)) return failed(detail, z->streamPos);
            advance(4);
            z->phase = achip_zstd_dstream::HEADER;
            continue;
        }
        if (z->phase == achip_zstd_dstream::HEADER) {  // ZstdFrameDecompressor.readFrameHeader :860-947 behind determineFrameHeaderSize
            const achip::zframe::FrameHeader fh = achip::zframe::read_frame_header(p, have);
            if (fh.state == achip::zframe::FrameHeader::NEED_MORE) return 0;
            if (fh.state == achip::zframe::FrameHeader::FAILED) return failed(fh.detail, z->streamPos + fh.offset);
            const achip::zframe::FrameWindow w = achip::zframe::frame_window(fh, achip_zstd_dstream::kMaxWindow);  // (what large windows mean here and in Java: achip_zstd_frame.h)
            if (w.lookBack < 0) return failed(ACHIP_D_ZSTD_WINDOW_TOO_LARGE, z->streamPos);
            z->lookBack = w.lookBack;
            z->windowBeyondJava = w.windowBeyondJava;
            z->hasChecksum = fh.hasChecksum;
            int32_t r = dstream_window(z, w.lookBack);
            if (r < 0) return r;
            // ZstdFrameDecompressor.reset() :199-203 and a fresh XxHash64: the carry of a new frame
            {
                std::vector<uint8_t> zero((size_t)achip::zstd_stream_carry_bytes(), 0);
                achip::zstd_stream_carry_init(zero.data());
                HIP_TRY(hipSetDevice(ctx->device));
                // (on the context's stream, where the steps run, and waited for: see achip_zstdstream_compress_begin)
                HIP_TRY(hipMemcpyAsync(z->carry.get(), zero.data(), zero.size(), hipMemcpyHostToDevice, ctx->stream.get()));
                HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
            }
            advance(fh.headerSize);
            z->phase = achip_zstd_dstream::BLOCKS;
            continue;
        }
        // ---- BLOCKS: the whole blocks that lie in pending, up to a step ----
        const achip::zframe::Step step = achip::zframe::list_step(p, have, z->hasChecksum, z->windowBeyondJava, achip_zstd_dstream::kStepBlocks);
        const std::vector<StepBlock>& list = step.blocks;
        const bool closing = step.closing;
        if (list.empty()) {
            if (step.broken != achip::zframe::Step::NONE) return failed(step.broken == achip::zframe::Step::WINDOW ? ACHIP_D_ZSTD_WINDOW_TOO_LARGE : ACHIP_D_ZSTD_INVALID_BLOCK_TYPE, z->streamPos + 3);
            if (*consumed == srcLen) {
                return 0;  // (a block is not whole yet: more input)
            }
            continue;  // (there was room for more of the caller's input)
        }
        const int32_t r = dstream_step(z, list, closing, step.expected);
        if (r < 0) return r;
        if (z->phase != achip_zstd_dstream::FAILED) {
            advance(step.bytes + (closing && z->hasChecksum ? 4 : 0));
            if (closing) {
                z->phase = achip_zstd_dstream::MAGIC;
                z->frameDone = true;
            }
        }
    }
}

// ---- ... and written a chunk at a time: ZstdOutputStream (M/zstd/ZstdOutputStream.java:93-221) in the 4 MiB it buffers --------------------------
// write() appends to the stream's buffer -- here on the device --, a full buffer is flushed (compressIfNecessary :122-131: whole blocks, the
// window and one block stay), close() writes the rest and the checksum.  One kernel step per writeChunk (zstd_stream.hip:
// zstd_ostream_step_kernel), the CompressionContext between the steps in a device-side record.  The bytes are the Java stream's whatever the
// sizes of the write() calls: the flush schedule only depends on how many bytes have arrived.
namespace {
struct achip_zstd_cstream {
    static constexpr int32_t kBuffer = 4 << 20, kWindow = 1 << 20, kBlock = 131072;   // maxBufferSize = 4 x window (:52-54), level 3 / unknown size
    static constexpr int32_t kOutBytes = kBuffer + (kBuffer >> 7) + 4096;              // a step's blocks + their headers + frame header + checksum
    ~achip_zstd_cstream() { (void)hipSetDevice(ctx->device); }  // (the members free what they hold)
    achip_ctx* ctx = nullptr;
    DeviceBuffer<uint8_t> buf;      // the stream's buffer
    DeviceBuffer<uint8_t> dOut;     // a step's output
    PinnedBuffer<uint8_t> hostOut;  // the same, on its way to the caller
    DeviceBuffer<> state;
    DeviceBuffer<> slab;
    int32_t position = 0, offset = 0;  // uncompressedPosition, uncompressedOffset
    int64_t outLen = 0, outAt = 0;
    bool finished = false;
    int32_t failStatus = 0;
};

// writeChunk(lastChunk) :154-221
int32_t cstream_step(achip_zstd_cstream* z, bool closing)
{
    achip_ctx* ctx = z->ctx;
    const int32_t chunk = closing ? z->position - z->offset : ((z->position - z->offset - achip_zstd_cstream::kWindow - achip_zstd_cstream::kBlock) / achip_zstd_cstream::kBlock) * achip_zstd_cstream::kBlock;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(achip::launch_zstd_ostream_step(ctx->stream.get(), z->state.get(), z->slab.get(), z->buf.get(), z->offset, chunk, closing ? 1 : 0, z->dOut.get(), achip_zstd_cstream::kOutBytes));
    int32_t result[2] = {0, 0};  // outSize, status (ZstdOStreamState words 8 and 9)
    HIP_TRY(hipMemcpyAsync(result, (const int32_t*)z->state.get() + 8, sizeof(result), hipMemcpyDeviceToHost, ctx->stream.get()));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    if (result[1] != 0) {
        z->failStatus = result[1];
        return result[1];
    }
    if (result[0] > 0) {
        HIP_TRY(hipMemcpyAsync(z->hostOut.get(), z->dOut.get(), (size_t)result[0], hipMemcpyDeviceToHost, ctx->stream.get()));
    }
    z->offset += chunk;
    if (!closing) {
        // the window and the bytes not yet compressed move to the buffer's front (:214-219: System.arraycopy, i.e. memmove).  Source and destination
        // OVERLAP at every flush of a full buffer (slide 1.875 MiB, 2.125 MiB to move), and an overlapping hipMemcpy is undefined: the move is made
        // in pieces of at most `slide` bytes, front to back on the one stream -- a piece's destination ends where its source begins, and a piece has
        // been read before the next one overwrites it
        const int32_t slide = z->offset - achip_zstd_cstream::kWindow;
        const int32_t toMove = achip_zstd_cstream::kWindow + (z->position - z->offset);
        for (int32_t at = 0; at < toMove && slide > 0; at += slide) {
            const int32_t n = std::min(slide, toMove - at);
            HIP_TRY(hipMemcpyAsync(z->buf.get() + at, z->buf.get() + at + slide, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream.get()));
        }
        z->offset -= slide;
        z->position -= slide;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    z->outLen = result[0];
    z->outAt = 0;
    return 0;
}

int64_t cstream_deliver(achip_zstd_cstream* z, uint8_t* out, int64_t room)
{
    const int64_t n = std::min<int64_t>(z->outLen - z->outAt, room);
    if (n > 0) {
        memcpy(out, z->hostOut.get() + z->outAt, (size_t)n);
        z->outAt += n;
    }
    return n > 0 ? n : 0;
}
}  // namespace

void* achip_zstdstream_compress_begin(achip_ctx* ctx)
{
    if (!ctx) {
        g_lastError = "ctx is null";
        return nullptr;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        g_lastError = "hipSetDevice failed";
        return nullptr;
    }
    achip_zstd_cstream* z = new achip_zstd_cstream();
    z->ctx = ctx;
    const size_t stateBytes = (size_t)achip::zstd_ostream_state_bytes();
    bool ok = z->hostOut.alloc((size_t)achip_zstd_cstream::kOutBytes) == hipSuccess;
    ok = ok && z->buf.alloc((size_t)achip_zstd_cstream::kBuffer + 256) == hipSuccess;
    ok = ok && z->dOut.alloc((size_t)achip_zstd_cstream::kOutBytes) == hipSuccess;
    ok = ok && z->state.alloc(stateBytes) == hipSuccess;
    ok = ok && z->slab.alloc((size_t)achip::zstd_ostream_slab_bytes()) == hipSuccess;
    // (on the context's stream, where the steps run: a hipMemset on the null stream is not ordered in front of work on a non-blocking stream, and an empty stream's
    // only step -- begin, close -- then met whatever the allocation held: found by tools/fuzz_zstd_stream.py as a frame without its header)
    ok = ok && hipMemsetAsync(z->state.get(), 0, stateBytes, ctx->stream.get()) == hipSuccess;
    if (!ok) {
        g_lastError = "out of memory for a Zstd stream's buffers";
        delete z;
        return nullptr;
    }
    return z;
}

int32_t achip_zstdstream_compress_end(achip_ctx* ctx, void* state)
{
    (void)ctx;
    delete (achip_zstd_cstream*)state;
    return 0;
}

// write(src, 0, srcLen) :93-104, as far as dst has room for what the flushes on the way put out
int32_t achip_zstdstream_compress_feed(achip_ctx* ctx, void* state, const void* src, int64_t srcLen, void* dst, int64_t dstCap, int64_t* consumed, int64_t* produced)
{
    achip_zstd_cstream* z = (achip_zstd_cstream*)state;
    if (!ctx || !z || z->ctx != ctx) return bad_argument("stream state");
    if (srcLen < 0 || dstCap < 0 || (srcLen > 0 && !src) || (dstCap > 0 && !dst) || !consumed || !produced) return bad_argument("buffers");
    if (z->finished) return bad_argument("Stream is closed");
    *consumed = 0;
    *produced = 0;
    if (z->failStatus != 0) return z->failStatus;
    const uint8_t* in = (const uint8_t*)src;
    for (;;) {
        *produced += cstream_deliver(z, (uint8_t*)dst + *produced, dstCap - *produced);
        if (z->outAt < z->outLen || *consumed == srcLen) {
            return 0;  // (the caller's buffer is full, or everything is taken)
        }
        const int64_t take = std::min<int64_t>(srcLen - *consumed, achip_zstd_cstream::kBuffer - z->position);
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMemcpyAsync(z->buf.get() + z->position, in + *consumed, (size_t)take, hipMemcpyHostToDevice, ctx->stream.get()));
        HIP_TRY(hipStreamSynchronize(ctx->stream.get()));  // (the caller's memory is its own again when the call returns)
        z->position += (int32_t)take;
        *consumed += take;
        if (z->position == achip_zstd_cstream::kBuffer) {  // compressIfNecessary :122-131
            const int32_t r = cstream_step(z, false);
            if (r < 0) return r;
        }
    }
}

// close() :143-152: the last chunk and the checksum; returns 1 when the stream's last byte has been delivered, 0 when dst was too small for the rest
// (call again), a negative status otherwise
int32_t achip_zstdstream_compress_finish(achip_ctx* ctx, void* state, void* dst, int64_t dstCap, int64_t* produced)
{
    achip_zstd_cstream* z = (achip_zstd_cstream*)state;
    if (!ctx || !z || z->ctx != ctx) return bad_argument("stream state");
    if (dstCap < 0 || (dstCap > 0 && !dst) || !produced) return bad_argument("buffers");
    *produced = 0;
    if (z->failStatus != 0) return z->failStatus;
    *produced += cstream_deliver(z, (uint8_t*)dst, dstCap);
    if (z->outAt < z->outLen) {
        return 0;
    }
    if (!z->finished) {
        const int32_t r = cstream_step(z, true);
        if (r < 0) return r;
        z->finished = true;
        *produced += cstream_deliver(z, (uint8_t*)dst + *produced, dstCap - *produced);
    }
    return z->outAt < z->outLen ? 0 : 1;
}

}  // extern "C"
