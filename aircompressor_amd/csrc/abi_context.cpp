// abi_context.cpp -- the context of libaircompressor_hip.so's C ABI (include/aircompressor_hip.h), and what needs no codec kernel: create / destroy, options
// and statistics, device / host memory and event helpers, statuses and their texts, and the size functions that are host arithmetic.
//
// Mirrors what the reference's FFM layer expects from a native codec library
// (M/internal/NativeLoader.java:66-117; M/lz4/Lz4Native.java:30-40): plain C symbols,
// int/long/pointer arguments, integer results.  Depends only on libamdhip64.
#include "achip_host.h"

#include "achip_bounds.h"
#include "achip_zstd_frame.h"

using namespace achip::host;

namespace achip {
namespace host ACHIP_HIDDEN {

thread_local std::string g_lastError;

int32_t device_failure(const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    g_lastError = buf;
    return ACHIP_STATUS(ACHIP_CLASS_DEVICE, ACHIP_D_HIP_ERROR);
}
int32_t bad_argument(const char* what)
{
    g_lastError = what;
    return ACHIP_STATUS(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
}

BatchArgs make_args(const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen,
                    int32_t* status, int64_t* errOffset, int32_t nBlocks)
{
    return BatchArgs{(const uint8_t*)srcBase, srcOff, srcLen, (uint8_t*)dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks, 0};  // (the rest: as BatchArgs says)
}

}  // namespace host
}  // namespace achip

achip_ctx::~achip_ctx()
{
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream.get());
}

namespace {
struct DetailText {
    int32_t detail;
    const char* text;
};
const DetailText kDetailText[] = {
    {ACHIP_D_GENERIC, "Unknown error"},
    {ACHIP_D_LZ4_INPUT_EMPTY, "input is empty"},
    {ACHIP_D_LZ4_MALFORMED, "Malformed input"},
    {ACHIP_D_LZ4_LAST_LITERAL_OUTSIDE, "attempt to write last literal outside of destination buffer"},
    {ACHIP_D_LZ4_INPUT_NOT_CONSUMED, "all input must be consumed"},
    {ACHIP_D_LZ4_OFFSET_OUTSIDE, "offset outside destination buffer"},
    {ACHIP_D_LZ4_LAST_5_LITERALS, "last 5 bytes must be literals"},
    {ACHIP_D_LZ4_EMPTY_OUTPUT, "Output buffer too small"},
    {ACHIP_D_LZ4_MAX_INPUT, "Max input length exceeded"},
    {ACHIP_D_LZ4_MAX_OUTPUT, "Max output length must be larger than the LZ4 bound"},
    {ACHIP_D_LZO_MALFORMED, "Malformed input"},
    {ACHIP_D_LZO_MAX_INPUT, "Max input length exceeded"},
    {ACHIP_D_LZO_MAX_OUTPUT, "Max output length must be larger than the LZO bound"},
    {ACHIP_D_LZ4F_TOO_SHORT, "Input is too short to be an LZ4 frame"},
    {ACHIP_D_LZ4F_TRUNC_MAGIC, "Truncated LZ4 frame: incomplete magic number"},
    {ACHIP_D_LZ4F_BAD_MAGIC, "Invalid LZ4 frame magic number"},
    {ACHIP_D_LZ4F_TRUNC_HEADER, "Truncated LZ4 frame header"},
    {ACHIP_D_LZ4F_VERSION_0, "Unsupported LZ4 frame version: 0"},
    {ACHIP_D_LZ4F_VERSION_2, "Unsupported LZ4 frame version: 2"},
    {ACHIP_D_LZ4F_VERSION_3, "Unsupported LZ4 frame version: 3"},
    {ACHIP_D_LZ4F_RESERVED_BITS, "Corrupt LZ4 frame: reserved bits in the frame descriptor must be zero"},
    {ACHIP_D_LZ4F_LINKED_BLOCKS, "LZ4 frames with linked blocks are not supported"},
    {ACHIP_D_LZ4F_DICTIONARY, "LZ4 frames with a dictionary are not supported"},
    {ACHIP_D_LZ4F_BLOCK_MAX_SIZE, "Invalid LZ4 frame block maximum size"},
    {ACHIP_D_LZ4F_HEADER_CHECKSUM, "Corrupt LZ4 frame: invalid header checksum"},
    {ACHIP_D_LZ4F_MISSING_BLOCK_SIZE, "Truncated LZ4 frame: missing block size"},
    {ACHIP_D_LZ4F_BLOCK_PAST_END, "Truncated LZ4 frame: block extends past end of input"},
    {ACHIP_D_LZ4F_OUTPUT_TOO_SMALL, "Output buffer too small"},
    {ACHIP_D_LZ4F_BLOCK_EXCEEDS_MAX, "Corrupt LZ4 frame: decompressed block exceeds maximum block size"},
    {ACHIP_D_LZ4F_MISSING_BLOCK_CHECKSUM, "Truncated LZ4 frame: missing block checksum"},
    {ACHIP_D_LZ4F_BLOCK_CHECKSUM, "Corrupt LZ4 frame: invalid block checksum"},
    {ACHIP_D_LZ4F_MISSING_CONTENT_CHECKSUM, "Truncated LZ4 frame: missing content checksum"},
    {ACHIP_D_LZ4F_CONTENT_CHECKSUM, "Corrupt LZ4 frame: invalid content checksum"},
    {ACHIP_D_LZ4F_CONTENT_SIZE, "Corrupt LZ4 frame: content size does not match frame header"},
    {ACHIP_D_LZ4F_TRUNC_SKIP_SIZE, "Truncated LZ4 skippable frame: missing frame size"},
    {ACHIP_D_LZ4F_TRUNC_SKIP, "Truncated LZ4 skippable frame"},
    {ACHIP_D_LZ4F_MAX_OUTPUT, "Output buffer too small"},
    {ACHIP_D_SNF_EOF_STREAM_HEADER, "encountered EOF while reading stream header"},
    {ACHIP_D_SNF_BAD_STREAM_HEADER, "invalid stream header"},
    {ACHIP_D_SNF_EOF_BLOCK_HEADER, "encountered EOF while reading block header"},
    {ACHIP_D_SNF_EOF_FRAME, "unexpectd EOF when reading frame"},
    {ACHIP_D_SNF_STREAM_ID_LENGTH, "stream identifier chunk with invalid length"},
    {ACHIP_D_SNF_UNSKIPPABLE, "unsupported unskippable chunk"},
    {ACHIP_D_SNF_INVALID_LENGTH, "invalid length for chunk flag"},
    {ACHIP_D_SNF_CHECKSUM, "Corrupt input: invalid checksum"},
    {ACHIP_D_SNF_OUTPUT_TOO_SMALL, "Output buffer too small for the stream"},
    {ACHIP_D_SNF_MAX_OUTPUT, "Output buffer too small"},
    {ACHIP_D_HDP_TRUNCATED_INT, "Stream is truncated"},
    {ACHIP_D_HDP_EOF_BLOCK_DATA, "encountered EOF while reading block data"},
    {ACHIP_D_HDP_CHUNK_EXCEEDS_BLOCK, "Chunk uncompressed size is greater than block size"},
    {ACHIP_D_HDP_LENGTH_MISMATCH, "Expected to read the chunk's announced bytes, but data only contained fewer"},
    {ACHIP_D_HDP_NOT_CONSUMED, "All input was not consumed"},
    {ACHIP_D_HDP_NEGATIVE_LENGTH, "negative chunk length"},
    {ACHIP_D_HDP_MAX_OUTPUT, "Output buffer too small"},
    {ACHIP_D_SNAPPY_MALFORMED, "Malformed input"},
    {ACHIP_D_SNAPPY_TRUNCATED, "Input is truncated"},
    {ACHIP_D_SNAPPY_LEN_HIGH_BIT, "last byte of compressed length int has high bit set"},
    {ACHIP_D_SNAPPY_INVALID_LENGTH, "invalid compressed length"},
    {ACHIP_D_SNAPPY_LENGTH_MISMATCH, "Recorded length differs from actual length after decompression"},
    {ACHIP_D_SNAPPY_OUTPUT_TOO_SMALL, "Uncompressed length must be less than the output buffer size"},
    {ACHIP_D_SNAPPY_MAX_OUTPUT, "Output buffer must be at least the Snappy bound"},
    {ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, "Not enough input bytes"},
    {ACHIP_D_ZSTD_OUTPUT_TOO_SMALL, "Output buffer too small"},
    {ACHIP_D_ZSTD_CORRUPTED, "Input is corrupted"},
    {ACHIP_D_ZSTD_BAD_MAGIC, "Invalid magic prefix"},
    {ACHIP_D_ZSTD_V07_MAGIC, "Data encoded in unsupported ZSTD v0.7 format"},
    {ACHIP_D_ZSTD_BAD_CHECKSUM, "Bad checksum"},
    {ACHIP_D_ZSTD_DICTIONARY, "Custom dictionaries not supported"},
    {ACHIP_D_ZSTD_INVALID_BLOCK_TYPE, "Invalid block type"},
    {ACHIP_D_ZSTD_BLOCK_TOO_LARGE, "Expected match length table to be present"},
    {ACHIP_D_ZSTD_BLOCK_TOO_SMALL, "Compressed block size too small"},
    {ACHIP_D_ZSTD_WINDOW_TOO_LARGE, "Window size too large (not yet supported)"},
    {ACHIP_D_ZSTD_DICT_CORRUPTED, "Dictionary is corrupted"},
    {ACHIP_D_ZSTD_LITERALS_TOO_LARGE, "Block exceeds maximum size"},
    {ACHIP_D_ZSTD_FSE_TABLE_LOG, "FSE table size exceeds maximum allowed size"},
    {ACHIP_D_ZSTD_FSE_SYMBOL, "Symbol larger than max value"},
    {ACHIP_D_ZSTD_TABLE_MISSING, "Expected match length table to be present"},
    {ACHIP_D_ZSTD_VALUE_TOO_LARGE, "Value exceeds expected maximum value"},
    {ACHIP_D_ZSTD_BITSTREAM_EMPTY, "Bitstream is empty"},
    {ACHIP_D_ZSTD_BITSTREAM_NO_MARK, "Bitstream end mark not present"},
    {ACHIP_D_ZSTD_BITSTREAM_NOT_CONSUMED, "Bit stream is not fully consumed"},
    {ACHIP_D_ZSTD_SEQUENCES_NOT_CONSUMED, "Not all sequences were consumed"},
    {ACHIP_D_ZSTD_FSE_OUTPUT_SMALL, "Output buffer is too small"},
    {ACHIP_D_ZSTD_MAX_OUTPUT, "Output buffer too small"},
    {ACHIP_D_NO_DEVICE, "No HIP device available"},
    {ACHIP_D_HIP_ERROR, "HIP runtime error"},
    {ACHIP_D_BAD_ARGUMENT, "Invalid argument"},
    {ACHIP_D_UNSUPPORTED, "Operation not supported by this build"},
};

// (Lz4FrameCompression.maxCompressedLength  M/lz4/Lz4FrameCompression.java:70-83, and the others after it: a negative size is refused before its bound is
// worked out, a bound beyond an int after)
template <class Bound>
int32_t int_bound(int32_t n, Bound bound)
{
    if (n < 0) return bad_argument("uncompressedSize is negative");
    const int64_t maxLength = bound();
    if (maxLength > 0x7FFFFFFF) return bad_argument("Maximum compressed length exceeds Integer.MAX_VALUE");
    return (int32_t)maxLength;
}
}  // namespace

extern "C" {

int32_t achip_status_class(int32_t status) { return status < 0 ? ((-status) & 15) : 0; }
int32_t achip_status_detail(int32_t status) { return status < 0 ? ((-status) >> 4) : 0; }

const char* achip_detail_message(int32_t detail)
{
    for (const DetailText& d : kDetailText) {
        if (d.detail == detail) {
            return d.text;
        }
    }
    return "Unknown error";
}

const char* achip_version(void) { return "aircompressor-hip 0.1 (gfx950)"; }

int32_t achip_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* achip_last_error(void) { return g_lastError.c_str(); }

// ---- size helpers (the formulas: achip_bounds.h, which the bound kernel of achip_compress_bound_batch calls too) ----
int32_t achip_lz4_max_compressed_length(int32_t n) { return (int32_t)achip::bound::lz4(n); }
int32_t achip_snappy_max_compressed_length(int32_t n) { return (int32_t)achip::bound::snappy(n); }
int32_t achip_lzo_max_compressed_length(int32_t n) { return (int32_t)achip::bound::lzo(n); }
int32_t achip_lz4frame_max_compressed_length(int32_t n) { return int_bound(n, [&] { return achip::bound::lz4frame(n); }); }
// what the block-list writer asks (achip_ctx_set_lz4frame_writer): the worst-case places of the frame's blocks
int32_t achip_lz4frame_max_compressed_length_for(int32_t n, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize)
{
    if (n < 0) return bad_argument("uncompressedSize is negative");
    const achip::Lz4fRefusal r = achip::check_lz4f_writer(blockMaxSize, blockChecksum, contentChecksum, contentSize);
    if (r != achip::Lz4fRefusal::None) return bad_argument(achip::lz4f_refusal_text(r));
    return int_bound(n, [&] { return achip::bound::lz4frame_list(n, blockMaxSize, blockChecksum, contentChecksum, contentSize); });
}
// stream header + per 64 KiB block a chunk header, the masked CRC and at most the block itself (a compressed chunk is kept
// only at <= 0.85 of its block: M/snappy/SnappyFramedOutputStream.java:214)
int32_t achip_snappyframed_max_compressed_length(int32_t n) { return int_bound(n, [&] { return achip::bound::snappyframed(n); }); }
// the same for a writer built with another block size (achip_ctx_set_snappyframed_writer)
int32_t achip_snappyframed_max_compressed_length_for(int32_t n, int32_t blockSize)
{
    if (n < 0) return bad_argument("uncompressedSize is negative");
    if (blockSize <= 0 || blockSize > ACHIP_SNF_MAX_BLOCK_SIZE) return bad_argument("blockSize must be in (0, 65536]");
    return int_bound(n, [&] { return achip::bound::snappyframed(n, blockSize); });
}
int32_t achip_hadoop_max_compressed_length(int32_t codec, int32_t n, int32_t bufferSize)
{
    // per chunk of bufferSize - overhead plaintext bytes: two big-endian ints and at most the codec's maxCompressedLength
    // (M/lz4/Lz4HadoopOutputStream.java:44-46, 107-118, 128-131; M/snappy/SnappyHadoopOutputStream.java likewise)
    if (n < 0) return bad_argument("uncompressedSize is negative");
    if (codec != 0 && codec != 1) return bad_argument("codec must be 0 (LZ4) or 1 (Snappy)");
    const int64_t maxLength = achip::bound::hadoop(codec == 1, n, bufferSize);
    if (maxLength < 0) return bad_argument("bufferSize too small");
    return int_bound(n, [&] { return maxLength; });
}
// (bound::zstdstream with the Zstd bound as the int the host function returns)
int32_t achip_zstdstream_max_compressed_length(int32_t n) { return int_bound(n, [&] { return (int64_t)achip_zstd_max_compressed_length(n) + 16; }); }
int32_t achip_zstd_max_compressed_length(int32_t n)
{
    return (int32_t)achip::bound::zstd(n);
}

int64_t achip_snappy_uncompressed_length(const void* src, int64_t srcLen, int64_t* errOffset)
{
    // SnappyRawDecompressor.readUncompressedLength  M/snappy/SnappyRawDecompressor.java:277-321 (at most 5 bytes are looked at)
    int32_t expected = 0, nread = 0, eo = 0;
    const int32_t st = achip::snappy_read_uncompressed_length((const uint8_t*)src, (int32_t)(srcLen > 5 ? 5 : (srcLen < 0 ? 0 : srcLen)), expected, nread, eo);
    if (st != 0 && errOffset) *errOffset = srcLen < 0 ? srcLen : eo;
    return st != 0 ? st : expected;
}
// Magic and frame header (verifyMagic + readFrameHeader, M/zstd/ZstdFrameDecompressor.java:860-962) of the frame at in[0, srcLen): 0 with *h read, or the status
// the bytes are refused with and *off where.
static int64_t frame_header_at(const uint8_t* in, int64_t srcLen, achip::zframe::FrameHeader* h, int64_t* off)
{
    using achip::zframe::FrameHeader;
    auto fail = [&](int detail, int64_t at) -> int64_t {
        *off = at;
        return ACHIP_STATUS(ACHIP_CLASS_MALFORMED, detail);
    };
    if (srcLen < 4) return fail(ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, 0);
    if (const int32_t d = achip::zframe::magic_detail(in)) return fail(d, 0);
    *h = achip::zframe::read_frame_header(in + 4, srcLen - 4);
    if (h->state == FrameHeader::NEED_MORE) return fail(ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, 4 + h->offset);
    if (h->state == FrameHeader::FAILED) return fail(h->detail, 4 + h->offset);
    // the reference returns the raw long; a content size >= 2^63 would collide with this API's negative statuses, so it is
    // reported as what it is (no such frame can be decoded: the window check rejects it)
    if (h->contentBeyondInt64) return fail(ACHIP_D_ZSTD_WINDOW_TOO_LARGE, 4 + h->offset);
    return 0;
}

// An upper bound of what the frames in [src, src + srcLen) decode to -- what a one-shot decoder needs before it can read a stream
// whose frames carry NO content size (ZstdOutputStream writes such frames from 4 MiB on, M/zstd/ZstdOutputStream.java:193-221; the
// reference reads them through a growing window, M/zstd/ZstdIncrementalFrameDecompressor.java:99-234,305-352, never knowing the size).
// Walks the frame headers and the block headers (achip_zstd_frame.h): a raw or RLE block decodes to its size field, a compressed block
// to at most MAX_BLOCK_SIZE = 128 KiB (:278), a frame to at most its content size when it has one.  Host code, no device.
// Negative = status (the bytes do not parse as frames; *errOffset set).
int64_t achip_zstd_decompress_bound(const void* src, int64_t srcLen, int64_t* errOffset)
{
    const uint8_t* in = (const uint8_t*)src;
    auto fail = [&](int detail, int64_t off) -> int64_t {
        if (errOffset) *errOffset = off;
        return ACHIP_STATUS(ACHIP_CLASS_MALFORMED, detail);
    };
    if (errOffset) *errOffset = 0;
    if (srcLen < 0 || (srcLen > 0 && in == nullptr)) return bad_argument("src");
    int64_t input = 0, total = 0;
    while (input < srcLen) {
        achip::zframe::FrameHeader h;
        int64_t eo = 0;
        const int64_t st = frame_header_at(in + input, srcLen - input, &h, &eo);
        if (st < 0) {
            if (errOffset) *errOffset = input + eo;
            return st;
        }
        input += 4 + h.headerSize;
        int64_t blocks = 0;
        for (;;) {
            if (srcLen - input < 3) return fail(ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
            const achip::zframe::BlockHeader b = achip::zframe::read_block_header(in + input);
            input += 3;
            if (b.type == 3) return fail(ACHIP_D_ZSTD_INVALID_BLOCK_TYPE, input);
            if (b.stored > srcLen - input) return fail(ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
            input += b.stored;
            blocks += b.type == 2 ? achip::zframe::kMaxBlock : b.size;
            if (b.last) {
                break;
            }
        }
        if (h.hasChecksum) {
            if (srcLen - input < 4) return fail(ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
            input += 4;
        }
        total += h.contentSize >= 0 && h.contentSize < blocks ? h.contentSize : blocks;
    }
    return total;
}

// ZstdFrameDecompressor.getDecompressedSize: the frame's content size, -1 when it has none
int64_t achip_zstd_decompressed_size(const void* src, int64_t srcLen, int64_t* errOffset)
{
    achip::zframe::FrameHeader h;
    int64_t off = 0;
    const int64_t st = frame_header_at((const uint8_t*)src, srcLen, &h, &off);
    if (st < 0 && errOffset) *errOffset = off;
    return st < 0 ? st : h.contentSize;
}

// ---- context -----------------------------------------------------------
achip_ctx* achip_ctx_create(int32_t device)
{
    int n = achip_device_count();
    if (n <= 0 || device < 0 || device >= n) {
        g_lastError = n <= 0 ? "no HIP device" : "device ordinal out of range";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        g_lastError = "hipSetDevice failed";
        return nullptr;
    }
    achip_ctx* ctx = new achip_ctx();
    ctx->device = device;
    hipError_t e = ctx->stream.create();
    if (e != hipSuccess) {
        device_failure("hipStreamCreate", e);
        delete ctx;
        return nullptr;
    }
    return ctx;
}

void achip_ctx_destroy(achip_ctx* ctx) { delete ctx; }  // (~achip_ctx, achip_host.h)

int32_t achip_ctx_device(achip_ctx* ctx) { return ctx ? ctx->device : -1; }
void* achip_ctx_stream(achip_ctx* ctx) { return ctx ? (void*)ctx->stream.get() : nullptr; }

int32_t achip_ctx_synchronize(achip_ctx* ctx)
{
    if (!ctx) return bad_argument("ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    return 0;
}

int32_t achip_ctx_set_option(achip_ctx* ctx, const char* name, int64_t value)
{
    if (!ctx || !name) return bad_argument("ctx/name is null");
    achip::Settings next = *ctx;
    const char* refusal = nullptr;
    switch (achip::apply(next, name, value, &refusal)) {
        case achip::Applied::Unknown: return bad_argument("unknown option");
        case achip::Applied::BadValue: return bad_argument(refusal);
        case achip::Applied::Ok: break;
    }
    const std::string k(name);
    if (k == "host.copy_threads" && ctx->pool) return bad_argument("host.copy_threads must be set before the first host-pointer batch");
    static_cast<achip::Settings&>(*ctx) = next;
    if (k == "decompress.auto_remember") ctx->autoChoice[0] = ctx->autoChoice[1] = -1;
    return 0;
}

// Lz4Compressor.create(acceleration): the check and its text are Lz4NativeCompressor's (M/lz4/Lz4NativeCompressor.java:34-41)
int32_t achip_ctx_set_lz4_acceleration(achip_ctx* ctx, int32_t acceleration)
{
    if (acceleration < ACHIP_LZ4_DEFAULT_ACCELERATION || acceleration > ACHIP_LZ4_MAX_ACCELERATION) {
        const std::string text = "LZ4 acceleration should be in the [1, 65537] range but got " + std::to_string(acceleration);
        return bad_argument(text.c_str());
    }
    if (!ctx) return bad_argument("ctx is null");
    ctx->kernel.lz4Acceleration = acceleration;
    return 0;
}

int32_t achip_ctx_get_lz4_acceleration(achip_ctx* ctx)
{
    if (!ctx) return bad_argument("ctx is null");
    return ctx->kernel.lz4Acceleration;
}

// Frames of linked blocks (nothing in the reference: its reader refuses them, M/lz4/Lz4FrameCompression.java:213-216)
int32_t achip_ctx_set_lz4frame_linked_blocks(achip_ctx* ctx, int32_t accept)
{
    if (accept != 0 && accept != 1) return bad_argument("accept must be 0 or 1");
    if (!ctx) return bad_argument("ctx is null");
    achip::set_lz4f_linked_blocks(ctx->kernel, accept);
    return 0;
}

int32_t achip_ctx_get_lz4frame_linked_blocks(achip_ctx* ctx)
{
    if (!ctx) return bad_argument("ctx is null");
    return ctx->kernel.lz4fLinkedBlocks;
}

// The LZ4 frame writer's frame descriptor (nothing in the reference: its writer has one shape, M/lz4/Lz4FrameCompression.java:98-132): checked in the order of
// the arguments, before the context is looked at
int32_t achip_ctx_set_lz4frame_writer(achip_ctx* ctx, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize)
{
    const achip::Lz4fRefusal r = achip::check_lz4f_writer(blockMaxSize, blockChecksum, contentChecksum, contentSize);
    if (r != achip::Lz4fRefusal::None) return bad_argument(achip::lz4f_refusal_text(r));
    if (!ctx) return bad_argument("ctx is null");
    achip::set_lz4f_writer(ctx->kernel, blockMaxSize, blockChecksum, contentChecksum, contentSize);
    return 0;
}

int32_t achip_ctx_get_lz4frame_writer(achip_ctx* ctx, int32_t* blockMaxSize, int32_t* blockChecksum, int32_t* contentChecksum, int32_t* contentSize)
{
    if (!ctx) return bad_argument("ctx is null");
    if (blockMaxSize) *blockMaxSize = ctx->kernel.lz4fBlockMaxSize;
    if (blockChecksum) *blockChecksum = ctx->kernel.lz4fBlockChecksum;
    if (contentChecksum) *contentChecksum = ctx->kernel.lz4fContentChecksum;
    if (contentSize) *contentSize = ctx->kernel.lz4fContentSize;
    return 0;
}

// Double.toString(v), which the reference's "%1s" prints: the shortest digits -- two at least -- that read back as v (Double.MIN_VALUE is 4.9E-324), d.d in
// [1e-3, 1e7) and d.dE±n outside.  aircompressor_amd/native.py has the same function for the Python classes' own check (tests/test_snf_params_abi.py compares).
static std::string java_double_text(double v)
{
    if (v != v) return "NaN";
    if (v == 0) return std::signbit(v) ? "-0.0" : "0.0";
    if (std::isinf(v)) return v < 0 ? "-Infinity" : "Infinity";
    char digits[40];
    int precision = 2;
    for (; precision < 17; precision++) {
        snprintf(digits, sizeof(digits), "%.*e", precision - 1, v);
        if (strtod(digits, nullptr) == v) break;
    }
    snprintf(digits, sizeof(digits), "%.*e", precision - 1, v);  // [-]d[.ddd]e[+-]xx
    std::string mantissa(digits, strchr(digits, 'e'));
    const int exponent = atoi(strchr(digits, 'e') + 1);
    const std::string sign = mantissa[0] == '-' ? "-" : "";
    std::string d;
    for (char c : mantissa) {
        if (c >= '0' && c <= '9') d += c;
    }
    while (d.size() > 1 && d.back() == '0') d.pop_back();
    if (exponent >= -3 && exponent < 7) {
        std::string whole, frac;
        if (exponent < 0) {
            whole = "0";
            frac = std::string((size_t)(-exponent - 1), '0') + d;
        }
        else {
            if ((int)d.size() < exponent + 1) d.append((size_t)(exponent + 1) - d.size(), '0');
            whole = d.substr(0, (size_t)exponent + 1);
            frac = d.substr((size_t)exponent + 1);
        }
        return sign + whole + "." + (frac.empty() ? "0" : frac);
    }
    return sign + d.substr(0, 1) + "." + (d.size() > 1 ? d.substr(1) : "0") + "E" + std::to_string(exponent);
}

// SnappyFramedOutputStream(compressor, out, writeChecksums, blockSize, minCompressionRatio): the checks, their order and their texts are the constructor's
// (M/snappy/SnappyFramedOutputStream.java:83, :90); the ratio arrives as Double.doubleToRawLongBits of it
int32_t achip_ctx_set_snappyframed_writer(achip_ctx* ctx, int32_t writeChecksums, int32_t blockSize, int64_t minCompressionRatioBits)
{
    switch (achip::check_snf_writer(writeChecksums, blockSize, minCompressionRatioBits)) {
        case achip::SnfRefusal::Ratio: {
            const std::string text = "minCompressionRatio " + java_double_text(achip::snf_ratio(minCompressionRatioBits)) + " must be between (0,1.0].";
            return bad_argument(text.c_str());
        }
        case achip::SnfRefusal::BlockSize: return bad_argument("blockSize must be in (0, 65536]");
        case achip::SnfRefusal::Flag: return bad_argument("writeChecksums must be 0 or 1");
        case achip::SnfRefusal::None: break;
    }
    if (!ctx) return bad_argument("ctx is null");
    achip::set_snf_writer(ctx->kernel, writeChecksums, blockSize, minCompressionRatioBits);
    return 0;
}

int32_t achip_ctx_get_snappyframed_writer(achip_ctx* ctx, int32_t* writeChecksums, int32_t* blockSize, int64_t* minCompressionRatioBits)
{
    if (!ctx) return bad_argument("ctx is null");
    if (writeChecksums) *writeChecksums = ctx->kernel.snfWriteChecksums;
    if (blockSize) *blockSize = ctx->kernel.snfBlockSize;
    if (minCompressionRatioBits) *minCompressionRatioBits = ctx->kernel.snfMinRatioBits;
    return 0;
}

// SnappyFramedInputStream(decompressor, in, verifyChecksums)  M/snappy/SnappyFramedInputStream.java:74-79
int32_t achip_ctx_set_snappyframed_verify_checksums(achip_ctx* ctx, int32_t verify)
{
    if (verify != 0 && verify != 1) return bad_argument("verifyChecksums must be 0 or 1");
    if (!ctx) return bad_argument("ctx is null");
    achip::set_snf_verify(ctx->kernel, verify);
    return 0;
}

int32_t achip_ctx_get_snappyframed_verify_checksums(achip_ctx* ctx)
{
    if (!ctx) return bad_argument("ctx is null");
    return ctx->kernel.snfVerifyChecksums;
}

// n words at byte `offset` of the scratch, once everything the context has launched is done
static bool read_scratch(achip_ctx* ctx, int64_t offset, int32_t* v, int n)
{
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream.get()) != hipSuccess) return false;
    return hipMemcpy(v, (const uint8_t*)ctx->scratch.get() + offset, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
}

int64_t achip_ctx_get_stat(achip_ctx* ctx, const char* name)
{
    if (!ctx || !name) return -1;
    const std::string k(name);
    // what the context itself knows
    if (k == "pack.tile_bytes") return achip::PACK_TILE_BYTES;  // the unit of achip_pack_outputs' copy (a constant of the build)
    if (k == "host.gather_us") return ctx->hostGatherUs;          // the gather thread copying the caller's inputs into pinned slots
    if (k == "host.scatter_us") return ctx->hostScatterUs;        // the finalizer thread copying outputs to the caller's buffers
    if (k == "host.wait_slot_us") return ctx->hostWaitSlotUs;     // the gather thread waiting for a free slot (the pipeline behind it is the limit)
    if (k == "host.wait_download_us") return ctx->hostWaitDownloadUs;  // the finalizer waiting for a chunk's download (the device side / the gather is the limit)
    if (k == "host.chunks") return ctx->hostChunks;
    if (k == "host.total_us") return ctx->hostTotalUs;
    if (k == "decompress.scratch_bytes") {  // the context's decode scratch as granted (the two-pass decoders' record arena is what lies behind its fixed part): a smaller grant than a batch asked for shows here and in decompress.twopass_fallback_blocks
        return ctx->scratchBytes;
    }
    // what the last launch left at the head of the scratch (achip_stats.h: the names, the layouts and the rule; -1: that launch left no such statistic)
    const achip::stats::Located at = achip::stats::locate(ctx->last, name);
    if (at.words == 0) return at.value;
    int32_t v[achip::stats::PROBE_WORDS] = {};
    if (ctx->scratch.get() == nullptr || !read_scratch(ctx, at.byteOffset, v, at.words)) return -1;
    return at.pick ? achip::plan::auto_pick(v, at.pickBlocks, at.pickShortLimit) : v[at.word];
}

// ---- memory helpers ----------------------------------------------------
void* achip_device_alloc(achip_ctx* ctx, int64_t bytes)
{
    if (!ctx || bytes < 0) return nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)std::max<int64_t>(bytes, 1));
    if (e != hipSuccess) {
        device_failure("hipMalloc", e);
        return nullptr;
    }
    return p;
}

int32_t achip_device_free(achip_ctx* ctx, void* p)
{
    if (!ctx) return bad_argument("ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipFree(p));
    return 0;
}

void* achip_host_alloc_pinned(int64_t bytes)
{
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, (size_t)std::max<int64_t>(bytes, 1), hipHostMallocDefault);
    if (e != hipSuccess) {
        device_failure("hipHostMalloc", e);
        return nullptr;
    }
    return p;
}

int32_t achip_host_free_pinned(void* p)
{
    HIP_TRY(hipHostFree(p));
    return 0;
}

int32_t achip_memcpy_h2d(achip_ctx* ctx, void* dst, const void* src, int64_t bytes)
{
    if (!ctx) return bad_argument("ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream.get()));
    return 0;
}

int32_t achip_memcpy_d2h(achip_ctx* ctx, void* dst, const void* src, int64_t bytes)
{
    if (!ctx) return bad_argument("ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream.get()));
    return 0;
}

int32_t achip_memset_d(achip_ctx* ctx, void* dst, int32_t value, int64_t bytes)
{
    if (!ctx) return bad_argument("ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(dst, value, (size_t)bytes, ctx->stream.get()));
    return 0;
}

// ---- events ------------------------------------------------------------
void* achip_event_create(void)
{
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return (void*)ev;
}
int32_t achip_event_destroy(void* ev)
{
    HIP_TRY(hipEventDestroy((hipEvent_t)ev));
    return 0;
}
int32_t achip_event_record(achip_ctx* ctx, void* ev)
{
    if (!ctx) return bad_argument("ctx is null");
    HIP_TRY(hipEventRecord((hipEvent_t)ev, ctx->stream.get()));
    return 0;
}
float achip_event_elapsed_ms(void* evStart, void* evStop)
{
    if (hipEventSynchronize((hipEvent_t)evStop) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, (hipEvent_t)evStart, (hipEvent_t)evStop) != hipSuccess) return -1.0f;
    return ms;
}

}  // extern "C"
