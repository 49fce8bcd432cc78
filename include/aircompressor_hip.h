/*
 * aircompressor_hip.h -- C ABI of libaircompressor_hip.so
 *
 * The MI355X (gfx950) batched block-codec backend for airlift/aircompressor's
 * LZ4 / Snappy / Zstd block API.  Every entry point is `extern "C"`, takes plain
 * pointers and integer sizes, and depends on nothing but libamdhip64.  This is
 * the boundary a Java `java.lang.foreign` (FFM) binding attaches to, exactly the
 * way the reference binds liblz4/libsnappy/libzstd:
 *
 *   reference binding mechanism ....... M/internal/NativeLoader.java:66-117
 *   reference LZ4 symbol record ....... M/lz4/Lz4Native.java:30-40
 *   reference Snappy symbol record .... M/snappy/SnappyNative.java:63-75
 *   reference Zstd symbol record ...... M/zstd/ZstdNative.java:27-41
 *   (M/ = src/main/java/io/airlift/compress/v3/ of airlift/aircompressor)
 *
 * FFM type map (NativeLoader.java:138-153): int8/int32/int64/pointer only --
 * every signature below uses only those.
 *
 * Return convention: >= 0 is "bytes written" (or a size); < 0 is an ACHIP status
 * (see achip_status_class / achip_status_detail).  Batched calls never abort a
 * batch: they fill status[i] / errOffset[i] per block.
 */
#ifndef AIRCOMPRESSOR_HIP_H
#define AIRCOMPRESSOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Status codes                                                              */
/* ------------------------------------------------------------------------- */
/* status = -(class + 16 * detail); class in 1..15, detail in 0..(2^26)       */
#define ACHIP_OK 0
#define ACHIP_CLASS_MALFORMED 1        /* -> MalformedInputException(offset, reason)  M/MalformedInputException.java:16-36 */
#define ACHIP_CLASS_OUTPUT_TOO_SMALL 2 /* -> IllegalArgumentException (buffer sizing) e.g. M/lz4/Lz4RawCompressor.java:87-89 */
#define ACHIP_CLASS_INVALID_ARGUMENT 3 /* -> IllegalArgumentException (bad args)      */
#define ACHIP_CLASS_DEVICE 4           /* HIP runtime / device failure                */

#define ACHIP_STATUS(cls, detail) (-((cls) + 16 * (detail)))

/* detail ids: one per distinct message of the reference's Java codecs. */
enum achip_detail {
    ACHIP_D_GENERIC = 0,
    /* LZ4 decode -- M/lz4/Lz4RawDecompressor.java */
    ACHIP_D_LZ4_INPUT_EMPTY = 1,          /* :48-50  "input is empty"                                  */
    ACHIP_D_LZ4_MALFORMED = 2,            /* :66,76,125,138 "Malformed input"                          */
    ACHIP_D_LZ4_LAST_LITERAL_OUTSIDE = 3, /* :85   "attempt to write last literal outside of destination buffer" */
    ACHIP_D_LZ4_INPUT_NOT_CONSUMED = 4,   /* :89   "all input must be consumed"                        */
    ACHIP_D_LZ4_OFFSET_OUTSIDE = 5,       /* :118  "offset outside destination buffer"                 */
    ACHIP_D_LZ4_LAST_5_LITERALS = 6,      /* :170  "last 5 bytes must be literals"                     */
    ACHIP_D_LZ4_EMPTY_OUTPUT = 7,         /* :52-57 the reference *returns -1* here (no exception)     */
    /* LZ4 encode -- M/lz4/Lz4RawCompressor.java */
    ACHIP_D_LZ4_MAX_INPUT = 8,            /* :83-85 "Max input length exceeded"                        */
    ACHIP_D_LZ4_MAX_OUTPUT = 9,           /* :87-89 "Max output length must be larger than N"          */
    /* Snappy decode -- M/snappy/SnappyRawDecompressor.java */
    ACHIP_D_SNAPPY_MALFORMED = 16,        /* :92,108,119,128,155,160,164 "Malformed input"             */
    ACHIP_D_SNAPPY_TRUNCATED = 17,        /* :316-318 "Input is truncated"                             */
    ACHIP_D_SNAPPY_LEN_HIGH_BIT = 18,     /* :300   "last byte of compressed length int has high bit set" */
    ACHIP_D_SNAPPY_INVALID_LENGTH = 19,   /* :308   "invalid compressed length"                        */
    ACHIP_D_SNAPPY_LENGTH_MISMATCH = 20,  /* :61-65 "Recorded length is N bytes but actual length ..." */
    ACHIP_D_SNAPPY_OUTPUT_TOO_SMALL = 21, /* :49-50 "Uncompressed length N must be less than M"        */
    /* Snappy encode -- M/snappy/SnappyRawCompressor.java */
    ACHIP_D_SNAPPY_MAX_OUTPUT = 22,       /* :85-88 "Output buffer must be at least N bytes"           */
    /* Zstd decode -- M/zstd/ZstdFrameDecompressor.java and friends */
    ACHIP_D_ZSTD_NOT_ENOUGH_INPUT = 32,   /* "Not enough input bytes"                                  */
    ACHIP_D_ZSTD_OUTPUT_TOO_SMALL = 33,   /* "Output buffer too small" (verify => MalformedInputException) */
    ACHIP_D_ZSTD_CORRUPTED = 34,          /* "Input is corrupted"                                      */
    ACHIP_D_ZSTD_BAD_MAGIC = 35,          /* :949-959 "Invalid magic prefix: <hex>"                    */
    ACHIP_D_ZSTD_V07_MAGIC = 36,          /* :955   "Data encoded in unsupported ZSTD v0.7 format"     */
    ACHIP_D_ZSTD_BAD_CHECKSUM = 37,       /* :199-201 "Bad checksum. Expected: .., actual: .."         */
    ACHIP_D_ZSTD_DICTIONARY = 38,         /* :905   "Custom dictionaries not supported"                */
    ACHIP_D_ZSTD_INVALID_BLOCK_TYPE = 39, /* :186   "Invalid block type"                               */
    ACHIP_D_ZSTD_BLOCK_TOO_LARGE = 40,    /* :278   (blockSize > 128 KiB)                              */
    ACHIP_D_ZSTD_BLOCK_TOO_SMALL = 41,    /* :279   "Compressed block size too small"                  */
    ACHIP_D_ZSTD_WINDOW_TOO_LARGE = 42,   /* :303   "Window size too large (not yet supported)"        */
    ACHIP_D_ZSTD_DICT_CORRUPTED = 43,     /* :294   treeless literals without a table                  */
    ACHIP_D_ZSTD_LITERALS_TOO_LARGE = 44, /* :752,795 "Block exceeds maximum size"                     */
    ACHIP_D_ZSTD_FSE_TABLE_LOG = 45,      /* FseTableReader.java:46 "FSE table size exceeds maximum allowed size" */
    ACHIP_D_ZSTD_FSE_SYMBOL = 46,         /* FseTableReader.java:74,127 symbol too large               */
    ACHIP_D_ZSTD_TABLE_MISSING = 47,      /* :622,645,668 repeat mode without a previous table         */
    ACHIP_D_ZSTD_VALUE_TOO_LARGE = 48,    /* :616,639,662 "Value exceeds expected maximum value"       */
    ACHIP_D_ZSTD_BITSTREAM_EMPTY = 49,    /* BitInputStream.java:112 "Bitstream is empty"              */
    ACHIP_D_ZSTD_BITSTREAM_NO_MARK = 50,  /* BitInputStream.java:115 "Bitstream end mark not present"  */
    ACHIP_D_ZSTD_BITSTREAM_NOT_CONSUMED = 51, /* Huffman.java:316 "Bit stream is not fully consumed"   */
    ACHIP_D_ZSTD_SEQUENCES_NOT_CONSUMED = 52, /* :396 "Not all sequences were consumed"                */
    ACHIP_D_ZSTD_FSE_OUTPUT_SMALL = 53,   /* FiniteStateEntropy.java:114,131 "Output buffer is too small" */
    /* Zstd encode */
    ACHIP_D_ZSTD_MAX_OUTPUT = 60,         /* Util.checkArgument "Output buffer too small"              */
    /* LZ4 frame container -- M/lz4/Lz4FrameCompression.java */
    ACHIP_D_LZ4F_TOO_SHORT = 64,          /* :150   "Input is too short to be an LZ4 frame"                 */
    ACHIP_D_LZ4F_TRUNC_MAGIC = 65,        /* :158   "Truncated LZ4 frame: incomplete magic number"          */
    ACHIP_D_LZ4F_BAD_MAGIC = 66,          /* :170   "Invalid LZ4 frame magic number"                        */
    ACHIP_D_LZ4F_TRUNC_HEADER = 67,       /* :191,230 "Truncated LZ4 frame header"                          */
    ACHIP_D_LZ4F_VERSION_0 = 68,          /* :198   "Unsupported LZ4 frame version: 0" (2, 3 follow)        */
    ACHIP_D_LZ4F_VERSION_2 = 69,
    ACHIP_D_LZ4F_VERSION_3 = 70,
    ACHIP_D_LZ4F_RESERVED_BITS = 71,      /* :202   "Corrupt LZ4 frame: reserved bits in the frame descriptor must be zero" */
    ACHIP_D_LZ4F_LINKED_BLOCKS = 72,      /* :213   "LZ4 frames with linked blocks are not supported"       */
    ACHIP_D_LZ4F_DICTIONARY = 73,         /* :217   "LZ4 frames with a dictionary are not supported"        */
    ACHIP_D_LZ4F_BLOCK_MAX_SIZE = 74,     /* :222   "Invalid LZ4 frame block maximum size"                  */
    ACHIP_D_LZ4F_HEADER_CHECKSUM = 75,    /* :241   "Corrupt LZ4 frame: invalid header checksum"            */
    ACHIP_D_LZ4F_MISSING_BLOCK_SIZE = 76, /* :248   "Truncated LZ4 frame: missing block size"               */
    ACHIP_D_LZ4F_BLOCK_PAST_END = 77,     /* :260   "Truncated LZ4 frame: block extends past end of input"  */
    ACHIP_D_LZ4F_OUTPUT_TOO_SMALL = 78,   /* :265,276 "Output buffer too small" (a MalformedInputException here)  */
    ACHIP_D_LZ4F_BLOCK_EXCEEDS_MAX = 79,  /* :279   "Corrupt LZ4 frame: decompressed block exceeds maximum block size" */
    ACHIP_D_LZ4F_MISSING_BLOCK_CHECKSUM = 80, /* :288 "Truncated LZ4 frame: missing block checksum"         */
    ACHIP_D_LZ4F_BLOCK_CHECKSUM = 81,     /* :293   "Corrupt LZ4 frame: invalid block checksum"             */
    ACHIP_D_LZ4F_MISSING_CONTENT_CHECKSUM = 82, /* :307 "Truncated LZ4 frame: missing content checksum"     */
    ACHIP_D_LZ4F_CONTENT_CHECKSUM = 83,   /* :312   "Corrupt LZ4 frame: invalid content checksum"           */
    ACHIP_D_LZ4F_CONTENT_SIZE = 84,       /* :318   "Corrupt LZ4 frame: content size does not match frame header" */
    ACHIP_D_LZ4F_TRUNC_SKIP_SIZE = 85,    /* :334   "Truncated LZ4 skippable frame: missing frame size"     */
    ACHIP_D_LZ4F_TRUNC_SKIP = 86,         /* :340   "Truncated LZ4 skippable frame"                         */
    ACHIP_D_LZ4F_MAX_OUTPUT = 87,         /* :362   "Output buffer too small" (IllegalArgumentException, encoder) */
    /* x-snappy-framed streams (M/snappy/SnappyFramedInputStream.java; IOException / EOFException unless noted) */
    ACHIP_D_SNF_EOF_STREAM_HEADER = 88,   /* :68    "encountered EOF while reading stream header"           */
    ACHIP_D_SNF_BAD_STREAM_HEADER = 89,   /* :71    "invalid stream header"                                 */
    ACHIP_D_SNF_EOF_BLOCK_HEADER = 90,    /* :323   "encountered EOF while reading block header"            */
    ACHIP_D_SNF_EOF_FRAME = 91,           /* :177   "unexpectd EOF when reading frame" (sic)                */
    ACHIP_D_SNF_STREAM_ID_LENGTH = 92,    /* :255   "stream identifier chunk with invalid length: N"        */
    ACHIP_D_SNF_UNSKIPPABLE = 93,         /* :263   "unsupported unskippable chunk: XX"                     */
    ACHIP_D_SNF_INVALID_LENGTH = 94,      /* :273   "invalid length: N for chunk flag: XX"                  */
    ACHIP_D_SNF_CHECKSUM = 95,            /* :207   "Corrupt input: invalid checksum"                       */
    ACHIP_D_SNF_OUTPUT_TOO_SMALL = 96,    /* this API: the destination cannot hold the stream's plaintext   */
    ACHIP_D_SNF_MAX_OUTPUT = 97,          /* this API (encoder): dstCap < achip_snappyframed_max_compressed_length */
    /* Hadoop LZ4 / Snappy block streams (M/lz4/Lz4HadoopInputStream.java, M/snappy/SnappyHadoopInputStream.java; IOException / EOFException) */
    ACHIP_D_HDP_TRUNCATED_INT = 104,      /* Lz4HadoopInputStream.java:153 "Stream is truncated"                                     */
    ACHIP_D_HDP_EOF_BLOCK_DATA = 105,     /* :136   "encountered EOF while reading block data"                                        */
    ACHIP_D_HDP_CHUNK_EXCEEDS_BLOCK = 106, /* SnappyHadoopInputStream.java:117 "Chunk uncompressed size is greater than block size"   */
    ACHIP_D_HDP_LENGTH_MISMATCH = 107,    /* SnappyHadoopInputStream.java:137 "Expected to read N bytes, but data only contained M bytes" */
    ACHIP_D_HDP_NOT_CONSUMED = 108,       /* T/HadoopCodecDecompressor.java:52 "All input was not consumed": the destination cannot hold the stream */
    ACHIP_D_HDP_NEGATIVE_LENGTH = 109,    /* this API: a negative chunk length (Java: the block codec's range check throws)           */
    ACHIP_D_HDP_MAX_OUTPUT = 110,         /* this API (encoder): dstCap < achip_hadoop_max_compressed_length                          */
    /* LZO decode -- M/lzo/LzoRawDecompressor.java */
    ACHIP_D_LZO_MALFORMED = 111,          /* :57,112,133,169,210,236,252,262,298,324,329 "Malformed input": every throw of the decoder, "output too small"
                                             included.  (Its "Invalid LZO command" branch :245-248 cannot be reached: the four tests in front of it --
                                             (c & 0xF0) == 0, == 0x10, (c & 0xE0) == 0x20, (c & 0xC0) != 0 -- cover every byte.) */
    /* LZO encode -- M/lzo/LzoRawCompressor.java */
    ACHIP_D_LZO_MAX_INPUT = 112,          /* :84-86 "Max input length exceeded"                        */
    ACHIP_D_LZO_MAX_OUTPUT = 113,         /* :88-90 "Max output length must be larger than N" (checked before "nothing compresses to nothing": an empty input
                                             with dstCap < 16 is this, not 0) */
    /* runtime */
    ACHIP_D_NO_DEVICE = 100,
    ACHIP_D_HIP_ERROR = 101,
    ACHIP_D_BAD_ARGUMENT = 102,
    ACHIP_D_UNSUPPORTED = 103
};

int32_t achip_status_class(int32_t status);  /* 0 for status >= 0 */
int32_t achip_status_detail(int32_t status);
/* English reason string for a detail id, matching the reference's exception text
 * up to the ": offset=N" suffix that MalformedInputException appends itself. */
const char* achip_detail_message(int32_t detail);

/* ------------------------------------------------------------------------- */
/* Library / device                                                          */
/* ------------------------------------------------------------------------- */
const char* achip_version(void);
int32_t achip_device_count(void); /* 0 when no HIP device is usable; isEnabled() keys off this, cf. M/lz4/Lz4Native.java:75-85 */
const char* achip_last_error(void); /* thread-local text of the last ACHIP_CLASS_DEVICE failure */

/* ------------------------------------------------------------------------- */
/* Size helpers (host only, no device)                                        */
/* ------------------------------------------------------------------------- */
/* replaces Lz4RawCompressor.maxCompressedLength      M/lz4/Lz4RawCompressor.java:64-67 (bound as LZ4_compressBound in M/lz4/Lz4Native.java:31) */
int32_t achip_lz4_max_compressed_length(int32_t uncompressedSize);
/* replaces SnappyRawCompressor.maxCompressedLength   M/snappy/SnappyRawCompressor.java:47-70 (snappy_max_compressed_length, M/snappy/SnappyNative.java:68) */
int32_t achip_snappy_max_compressed_length(int32_t uncompressedSize);
/* replaces ZstdJavaCompressor.maxCompressedLength    M/zstd/ZstdJavaCompressor.java:31-40 (ZSTD_compressBound, M/zstd/ZstdNative.java:28) */
int32_t achip_zstd_max_compressed_length(int32_t uncompressedSize);
/* replaces LzoRawCompressor.maxCompressedLength      M/lzo/LzoRawCompressor.java:65-68: n + n / 255 + 16 */
int32_t achip_lzo_max_compressed_length(int32_t uncompressedSize);
/* replaces SnappyRawDecompressor.getUncompressedLength  M/snappy/SnappyRawDecompressor.java:30-33,277-321; negative = status, *errOffset set */
int64_t achip_snappy_uncompressed_length(const void* src, int64_t srcLen, int64_t* errOffset);
/* replaces ZstdFrameDecompressor.getDecompressedSize    M/zstd/ZstdFrameDecompressor.java:942-947; -1 = unknown, < -1 = status */
int64_t achip_zstd_decompressed_size(const void* src, int64_t srcLen, int64_t* errOffset);
/* what the reading side of the stream classes needs in one-shot form (M/zstd/ZstdInputStream.java:63-105 over
 * M/zstd/ZstdIncrementalFrameDecompressor.java:99-352 reads frames WITHOUT a content size -- ZstdOutputStream's from 4 MiB on -- through a
 * growing window): an upper bound of the decoded size of all frames in the buffer, from the frame and block headers alone (host code);
 * >= 0 bound, negative = status, *errOffset set */
int64_t achip_zstd_decompress_bound(const void* src, int64_t srcLen, int64_t* errOffset);

/* ------------------------------------------------------------------------- */
/* Context: one HIP stream + device scratch on one GPU.                       */
/* Not thread-safe (like one codec instance, M/lz4/Lz4JavaCompressor.java:27-29);*/
/* distinct contexts may be used concurrently from distinct threads.           */
/* ------------------------------------------------------------------------- */
typedef struct achip_ctx achip_ctx;

achip_ctx* achip_ctx_create(int32_t device);      /* NULL on failure; see achip_last_error */
void achip_ctx_destroy(achip_ctx* ctx);
int32_t achip_ctx_device(achip_ctx* ctx);
void* achip_ctx_stream(achip_ctx* ctx);           /* the hipStream_t the batched calls launch on */
int32_t achip_ctx_synchronize(achip_ctx* ctx);    /* hipStreamSynchronize */
/* tuning knobs (kernel variant selection) of this context -- a mixed batch's helper contexts take a copy of them; name/value pairs documented
 * in DESIGN.md. returns 0 or status */
int32_t achip_ctx_set_option(achip_ctx* ctx, const char* name, int64_t value);
/* replaces the argument of Lz4Compressor.create(int acceleration)  M/lz4/Lz4Compressor.java:33-41, Lz4NativeCompressor(int acceleration)
 * M/lz4/Lz4NativeCompressor.java:34-41 and Lz4FrameNativeCompressor(int acceleration)  M/lz4/Lz4FrameNativeCompressor.java:37-40 (the bounds:
 * M/lz4/Lz4Native.java:49-50).  A property of the context, as it is of the Java compressor object; a mixed batch's helper contexts take a copy of it.
 * The encoders follow the Java encoder, so the parameter is defined on its loop by liblz4's rule: M/lz4/Lz4RawCompressor.java:115 reads
 * `acceleration << SKIP_TRIGGER` -- the search advances by `acceleration` positions per probe from its second probe on; 1 is the
 * Java encoder, byte for byte.
 * It applies to every LZ4 block encode and every LZ4 frame encode the context launches: achip_lz4_compress_batch, achip_lz4_compress,
 * achip_lz4frame_compress_batch, achip_lz4frame_compress, and ACHIP_OP_LZ4_COMPRESS / ACHIP_OP_LZ4FRAME_COMPRESS inside achip_batch_host,
 * achip_mixed_batch, achip_mixed_batch_host and achip_multi_batch_host (each context its own value).
 * It does NOT change: the Hadoop LZ4 writer in its one-shot or its window form (Lz4HadoopStreams creates a default compressor:
 * M/lz4/Lz4HadoopStreams.java:52-66), any bound, any decoder, any other codec.
 * set: 0, or for a value outside [1, 65537] a status of class INVALID_ARGUMENT with detail ACHIP_D_BAD_ARGUMENT -- the context keeps its value,
 * achip_last_error has the reference's text "LZ4 acceleration should be in the [1, 65537] range but got N" (checked before the context is looked at).
 * get: the value, or a status for a null context. */
#define ACHIP_LZ4_DEFAULT_ACCELERATION 1
#define ACHIP_LZ4_MAX_ACCELERATION 65537
int32_t achip_ctx_set_lz4_acceleration(achip_ctx* ctx, int32_t acceleration);
int32_t achip_ctx_get_lz4_acceleration(achip_ctx* ctx);
/* replaces nothing in the reference: Lz4FrameCompression.decompressFrame refuses a frame whose block-independence bit is clear ("LZ4 frames with linked
 * blocks are not supported", M/lz4/Lz4FrameCompression.java:213-216) because it "cannot decode block by block".  This reader decodes a frame's blocks in
 * order into one contiguous output, so it can: with accept = 1 such frames -- what liblz4's frame API writes at its defaults (LZ4F_blockLinked), `lz4 -BD`,
 * python-lz4's lz4.frame.compress() -- are decoded.  A deliberate step beyond the Java reader, hence OFF by default; a property of the
 * context, as accepting them would be of a reader object; a mixed batch's helper contexts take a copy of it.
 * With accept = 1 a match of a linked frame's block may begin up to 65 535 bytes in front of the position being written, in the decoded content of the SAME
 * frame (stored blocks' bytes included; never a previous frame of the item, never anything in front of the item's dstOff).  The only check that changes is
 * the block decoder's ACHIP_D_LZ4_OFFSET_OUTSIDE (M/lz4/Lz4RawDecompressor.java:118): the offset is compared with the bytes of this frame produced so far
 * instead of the bytes of this block; status, detail and the block-relative errOffset of that failure are the block decoder's.  Every other check of
 * decompressFrame keeps its order, detail and offset; a frame with a dictionary ID is still ACHIP_D_LZ4F_DICTIONARY.
 * It applies to every LZ4 frame decode the context launches: achip_lz4frame_decompress_batch, achip_lz4frame_decompress, ACHIP_OP_LZ4FRAME_DECOMPRESS inside
 * achip_batch_host, achip_mixed_batch, achip_mixed_batch_host and achip_multi_batch_host, and that op's line of achip_decoded_size_batch (linked frames are
 * sized instead of reported).
 * It does NOT change: any encoder (no writer here writes linked blocks), any bound, any other reader, the Hadoop LZ4 streams (they have no frames), frames of
 * independent blocks (same bytes, same path), or anything at all with accept = 0: every byte, status, detail and offset is then what it was without this call.
 * set: 0, or for a value other than 0 or 1 a status of class INVALID_ARGUMENT with detail ACHIP_D_BAD_ARGUMENT -- the context keeps its value (checked
 * before the context is looked at).
 * get: 0 or 1, or a status for a null context. */
int32_t achip_ctx_set_lz4frame_linked_blocks(achip_ctx* ctx, int32_t accept);
int32_t achip_ctx_get_lz4frame_linked_blocks(achip_ctx* ctx);
/* replaces nothing in the reference: Lz4FrameCompression.compress writes one shape of frame -- FLG 0x60, BD 0x70: independent 4 MiB blocks, no checksum, no
 * content size (M/lz4/Lz4FrameCompression.java:98-132) -- while its reader, and this library's, accept the whole format.  With these values the writer writes the
 * rest: blockMaxSize is the frame's block-maximum size, one of 65536, 262144, 1048576, 4194304 (BD ids 4 .. 7); blockChecksum = 1 puts XXH32 (seed 0) of every
 * block's data as stored behind it, contentChecksum = 1 XXH32 of the frame's content behind the end mark, contentSize = 1 the 8-byte content size into the
 * header.  FLG = 0x60 | blockChecksum << 4 | contentSize << 3 | contentChecksum << 2; the blocks are independent, each the block encoder's bytes for that block
 * alone at the context's acceleration, stored raw (high bit of the size field) where that is not smaller (:114-126).  A deliberate step beyond the Java writer,
 * hence OFF unless asked for; properties of the context, as they would be of a writer object; a mixed batch's helper contexts take a copy.
 * The defaults are (4194304, 0, 0, 0).  At the defaults -- and context option "lz4frame.compress.variant" 0 -- every byte, bound, status and kernel is what it was
 * without these calls.  With any other value, or with that option at 1, every LZ4 frame encode of the context takes the block-list writer: a
 * frame's blocks are encoded side by side at worst-case places INSIDE the item's destination and then moved together, so that writer asks of dstCap
 *     7 + 8 contentSize + (n / B) (e + lz4(B)) + (n % B ? e + lz4(n % B) : 0) + 4 + 4 contentChecksum,   B = blockMaxSize, e = 4 + 4 blockChecksum,
 *     lz4(n) = n + n / 255 + 16
 * -- achip_lz4frame_max_compressed_length_for, and that op's line of achip_compress_bound_batch -- and refuses less with OUTPUT_TOO_SMALL /
 * ACHIP_D_LZ4F_MAX_OUTPUT before it writes one byte of the item's destination (the Java writer's rule, "fits if the output fits", is the default writer's
 * only).  A frame of more than 2^20 blocks is INVALID_ARGUMENT / ACHIP_D_UNSUPPORTED, a negative length INVALID_ARGUMENT / ACHIP_D_BAD_ARGUMENT.
 * They apply to every LZ4 frame encode the context launches: achip_lz4frame_compress_batch, achip_lz4frame_compress, and ACHIP_OP_LZ4FRAME_COMPRESS inside
 * achip_batch_host, achip_mixed_batch, achip_mixed_batch_host and achip_multi_batch_host (each context its own values).
 * They do NOT change: the LZ4 block encoder, the Hadoop LZ4 writer, any reader, any other codec, or achip_lz4frame_max_compressed_length (Java's formula).
 * set: 0, or a status of class INVALID_ARGUMENT with detail ACHIP_D_BAD_ARGUMENT -- the context keeps all of its values.  Checked in the order of the arguments,
 * before the context is looked at: "blockMaxSize must be 65536, 262144, 1048576 or 4194304", then "<flag> must be 0 or 1" for the three flags.
 * get: 0 with the values stored through the non-null pointers, or a status for a null context.
 * achip_lz4frame_max_compressed_length_for: the formula above in 64-bit arithmetic, for every parameter set, (4194304, 0, 0, 0) included; a negative status for
 * n < 0, for a value the setter refuses, or for a result above INT32_MAX. */
#define ACHIP_LZ4F_DEFAULT_BLOCK_MAX_SIZE 4194304
int32_t achip_ctx_set_lz4frame_writer(achip_ctx* ctx, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize);
int32_t achip_ctx_get_lz4frame_writer(achip_ctx* ctx, int32_t* blockMaxSize, int32_t* blockChecksum, int32_t* contentChecksum, int32_t* contentSize);
int32_t achip_lz4frame_max_compressed_length_for(int32_t uncompressedSize, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize);
/* replaces the arguments of SnappyFramedOutputStream(compressor, out, writeChecksums, blockSize, minCompressionRatio)
 * M/snappy/SnappyFramedOutputStream.java:77-91 (newChecksumFreeBenchmarkOutputStream :65-69 is writeChecksums = 0 at the defaults) and of
 * SnappyFramedInputStream(decompressor, in, verifyChecksums)  M/snappy/SnappyFramedInputStream.java:74-79.  Properties of the context, as they are of the
 * Java stream objects; a mixed batch's helper contexts take a copy of them.  Every type here is one NativeLoader.getMemoryLayout binds, so the ratio
 * crosses as its IEEE-754 bit pattern (Double.doubleToRawLongBits), never as a double.
 * The writer cuts its input into blocks of blockSize bytes (:116-141), keeps a chunk compressed where (double) compressed / (double) length <=
 * minCompressionRatio (:213, the same correctly rounded division on the device) and stores the block raw otherwise, and writes the masked CRC-32C of
 * the block's plaintext or, without checksums, 0 (:203 -- the CRC is then not computed at all).  The reader with verify = 0 does not look at the CRC
 * field and runs no CRC pass: ACHIP_D_SNF_CHECKSUM cannot arise; every structure error, its offset, the lengths and the window calls' stop reasons stay
 * as they are.  At the defaults every byte, status and offset is what it was before these calls existed.
 * The writer's values apply to every x-snappy-framed encode the context launches: achip_snappyframed_compress_batch, achip_snappyframed_compress,
 * ACHIP_OP_SNAPPYFRAMED_COMPRESS inside achip_batch_host, achip_mixed_batch, achip_mixed_batch_host and achip_multi_batch_host (each context its own
 * values), achip_window_compress_batch and achip_window_compress under that op (consumed, need and the worst-case room count in blocks of blockSize:
 * need = blockSize on a partial block, 8 + blockSize (+ 10) on want of room), and to that op's line of achip_compress_bound_batch -- the bound at the
 * context's block size, as the Hadoop ops use "hadoop.buffer_size"; the encoders' ACHIP_D_SNF_MAX_OUTPUT check asks for the same bound,
 * achip_snappyframed_max_compressed_length_for(n, blockSize).  verify applies to every x-snappy-framed decode: the one-shot calls, host and mixed
 * batches, achip_window_decompress_batch and achip_window_decompress.
 * They do NOT change: raw Snappy, the Hadoop Snappy streams, achip_decoded_size_batch (checksums are not its business), any other codec, or
 * achip_snappyframed_max_compressed_length (the bound at 65536).
 * set_writer: 0, or a status of class INVALID_ARGUMENT with detail ACHIP_D_BAD_ARGUMENT -- the context keeps all of its values.  Checked before the
 * context is looked at, in the constructor's order: the ratio must be > 0 and <= 1.0 (NaN is refused), achip_last_error "minCompressionRatio <value>
 * must be between (0,1.0]." (:83); then blockSize, "blockSize must be in (0, 65536]" (:90); then both flags must be 0 or 1.
 * get_writer: 0 with the values stored through the non-null pointers, or a status for a null context.  get_verify: 0 / 1, or a status.
 * achip_snappyframed_max_compressed_length_for: 10 + 8 * ceil(n / blockSize) + n in 64-bit arithmetic; a negative status for n < 0, a block size outside
 * (0, 65536] or a result above INT32_MAX (n = 2^30 at blockSize 1). */
#define ACHIP_SNF_DEFAULT_BLOCK_SIZE 65536
#define ACHIP_SNF_MAX_BLOCK_SIZE     65536
#define ACHIP_SNF_DEFAULT_MIN_RATIO_BITS 0x3FEB333333333333LL   /* 0.85 */
int32_t achip_ctx_set_snappyframed_writer(achip_ctx* ctx, int32_t writeChecksums, int32_t blockSize, int64_t minCompressionRatioBits);
int32_t achip_ctx_get_snappyframed_writer(achip_ctx* ctx, int32_t* writeChecksums, int32_t* blockSize, int64_t* minCompressionRatioBits);
int32_t achip_ctx_set_snappyframed_verify_checksums(achip_ctx* ctx, int32_t verify);
int32_t achip_ctx_get_snappyframed_verify_checksums(achip_ctx* ctx);
int32_t achip_snappyframed_max_compressed_length_for(int32_t uncompressedSize, int32_t blockSize);
/* diagnostics of the LAST batched call on this context (synchronizes the stream); -1 = unknown name / nothing recorded.
 * "zstd.decompress.fallback_items": items the five-stage pipeline handed to the one-kernel decoder;
 * "zstd.decompress.fallback_stage1" .. "stage6": the same, by the stage that handed them over (6: the multi-block stages' walk);
 * "zstd.decompress.multiblock_items" / "_blocks" / "_fast_items": items of the last Zstd decode that hold one frame of several blocks
 *   (ZstdOutputStream's output; ZstdFrameCompressor's and libzstd's beyond 128 KiB), their blocks, and how many of them the pipeline's
 *   multi-block stages finished (the rest went to the one-kernel decoder); option "zstd.decompress.stream_blocks" sizes those stages;
 * "zstd.decompress.long_items": items of the last Zstd decode's last tile that the pipeline's sequence stage counted as long-sequence
 *   items (capacity >= 80 bytes per sequence): a tile of more than 16 384 items with at least 24 576 of them runs those on the ring executor,
 *   everything else runs on the record executor (-1: the one-kernel decoder ran);
 * "lz4.decompress.mixed_groups": auto mode's count of mixed 16-block groups of the last LZ4 / Snappy decode (-1: no probe ran);
 * "lzo.decompress.fallback_blocks": items of the last LZO decode whose records did not fit the two passes' arena (or cannot be expressed as
 *   records): the wavefront-per-item decoder took them (0 when that decoder ran alone; -1: the last launch was no LZO decode);
 * "decompress.choice": the decoder auto mode ran (0 LDS rings, 3 two passes; -1: no probe ran).  DESIGN.md 8b lists every option and
 *   statistic. */
int64_t achip_ctx_get_stat(achip_ctx* ctx, const char* name);

/* device / pinned memory helpers; addresses are usable as MemorySegment.ofAddress */
void* achip_device_alloc(achip_ctx* ctx, int64_t bytes);
int32_t achip_device_free(achip_ctx* ctx, void* p);
void* achip_host_alloc_pinned(int64_t bytes);
int32_t achip_host_free_pinned(void* p);
int32_t achip_memcpy_h2d(achip_ctx* ctx, void* dst, const void* src, int64_t bytes); /* async on the ctx stream */
int32_t achip_memcpy_d2h(achip_ctx* ctx, void* dst, const void* src, int64_t bytes); /* async on the ctx stream */
int32_t achip_memset_d(achip_ctx* ctx, void* dst, int32_t value, int64_t bytes);     /* async on the ctx stream */

/* HIP events on the ctx stream, for timing from a host language */
void* achip_event_create(void);
int32_t achip_event_destroy(void* ev);
int32_t achip_event_record(achip_ctx* ctx, void* ev);
float achip_event_elapsed_ms(void* evStart, void* evStop); /* synchronizes on evStop; <0 on failure */

/* ------------------------------------------------------------------------- */
/* Batched, device-resident block API (the hot path).                         */
/*                                                                           */
/* Every pointer is a DEVICE-accessible address (device memory, or pinned     */
/* host memory).  Block i reads srcBase[srcOff[i] .. +srcLen[i]) and writes   */
/* dstBase[dstOff[i] .. +dstCap[i]); on return (after achip_ctx_synchronize)  */
/* outLen[i] = bytes written, status[i] = 0 or an ACHIP status,               */
/* errOffset[i] = the offset the reference's exception would carry.           */
/* The call itself is asynchronous on the ctx stream; its return value only   */
/* reports launch failures.  Regions of distinct blocks must not overlap --    */
/* the WHOLE capacity [dstOff[i], dstOff[i] + dstCap[i]) belongs to block i    */
/* for the call: as with the Java decoders' 8-byte copies, bytes between      */
/* outLen[i] and dstCap[i] may be written (their content is unspecified).     */
/* ------------------------------------------------------------------------- */
#define ACHIP_BATCH_ARGS                                                            \
    achip_ctx *ctx, const void *srcBase, const int64_t *srcOff, const int32_t *srcLen, \
        void *dstBase, const int64_t *dstOff, const int32_t *dstCap, int32_t *outLen, \
        int32_t *status, int64_t *errOffset, int32_t nBlocks

/* replaces Lz4RawDecompressor.decompress    M/lz4/Lz4RawDecompressor.java:35-198   (a1) */
int32_t achip_lz4_decompress_batch(ACHIP_BATCH_ARGS);
/* replaces Lz4RawCompressor.compress        M/lz4/Lz4RawCompressor.java:69-192     (a2) */
int32_t achip_lz4_compress_batch(ACHIP_BATCH_ARGS);
/* replaces SnappyRawDecompressor.decompress M/snappy/SnappyRawDecompressor.java:35-220 (a3) */
int32_t achip_snappy_decompress_batch(ACHIP_BATCH_ARGS);
/* replaces SnappyRawCompressor.compress     M/snappy/SnappyRawCompressor.java:74-233   (a4) */
int32_t achip_snappy_compress_batch(ACHIP_BATCH_ARGS);
/* replaces ZstdFrameDecompressor.decompress M/zstd/ZstdFrameDecompressor.java:135-210  (a5-a10); frames of several blocks -- what
 * ZstdOutputStream (M/zstd/ZstdOutputStream.java:154-221) writes -- take the same fast path (f3, decode half) */
int32_t achip_zstd_decompress_batch(ACHIP_BATCH_ARGS);
/* replaces ZstdFrameCompressor.compress(level 3) M/zstd/ZstdFrameCompressor.java:136-150 (a11-a14) */
int32_t achip_zstd_compress_batch(ACHIP_BATCH_ARGS);
/* replaces LzoRawDecompressor.decompress    M/lzo/LzoRawDecompressor.java:32-352: an item is any number of concatenated LZO1X blocks (decoded until the
 * input is consumed); an empty item is 0 bytes, status 0.  Every failure is MALFORMED / ACHIP_D_LZO_MALFORMED with the Java `input - inputAddress` in
 * errOffset -- a destination that is too small included.  Context option "lzo.decompress.variant"  */
int32_t achip_lzo_decompress_batch(ACHIP_BATCH_ARGS);
/* replaces LzoRawCompressor.compress        M/lzo/LzoRawCompressor.java:70-201: byte for byte; wants dstCap >= achip_lzo_max_compressed_length(srcLen) */
int32_t achip_lzo_compress_batch(ACHIP_BATCH_ARGS);

/* ------------------------------------------------------------------------- */
/* Single-block host-pointer API: what Compressor.compress(MemorySegment,     */
/* MemorySegment) / Decompressor.decompress(...) bind to (M/Compressor.java:  */
/* 20-35, M/Decompressor.java:23-30).  src/dst are HOST pointers; the call    */
/* stages through the context's pinned buffers, runs a 1-block batch and      */
/* synchronizes.  Argument order follows LZ4_compress_fast /                  */
/* LZ4_decompress_safe as bound in M/lz4/Lz4Native.java:33,37.                */
/* ------------------------------------------------------------------------- */
int32_t achip_lz4_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_lz4_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_snappy_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_snappy_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_zstd_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_zstd_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
/* LzoCompressor.compress / LzoDecompressor.decompress  M/lzo/LzoCompressor.java, M/lzo/LzoDecompressor.java */
int32_t achip_lzo_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_lzo_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);

/* ---- LZ4 frame container ----
 * Replace Lz4FrameCompression.maxCompressedLength / compress / decompress    M/lz4/Lz4FrameCompression.java:70-83, 96-140, 145-343
 * (the methods behind Lz4FrameJavaCompressor / Lz4FrameJavaDecompressor, M/lz4/Lz4FrameJavaCompressor.java:26-44) with the
 * HIP block codec underneath.  An item of the batch is a whole buffer: any number of concatenated and skippable frames on
 * decode, one frame (4 MiB independent blocks, no checksums; achip_ctx_set_lz4frame_writer: the rest of the format) on encode.  Same batch arguments, result convention and
 * asynchrony as the block codecs; errOffset carries the MalformedInputException offset. */
int32_t achip_lz4frame_max_compressed_length(int32_t uncompressedSize);  /* negative: IllegalArgumentException */
int32_t achip_lz4frame_decompress_batch(ACHIP_BATCH_ARGS);
int32_t achip_lz4frame_compress_batch(ACHIP_BATCH_ARGS);
/* one HOST buffer, staged through the context's pinned buffer (Lz4FrameJava{De,}Compressor.{de,}compress(byte[]...)) */
int32_t achip_lz4frame_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_lz4frame_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);

/* ---- x-snappy-framed streams ----
 * Replace SnappyFramedOutputStream used as "write everything, close"   M/snappy/SnappyFramedOutputStream.java:73-96, 113-145, 200-255
 *     and SnappyFramedInputStream read to the end of the stream       M/snappy/SnappyFramedInputStream.java:52-73, 135-305
 * (64 KiB blocks, masked CRC-32C of every block's plaintext  M/snappy/Crc32C.java:29-50, a block stored raw when it does not
 * reach 0.85) with the HIP block codec underneath.  An item of the batch is a whole stream.  Same batch arguments, result
 * convention and asynchrony as the block codecs.  The stream-level IOExceptions (details ACHIP_D_SNF_*) report the position of
 * the offending chunk header in errOffset; a block codec error keeps its own detail and offset. */
int32_t achip_snappyframed_max_compressed_length(int32_t uncompressedSize);  /* bound this API asks of dstCap; negative: IllegalArgumentException */
int32_t achip_snappyframed_decompress_batch(ACHIP_BATCH_ARGS);
int32_t achip_snappyframed_compress_batch(ACHIP_BATCH_ARGS);
/* one HOST buffer, staged through the context's pinned buffer */
int32_t achip_snappyframed_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_snappyframed_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);

/* ---- Hadoop LZ4 / Snappy block streams (second half) ----
 * Replace Lz4HadoopOutputStream / SnappyHadoopOutputStream used as "write everything, close"   M/lz4/Lz4HadoopOutputStream.java:60-118,
 *     M/snappy/SnappyHadoopOutputStream.java:60-131   (as T/HadoopCodecCompressor.java:57-72 drives them)
 * and Lz4HadoopInputStream / SnappyHadoopInputStream read to the end   M/lz4/Lz4HadoopInputStream.java:47-156,
 *     M/snappy/SnappyHadoopInputStream.java:44-170   (as T/HadoopCodecDecompressor.java:40-60 drives them: a destination that cannot hold
 *     the stream is ACHIP_D_HDP_NOT_CONSUMED)
 * -- the streams behind org.apache.hadoop.io.compress.Lz4Codec / SnappyCodec (M/lz4/Lz4HadoopStreams.java:52-66) -- with the HIP block
 * codecs underneath.  [BE int plaintext length][BE int compressed length][block] ...; an item of the batch is a whole stream.  The
 * streams' buffer size (256 KiB unless configured, M/lz4/Lz4HadoopStreams.java:30) is the context option "hadoop.buffer_size".  Same
 * batch arguments, result convention and asynchrony as the block codecs; stream-level IOExceptions (details ACHIP_D_HDP_*) report the
 * position where the failing read began, a block codec error keeps its own detail and offset. */
int32_t achip_hadoop_max_compressed_length(int32_t codec /* 0 LZ4, 1 Snappy */, int32_t uncompressedSize, int32_t bufferSize);  /* bound this API asks of dstCap */
int32_t achip_lz4hadoop_decompress_batch(ACHIP_BATCH_ARGS);
int32_t achip_lz4hadoop_compress_batch(ACHIP_BATCH_ARGS);
int32_t achip_snappyhadoop_decompress_batch(ACHIP_BATCH_ARGS);
int32_t achip_snappyhadoop_compress_batch(ACHIP_BATCH_ARGS);
/* one HOST buffer, staged through the context's pinned buffer */
int32_t achip_lz4hadoop_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_lz4hadoop_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_snappyhadoop_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);
int32_t achip_snappyhadoop_decompress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);

/* ---- Zstd streams ----
 * READING needs no entry point of its own: what ZstdInputStream (M/zstd/ZstdInputStream.java:26-151, through
 * ZstdIncrementalFrameDecompressor.java:44-72,216-234) yields for a stream is what ZstdFrameDecompressor yields for its bytes, and
 * achip_zstd_decompress* take frames of any number of blocks on their fast path (DESIGN 6 "Multi-block frames").
 * WRITING: item i = everything a caller hands to ONE ZstdOutputStream (M/zstd/ZstdOutputStream.java:30-221) -- write(buffer, 0, n) and
 * close(), the way the reference's stream harness drives it (T/HadoopCodecCompressor.java:57-72); dst receives what the stream puts on
 * its sink.  That is NOT achip_zstd_compress' output: the stream's parameters are those for an unknown input size (window 2^20, hash
 * 2^17, chain 2^16 whatever n is; :48-58).  Below 4 MiB close() writes the input as one chunk whose size the frame header announces; from
 * 4 MiB on the stream flushes chunks before close() (header without content size, 23 blocks, then 15 per further 1920 KiB, the window slid
 * in between -- and, as in the reference, 7 blocks after every slide without a match: DESIGN 10 row 3).  n >= 2^30 is INVALID_ARGUMENT /
 * ACHIP_D_UNSUPPORTED (the Java code overflows there); option "zstd.stream.chunked" = 0 refuses everything from 4 MiB on the same way.
 * Byte-identical output wants dstCap >= achip_zstdstream_max_compressed_length(n) (the stream itself never runs out of room). */
int32_t achip_zstdstream_max_compressed_length(int32_t uncompressedSize);
int32_t achip_zstdstream_compress_batch(ACHIP_BATCH_ARGS);
int32_t achip_zstdstream_compress(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset);

/* ---- xxhash: batched XXH64 / XXH32 of device-resident buffers ----
 * Replace XxHash64Hasher.hash(MemorySegment input, long seed)   M/xxhash/XxHash64Hasher.java:78-86  (-> XxHash64JavaHasher.java:126)
 *     and XxHash32Hasher.hash(MemorySegment input, int seed)    M/xxhash/XxHash32Hasher.java       (-> XxHash32JavaHasher.java:112)
 * for nBuffers buffers per call: buffer i = srcBase + srcOff[i], srcLen[i] bytes; outHash[i] receives the hash
 * (all arrays device memory; asynchronous on the context's stream).  Returns 0 or a negative status. */
int32_t achip_xxhash64_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t seed, int64_t* outHash, int32_t nBuffers);
int32_t achip_xxhash32_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t seed, int32_t* outHash, int32_t nBuffers);
/* one HOST buffer (staged through the context's pinned buffer; synchronous): the one-shot form of the same two methods */
int32_t achip_xxhash64(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, int64_t* outHash);
int32_t achip_xxhash32(achip_ctx* ctx, const void* src, int64_t srcLen, int32_t seed, int32_t* outHash);
/* ---- XXH3 (xxhash3.hip): the reference's XxHash3Native.hash(MemorySegment, long seed) and hash128(MemorySegment, long seed) ----
 * Same conventions as achip_xxhash64[_batch]: device arrays and asynchronous on the context's stream for the batches (nBuffers == 0: no
 * launch; a negative length hashes as empty), one staged HOST buffer for the single calls.  The 128-bit hash comes back through the pointer:
 * outHash[2i] = low 64 bits, outHash[2i + 1] = high 64 bits (a single call fills outHash[0], outHash[1]). */
int32_t achip_xxhash3_64_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t seed, int64_t* outHash, int32_t nBuffers);
int32_t achip_xxhash3_128_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t seed, int64_t* outHash, int32_t nBuffers);
int32_t achip_xxhash3_64(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, int64_t* outHash);
int32_t achip_xxhash3_128(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, int64_t* outHash);

/* ---- streaming hashers (xxhash_stream.hip): the update / digest form of the four hashers ----
 * Replace the streaming half of the reference's hasher objects, for MANY streams per call:
 *   XxHash64Hasher.create(seed) / update / updateLE / digest / reset / close   M/xxhash/XxHash64Hasher.java:91-169
 *   the same interface of XxHash32Hasher.java, XxHash3Hasher.java and XxHash3Hasher128.java
 *   XxHash3Native.newHasher / newHasher128 (:77-105), Hasher64Impl (:220-344) and its 128-bit twin.
 * A hasher is a fixed-size record in device memory whose layout is private; `algo` is one of ACHIP_HASH_*.  State i of a batch lies at
 * states + i * achip_hash_state_size(algo).  A state carries its seed (XXH3: the secret derived from it), so one array may hold states
 * reset with different seeds (reset sub-ranges through pointer arithmetic) and update / digest take none. */
#define ACHIP_HASH_XXH32 0
#define ACHIP_HASH_XXH64 1
#define ACHIP_HASH_XXH3_64 2  /* 2 and 3 share the record and the update; only the digest differs */
#define ACHIP_HASH_XXH3_128 3
/* bytes of one state: a multiple of 16, below 1024; an unknown algo gives the (negative) INVALID_ARGUMENT status */
int64_t achip_hash_state_size(int32_t algo);
/* The batch calls: all arrays device-accessible, asynchronous on the context's stream, nStates == 0 launches nothing and returns 0.
 * reset  (create(seed) / reset(seed), XxHash64Hasher.java:91-101,150-160): every state becomes a fresh hasher with `seed` (XXH32: its low 32 bits).
 * update (update(MemorySegment), :103-140): state i absorbs srcBase[srcOff[i] .. + srcLen[i]); srcLen[i] <= 0 leaves it untouched.  Two
 *        items of one call must not name the same state (there is no state index: item i IS state i); overlapping state arrays in one call are
 *        the caller's error and the result is undefined.
 * digest (digest(), :142-148): outHash[i] = the hash of everything state i absorbed since its last reset (XXH32: zero-extended;
 *        XXH3-128: outHash[2i] = low, outHash[2i + 1] = high, as achip_xxhash3_128_batch).  Reads the states, never writes them. */
int32_t achip_hash_states_reset(achip_ctx* ctx, int32_t algo, void* states, int32_t nStates, int64_t seed);
int32_t achip_hash_states_update(achip_ctx* ctx, int32_t algo, void* states, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t nStates);
int32_t achip_hash_states_digest(achip_ctx* ctx, int32_t algo, const void* states, int64_t* outHash, int32_t nStates);
/* One stream fed from HOST memory -- the literal twin of a reference hasher object (XxHash3Native.java:220-344): one state of its own on the
 * device, the bytes staged through the context's pinned buffer in chunks, so srcLen may exceed INT32_MAX.
 * create  NULL on failure (achip_last_error); asynchronous.
 * update  BLOCKS until the bytes are absorbed (src may be reused on return); srcLen == 0 does nothing.
 * digest  BLOCKS; out[0] = the hash (XXH32 zero-extended), out[1] = the high half of XXH3-128 (0 otherwise); the state is unchanged.
 * reset   asynchronous.   destroy  (close(), :162-169) BLOCKS until the context's stream is idle, then frees the state. */
void* achip_hasher_create(achip_ctx* ctx, int32_t algo, int64_t seed);
int32_t achip_hasher_update(void* hasher, const void* src, int64_t srcLen);
int32_t achip_hasher_digest(void* hasher, int64_t* out);
int32_t achip_hasher_reset(void* hasher, int64_t seed);
int32_t achip_hasher_destroy(void* hasher);

/* Host-pointer batch: nBlocks independent blocks described by HOST arrays of HOST
 * pointers' offsets relative to srcBase/dstBase (host).  Stages in, launches the
 * device batch for `codecOp`, stages out, synchronizes.  codecOp: see below. */
#define ACHIP_OP_LZ4_DECOMPRESS 0
#define ACHIP_OP_LZ4_COMPRESS 1
#define ACHIP_OP_SNAPPY_DECOMPRESS 2
#define ACHIP_OP_SNAPPY_COMPRESS 3
#define ACHIP_OP_ZSTD_DECOMPRESS 4
#define ACHIP_OP_ZSTD_COMPRESS 5
#define ACHIP_OP_LZ4FRAME_DECOMPRESS 6
#define ACHIP_OP_LZ4FRAME_COMPRESS 7
#define ACHIP_OP_SNAPPYFRAMED_DECOMPRESS 8
#define ACHIP_OP_SNAPPYFRAMED_COMPRESS 9
#define ACHIP_OP_LZ4HADOOP_DECOMPRESS 10
#define ACHIP_OP_LZ4HADOOP_COMPRESS 11
#define ACHIP_OP_SNAPPYHADOOP_DECOMPRESS 12
#define ACHIP_OP_SNAPPYHADOOP_COMPRESS 13
#define ACHIP_OP_ZSTDSTREAM_COMPRESS 14
/* (15 is no op, and every entry point refuses it: even ops decode, odd ops encode, and 14 had taken the Zstd stream writer's place out of turn) */
#define ACHIP_OP_LZO_DECOMPRESS 16
#define ACHIP_OP_LZO_COMPRESS 17
int32_t achip_batch_host(int32_t codecOp, ACHIP_BATCH_ARGS);
/* (Staging is chunked and pipelined over up to four pinned slots: this thread gathers chunk c+1 into pinned memory while chunk c
 * is uploaded / run / downloaded on three streams and a finalizer thread scatters chunk c-1 to dstBase -- each side with a few
 * copy threads of its own; one upload and one download per chunk.  A single chunk (e.g. a single block) runs in order on the
 * context stream.  Options "host.chunk_bytes", "host.copy_threads".  Replaces N calls of Compressor.compress(byte[]...) /
 * Decompressor.decompress(byte[]...), M/Compressor.java:20-35, M/Decompressor.java:23-30, over one device.) */

/* Mixed batches (BASELINE configs[4]): item i is processed by codecOp[i] (ACHIP_OP_*), any interleaving.  The items are
 * bucketed by codec op so that every kernel launch is homogeneous -- what a caller holding e.g. one ORC / Parquet stripe with
 * LZ4, Snappy and Zstd pages would otherwise do by hand with one Decompressor per codec (M/Decompressor.java:23-30) -- and the
 * results land in the caller's item order.
 *   achip_mixed_batch:      codecOp is a HOST array (the caller's own knowledge of its items); every other array and both buffers are
 *                           DEVICE-accessible as for the homogeneous batch calls; asynchronous on the ctx stream (the buckets of the
 *                           Snappy and Zstd families run on streams of the library's own, side by side with LZ4's, ordered by events behind
 *                           whatever the ctx stream held and in front of whatever is enqueued on it next: option "mixed.concurrent").
 *   achip_mixed_batch_host: everything is HOST memory; staged like achip_batch_host; synchronous. */
int32_t achip_mixed_batch(achip_ctx* ctx, const int32_t* codecOp, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                          const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks);
int32_t achip_mixed_batch_host(achip_ctx* ctx, const int32_t* codecOp, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                               const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks);

/* ---- Sizing a batch on the device: for a caller that holds compressed items in device memory and knows nothing else ----
 * achip_decoded_size_batch: outSize[i] = the bytes item i decodes to under `codecOp`, one of the eight decode ops (LZ4, SNAPPY, ZSTD, LZ4FRAME, SNAPPYFRAMED,
 *   LZ4HADOOP, SNAPPYHADOOP, LZO _DECOMPRESS; any other op is INVALID_ARGUMENT), found without decoding: what a Java caller asks
 *     SnappyJavaDecompressor.getUncompressedLength   M/snappy/SnappyJavaDecompressor.java (-> SnappyRawDecompressor.java:30-33,277-321)      Snappy: the preamble
 *     ZstdJavaDecompressor.getDecompressedSize       M/zstd/ZstdJavaDecompressor.java   (-> ZstdFrameDecompressor.java:942-947)              Zstd: here the walk of
 *         the frames' blocks (block headers, literals headers, the match lengths of the sequence sections): frames without a content size are sized too, and the
 *         header's field, which the decoder never checks, is not trusted
 *   for, one buffer at a time on the host; for LZ4 raw blocks there is no counterpart: the Java caller must know (here: the token walk of
 *   M/lz4/Lz4RawDecompressor.java:59-195).  Containers: the reader's loop over the stream's headers, the LZ4 walk / the Snappy preamble per chunk where the
 *   loop needs it (an LZ4 frame that announces its content size is that size).  LZO blocks carry no length: the command walk of
 *   M/lzo/LzoRawDecompressor.java:52-349 with a capacity of INT32_MAX (status and offset are the decoder's for that capacity).
 *   R1  if the op's decoder, given dstCap = the item's true plaintext length, succeeds, then status[i] == 0 and outSize[i] is that length;
 *   R2  if status[i] == 0, the decoder run with dstCap = outSize[i] returns exactly outSize[i] or fails -- it never succeeds with another length.
 *   status[i] != 0 (errOffset[i] set, outSize[i] = 0): the walk met a structural fault, reported as the op's reader reports it.  Faults only the payload decode
 *   sees (checksums, Huffman literals, a block the walk does not enter) leave status 0.  (An LZ4 block that ends in a match decodes with room to spare and
 *   fails with exact room, Lz4RawDecompressor.java:168-171: it is sized with status 0.)
 * achip_plan_outputs: the decoders' dstOff[] / dstCap[] from the sizes: dstCap[i] = outSize[i], dstOff[i] = the running sum of the capacities in front of i, each
 *   rounded up to `align` (a power of two in 1 .. 4096; else INVALID_ARGUMENT).  An item with status[i] != 0 or outSize[i] > INT32_MAX is left out: dstCap[i] = 0,
 *   it takes no room, dstOff[i] is the running offset.  total[0] = the bytes the output buffer must have, total[1] = the items left out.
 * All arrays device-accessible; both calls asynchronous on the ctx stream (scratch from the context); nBlocks == 0 launches nothing; the return value reports
 * launch and argument failures only.  size -> plan -> a 16-byte readback of total -> allocate -> decode: one synchronisation, no host walk. */
int32_t achip_decoded_size_batch(achip_ctx* ctx, int32_t codecOp, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen,
                                 int64_t* outSize, int32_t* status, int64_t* errOffset, int32_t nBlocks);
int32_t achip_plan_outputs(achip_ctx* ctx, const int64_t* outSize, const int32_t* status, int32_t nBlocks, int32_t align,
                           int64_t* dstOff, int32_t* dstCap, int64_t* total /* [2] */);

/* ---- The compress side of the same: bound -> plan -> compress -> pack, for a caller whose plaintexts and their lengths live in device memory ----
 * achip_compress_bound_batch: outSize[i] = what `codecOp`, one of the nine compress ops (LZ4, SNAPPY, ZSTD, LZ4FRAME, SNAPPYFRAMED, LZ4HADOOP, SNAPPYHADOOP,
 *   ZSTDSTREAM, LZO _COMPRESS; any other op is INVALID_ARGUMENT), asks of dstCap for srcLen[i] bytes: the op's achip_*_max_compressed_length(srcLen[i]), computed in
 *   64-bit arithmetic -- what a Java caller asks Compressor.maxCompressedLength (M/Compressor.java:20) for, one int at a time on the host.  The Hadoop ops use
 *   the context's "hadoop.buffer_size", as their compress call does.  A negative srcLen[i], or a bound above INT32_MAX, gives status[i] of class
 *   INVALID_ARGUMENT and outSize[i] = 0; else status[i] = 0.  outSize / status feed achip_plan_outputs unchanged: its dstOff[] / dstCap[] / total are the
 *   compress call's slots.
 * achip_pack_outputs: the compress call's sparse result (srcBase / srcOff / outLen / status = its dstBase / dstOff / outLen / status: outLen[i] bytes at the
 *   front of a worst-case slot each) as one dense stream -- the chunk loops of the writers (M/lz4/Lz4HadoopOutputStream.java:107-117,
 *   M/snappy/SnappyFramedOutputStream.java:199-220: compress a chunk, append exactly what it took -- the latter also keeps the chunk itself where
 *   compression did not pay) over a whole batch.
 *   Item i is packed when status[i] == 0 and outLen[i] >= 0; any other item is left out: packedLen[i] = 0, it takes no room, packedOff[i] is the running offset.
 *   Raw arrays given (all three, and `stored`; else all four NULL): a packed item with outLen[i] >= rawLen[i] is taken from rawBase[rawOff[i] .. + rawLen[i])
 *   instead and stored[i] = 1 (an ORC writer's isOriginal chunk: keep the smaller); every other item has stored[i] = 0.
 *   packedLen[i] = the bytes taken; packedOff[i] = the sum of the lengths in front of i, each rounded up to `align` (a power of two in 1 .. 4096; else
 *   INVALID_ARGUMENT).  total[0] = the bytes of the dense stream (the sum of the rounded lengths), total[1] = the items left out.
 *   packedBase == NULL: plan only (offsets, lengths, total[0..1]; total[2] = 0).  Else the bytes are copied if and only if total[0] <= packedCap -- decided on
 *   the device, no host wait -- and total[2] = 1; if they do not fit, total[2] = 0 and not one byte of packedBase is written.  When copied, every byte of
 *   [0, total[0]) is defined: the items at their offsets, zeros behind each up to `align`; bytes at and beyond total[0] are never written (no slack rule:
 *   the compaction exists to give exact extents).  packedBase[0, packedCap) must not overlap any source region.
 * Conventions as for the sizing calls above: all arrays device-accessible, asynchronous on the ctx stream, scratch from the context, nBlocks == 0 launches
 * nothing and returns 0, value arguments are checked before the context is touched, the return value reports launch and argument failures only.
 * bound -> plan -> readback of the total -> allocate the slots -> compress -> pack (plan only) -> readback of total[0] -> allocate exactly that -> pack:
 * two synchronisations, no host walk. */
int32_t achip_compress_bound_batch(achip_ctx* ctx, int32_t codecOp, const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t nBlocks);
int32_t achip_pack_outputs(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* outLen, const int32_t* status,
                           const void* rawBase, const int64_t* rawOff, const int32_t* rawLen, /* all three NULL, or all three set */
                           int32_t nBlocks, int32_t align, void* packedBase, int64_t packedCap,
                           int64_t* packedOff, int32_t* packedLen, int32_t* stored /* NULL iff raw is NULL */, int64_t* total /* [3] */);

/* One process, several devices: the batch is cut into nCtx contiguous slices balanced by srcLen[i] + dstCap[i] (the rule of
 * achip_partition_blocks) and slice d runs through achip_batch_host (codecOps == NULL: every item is `codecOp`) or
 * achip_mixed_batch_host (codecOps[i] per item) on ctxs[d], each slice in a host thread of its own, all inside this call -- what
 * a JVM (one process) does with the GPUs of a node; java/.../HipBatchCodec.run is the same split with Java threads.  ctxs: nCtx
 * distinct contexts (normally one per device; several on one device are legal).  sliceStarts (may be NULL) receives the nCtx + 1
 * slice boundaries.  Units are self-contained (each frame decode resets its state, M/zstd/ZstdFrameDecompressor.java:151; each
 * compress() builds a fresh context, M/zstd/ZstdFrameCompressor.java:162; LZ4 / Snappy blocks likewise): the slices
 * exchange nothing.  Returns 0, or the first failing slice's negative status (achip_last_error names the slice). */
int32_t achip_multi_batch_host(achip_ctx* const* ctxs, int32_t nCtx, int32_t codecOp, const int32_t* codecOps, const void* srcBase, const int64_t* srcOff,
                               const int32_t* srcLen, void* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status,
                               int64_t* errOffset, int32_t nBlocks, int32_t* sliceStarts);

/* One long Zstd stream in bounded memory: what ZstdInputStream does over ZstdIncrementalFrameDecompressor
 * (M/zstd/ZstdInputStream.java:63-105, M/zstd/ZstdIncrementalFrameDecompressor.java:44-72,216-234).  Input arrives in pieces, output
 * leaves in pieces, a frame may be any length (ZstdOutputStream writes ONE frame per stream), frames may follow each other.
 *   begin   a stream state on ctx (NULL: achip_last_error); per state ~45 MB of host + device memory at an 8 MiB window, whatever
 *           the stream's length
 *   feed    takes up to srcLen bytes of src (*consumed; it holds back at most one step of blocks), writes up to dstCap bytes to dst
 *           (*produced).  Returns 0, or a negative status once the stream is known to be damaged AND every byte in front of the damage
 *           has been delivered -- the call that would deliver the first byte of a damaged block fails, where ZstdInputStream.read
 *           throws (*errOffset: stream offset of the block).  *consumed < srcLen with *produced == dstCap: output room needed;
 *           *consumed == srcLen and *produced < dstCap: input needed (or the stream's end: at_stopping_point)
 *   at_stopping_point   1 when a frame has been read to its end, its bytes are delivered and the next frame's magic is not complete
 *           (ZstdIncrementalFrameDecompressor.isAtStoppingPoint: state READ_FRAME_MAGIC -- up to three bytes behind the last frame are
 *           ignored, as ZstdInputStream.java:81-86 ignores them; before the first frame the Java state is INITIAL and this returns 0):
 *           where a stream may end; the end of input anywhere else is "Not enough input bytes" (ZstdInputStream.java:86).
 *           (RAW / RLE blocks that say more than 128 KiB -- the format forbids them, the Java reader copies / fills what they say,
 *           ZstdIncrementalFrameDecompressor.java:204-226 -- are decoded as several blocks of at most 128 KiB.)
 *   end     releases the state
 * All host pointers; synchronous; a state serves one thread at a time like its context. */
void* achip_zstdstream_decompress_begin(achip_ctx* ctx);
int32_t achip_zstdstream_decompress_feed(achip_ctx* ctx, void* state, const void* src, int64_t srcLen, void* dst, int64_t dstCap, int64_t* consumed, int64_t* produced,
                                         int64_t* errOffset);
int32_t achip_zstdstream_decompress_at_stopping_point(void* state);
int32_t achip_zstdstream_decompress_end(achip_ctx* ctx, void* state);

/* ... and the writer: ZstdOutputStream (M/zstd/ZstdOutputStream.java:93-221) a chunk at a time, in the 4 MiB the Java stream buffers -- write()
 * appends to the stream's buffer (on the device), a full buffer is flushed as whole blocks (compressIfNecessary :122-131, writeChunk :154-221: the
 * window slides), close() writes the rest and the checksum.  The bytes are the Java stream's whatever the sizes of the calls.
 *   begin    a stream state on ctx (NULL: achip_last_error)
 *   feed     write(src, 0, srcLen): takes input until dst is full of flushed blocks (*consumed, *produced); 0 or a negative status
 *   finish   close(): 1 when the stream's last byte has been delivered, 0 when dst was too small for the rest (call again)
 *   end      releases the state */
void* achip_zstdstream_compress_begin(achip_ctx* ctx);
int32_t achip_zstdstream_compress_feed(achip_ctx* ctx, void* state, const void* src, int64_t srcLen, void* dst, int64_t dstCap, int64_t* consumed, int64_t* produced);
int32_t achip_zstdstream_compress_finish(achip_ctx* ctx, void* state, void* dst, int64_t dstCap, int64_t* produced);
int32_t achip_zstdstream_compress_end(achip_ctx* ctx, void* state);

/* ---- Windows over the chunked containers (SURVEY L4 streams): x-snappy-framed, Hadoop LZ4 and Hadoop Snappy streams of any length in bounded memory ----
 * What SnappyFramedInputStream / SnappyFramedOutputStream, Lz4HadoopInputStream / Lz4HadoopOutputStream and SnappyHadoopInputStream /
 * SnappyHadoopOutputStream (and the HadoopStreams factories that hand them out) do a read() / write() at a time.  These formats' chunks are independent, so the
 * incremental form needs no state: the CALLER keeps the stream position, the library keeps nothing between calls, and many streams' windows run side by side in
 * one call, chunk-parallel on the device.
 * A WINDOW is a piece of one stream that begins at a unit boundary.  A UNIT is what the format's reader reads as one step -- x-snappy-framed: one chunk of any
 * type (the 10-byte stream identifier and skippable chunks included); Hadoop: one zero length word, or one block: [BE plaintext length] and every
 * [BE compressed length][codec block] chunk the reader reads for it.  A unit is WHOLE when all the bytes its reader would read for it are in the window.
 * codecOp: ACHIP_OP_SNAPPYFRAMED_ / LZ4HADOOP_ / SNAPPYHADOOP_ DECOMPRESS for the decompress calls, the three _COMPRESS ops for the compress calls; anything else is
 * INVALID_ARGUMENT, decided before the context is touched.  Batch calls: every array (flags too) device-accessible, asynchronous on the ctx stream, scratch from the
 * context, nBlocks == 0 launches nothing; the Hadoop ops use the context's "hadoop.buffer_size".
 * DECODE, window W with room dstCap: the call takes k leading whole units.  consumed = their bytes; outLen and the destination are what the op's one-shot reader
 * yields for those bytes with the same dstCap (a window without FIRST: for those bytes behind a stream identifier).  If the first unit is whole, fits and decodes,
 * k >= 1; units of the writer's shape (Hadoop: one chunk per block that produces the declared length; x-snappy-framed: any well-formed chunk) are ALL taken in one
 * call as far as they are whole, fit and decode -- listed by a walk, decoded side by side, the prefix found by a fold; units of any other shape are taken by a
 * wavefront per window, at least one per call.  stop says why the call took no more:
 *   END         consumed == srcLen.
 *   NEED_INPUT  the next unit is not whole and LAST is not set -- whatever the partial bytes look like.  need = the window bytes that unit wants, counted from its
 *               start, as far as its headers tell; 0 if they do not.  (A Hadoop end-of-stream marker -- a length word of -1; for LZ4 any negative chunk length --
 *               leaves its unit not whole: the one-shot reader reads once more behind the end it announces, so its verdict waits for LAST.)
 *   NEED_ROOM   the next unit is whole and its declared plaintext (the Hadoop block length, the Snappy preamble of a compressed chunk, length - 4 of a raw chunk)
 *               exceeds dstCap - outLen: need = that length.  Takes the place of ACHIP_D_SNF_OUTPUT_TOO_SMALL / ACHIP_D_HDP_NOT_CONSUMED, which stay what they are in
 *               the one-shot calls.  need == 0: the call's chunk list (2^20 entries for all its windows together) was full -- call again with what is left.
 *   FAILED      status != 0: status, its detail and errOffset - consumed are what the one-shot reader reports for W[consumed:] with room dstCap - outLen; under LAST an
 *               incomplete tail is among them (the one-shot reader's truncation errors).  Everything in front of the damage has been delivered: consumed and outLen
 *               describe it (the feed contract of achip_zstdstream_decompress_feed).  x-snappy-framed checksums are verified as in the one-shot reader.
 * ENCODE: consumed = the largest multiple of the writer's block size (x-snappy-framed: the context's blockSize, 64 KiB unless set; Hadoop: bufferSize minus the codec's overhead, as the one-shot
 * writer cuts) that the window holds and whose worst-case output fits dstCap; with LAST the partial tail block too.  The bytes written are the one-shot writer's for
 * W[:consumed] -- the x-snappy-framed stream identifier only under FIRST, which a caller sets until the stream's first byte is out -- so the windows' outputs, one
 * behind the other, are the one-shot writer's stream however the stream was cut.  NEED_INPUT: a partial block is left (need = the block size); NEED_ROOM: a block is
 * left for want of room (need = its worst case: the codec's bound and the two Hadoop length words, or the chunk's 8 bytes of header and CRC and the block; plus the
 * stream identifier's 10 bytes where not even they fit); need == 0: the window has taken its share of the call's block list (2^20 entries for all its windows together:
 * 2^20 / nBlocks blocks a window, at least one -- reached with small x-snappy-framed blocks, e.g. one window of more than 1 MiB at blockSize 1) -- call again with what
 * is left.  FAILED only for argument faults (a negative length: INVALID_ARGUMENT; more than 2^20 windows in one call: INVALID_ARGUMENT / ACHIP_D_UNSUPPORTED). */
#define ACHIP_WINDOW_FIRST 1   /* the window starts the stream (x-snappy-framed: the stream identifier is required / written) */
#define ACHIP_WINDOW_LAST  2   /* the stream ends with this window */
#define ACHIP_STOP_END        0  /* the whole window was taken */
#define ACHIP_STOP_NEED_INPUT 1  /* the next unit is not whole (decode) / a partial block is left (encode) */
#define ACHIP_STOP_NEED_ROOM  2  /* the next unit is whole but does not fit what dst has left */
#define ACHIP_STOP_FAILED     3  /* status != 0 */
int32_t achip_window_decompress_batch(achip_ctx* ctx, int32_t codecOp, const int32_t* flags, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                                      const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks,
                                      int64_t* consumed, int32_t* stop, int64_t* need);
int32_t achip_window_compress_batch(achip_ctx* ctx, int32_t codecOp, const int32_t* flags, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                                    const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks,
                                    int64_t* consumed, int32_t* stop, int64_t* need);
/* one HOST window, staged through the context's pinned buffer, synchronous; returns the window's status (0, or negative with *stop == ACHIP_STOP_FAILED) or a launch /
 * argument failure; every out pointer is required */
int32_t achip_window_decompress(achip_ctx* ctx, int32_t codecOp, int32_t flags, const void* src, int32_t srcLen, void* dst, int32_t dstCap,
                                int64_t* consumed, int64_t* produced, int32_t* stop, int64_t* need, int64_t* errOffset);
int32_t achip_window_compress(achip_ctx* ctx, int32_t codecOp, int32_t flags, const void* src, int32_t srcLen, void* dst, int32_t dstCap,
                              int64_t* consumed, int64_t* produced, int32_t* stop, int64_t* need, int64_t* errOffset);

/* Balanced contiguous partition of a batch over nParts GPUs: fills
 * starts[0..nParts] with block indices so that each part's sum of weight[i] is
 * as equal as a contiguous split allows.  Pure host arithmetic. */
int32_t achip_partition_blocks(const int64_t* weight, int32_t nBlocks, int32_t nParts, int32_t* starts);

#ifdef __cplusplus
}
#endif
#endif /* AIRCOMPRESSOR_HIP_H */
