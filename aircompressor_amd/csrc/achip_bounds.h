// achip_bounds.h -- what the nine compress ops ask of dstCap, stated once: the host functions achip_*_max_compressed_length (abi_context.cpp) and the bound
// kernel of achip_compress_bound_batch (pack_outputs.hip) call these, so the two cannot drift.  Every helper takes a length n >= 0 and computes in 64 bits:
// a result above INT32_MAX is the caller's to refuse (the host functions with their message, the kernel with a status).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace achip {
namespace bound {

// Lz4RawCompressor.maxCompressedLength  M/lz4/Lz4RawCompressor.java:56-59
__host__ __device__ inline int64_t lz4(int64_t n) { return n + n / 255 + 16; }
// LzoRawCompressor.maxCompressedLength  M/lzo/LzoRawCompressor.java:65-68
__host__ __device__ inline int64_t lzo(int64_t n) { return n + n / 255 + 16; }
// SnappyRawCompressor.maxCompressedLength  M/snappy/SnappyRawCompressor.java:47-70
__host__ __device__ inline int64_t snappy(int64_t n) { return 32 + n + n / 6; }
// ZstdFrameCompressor's compressBound as ZstdJavaCompressor.maxCompressedLength states it (the shifts are those of the Java ints: for 0 <= n <= INT32_MAX
// they are the plain ones; a negative n, which only the host function can be handed, wraps as it does there)
__host__ __device__ inline int64_t zstd(int32_t n)
{
    int64_t result = (int64_t)n + (int64_t)((uint32_t)n >> 8);
    if (n < 128 * 1024) {
        result += (int64_t)((uint32_t)(128 * 1024 - (int64_t)n) >> 11);
    }
    return result;
}
// the stream writer's frame around the same blocks: header without a content size, the last block's header, the checksum
__host__ __device__ inline int64_t zstdstream(int32_t n) { return zstd(n) + 16; }
// Lz4FrameCompression.maxCompressedLength  M/lz4/Lz4FrameCompression.java:70-83
__host__ __device__ inline int64_t lz4frame(int64_t n)
{
    const int64_t blocks = (n + (4 << 20) - 1) / (4 << 20);
    return 7 + 4 + n + 4 * blocks;
}
// What the block-list LZ4 frame writer (lz4_frame_writer.hip; achip_ctx_set_lz4frame_writer) asks: the worst-case places its blocks are encoded at inside the
// destination -- header (with the content size), per block of blockMaxSize bytes its size field, the block encoder's bound and the block checksum, the end mark,
// the content checksum.  The flags are 0 or 1.
__host__ __device__ inline int64_t lz4frame_list(int64_t n, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize)
{
    const int64_t each = 4 + 4 * (int64_t)blockChecksum;
    const int64_t rest = n % blockMaxSize;
    return 7 + 8 * (int64_t)contentSize + (n / blockMaxSize) * (each + lz4(blockMaxSize)) + (rest > 0 ? each + lz4(rest) : 0) + 4 + 4 * (int64_t)contentChecksum;
}
// stream header + per block of blockSize bytes (1 .. 65536: the writer's constructor argument, M/snappy/SnappyFramedOutputStream.java:77-91) a chunk header, the
// CRC field and at most the block itself (a compressed chunk is kept only at <= minCompressionRatio <= 1.0 of its block: :213)
__host__ __device__ inline int64_t snappyframed(int64_t n, int32_t blockSize)
{
    const int64_t blocks = (n + blockSize - 1) / blockSize;
    return 10 + 8 * blocks + n;
}
// the same at the default block size of 64 KiB
__host__ __device__ inline int64_t snappyframed(int64_t n) { return snappyframed(n, 65536); }
// per chunk of bufferSize - overhead plaintext bytes: two big-endian ints and at most the codec's maxCompressedLength (M/lz4/Lz4HadoopOutputStream.java:44-46,
// 107-118, 128-131; M/snappy/SnappyHadoopOutputStream.java likewise).  -1: the buffer leaves a chunk no room
__host__ __device__ inline int64_t hadoop(bool snappyCodec, int64_t n, int32_t bufferSize)
{
    const int64_t overhead = snappyCodec ? bufferSize / 6 + 32 : ((int32_t)(bufferSize * 0.01) > 10 ? (int32_t)(bufferSize * 0.01) : 10);
    const int64_t chunk = (int64_t)bufferSize - overhead;
    if (bufferSize <= 0 || chunk <= 0) {
        return -1;
    }
    const int64_t rest = n % chunk;
    const int64_t full = snappyCodec ? snappy(chunk) : lz4(chunk);
    const int64_t last = snappyCodec ? snappy(rest) : lz4(rest);
    return (n / chunk) * (8 + full) + (rest > 0 ? 8 + last : 0);
}

}  // namespace bound
}  // namespace achip
