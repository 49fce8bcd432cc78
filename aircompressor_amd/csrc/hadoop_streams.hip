// hadoop_streams.hip -- batched Hadoop LZ4 / Snappy block streams for gfx950 (second half).
//
// The format: a sequence of [BE int plaintext bytes of the block][BE int compressed bytes][codec block] ... where a "block" may come
// as several [compressed bytes][codec block] chunks (the reference's writer always emits one).  Replaces, over the HIP block codecs,
//   the writers   M/lz4/Lz4HadoopOutputStream.java:60-118, M/snappy/SnappyHadoopOutputStream.java:60-131 used as "write everything, close"
//                 (T/HadoopCodecCompressor.java:57-72): chunks of bufferSize - overhead plaintext bytes, overhead = max((int)(size * 0.01), 10)
//                 for LZ4 and size / 6 + 32 for Snappy; bufferSize 256 KiB unless configured (context option hadoop.buffer_size);
//   the readers   M/lz4/Lz4HadoopInputStream.java:47-156, M/snappy/SnappyHadoopInputStream.java:44-170 read to the end the way the
//                 reference's test harness does (T/HadoopCodecDecompressor.java:40-60): read(output, done, capacity - done) until -1 or
//                 full, then one read() -- a byte there is "All input was not consumed" (ACHIP_D_HDP_NOT_CONSUMED).
// An item of the batch is a whole stream.
//
// Reader, the fast way (chunk-parallel, as for x-snappy-framed streams in snappy_frame.hip):
//   walk    a LANE per stream runs over the length fields only.  It accepts the shape every writer produces -- each block one chunk, the
//           chunk producing exactly the block's declared length (Snappy announces it in its preamble; for LZ4 it is assumed and checked
//           afterwards), every block fitting what the destination has left (so the Java reader decodes straight into the caller's buffer,
//           with the remaining capacity) -- and appends one descriptor per chunk to a batch that exists on the device only;
//   decode  that batch runs through the batched LZ4 / Snappy block decoders, chosen on the device as for any batch;
//   fold    a lane per stream: all chunks decoded to the declared lengths -> done; anything else -> the serial kernel.
// Reader, the general way (and the fallback): a WAVEFRONT per stream runs the Java loops themselves -- same checks in the same order,
// the stream's own buffer included (LZ4: bufferSize + 8 bytes; Snappy: grown to the largest chunk + 8), because its capacity decides
// what the block decoder says about a malformed chunk -- with the 64-lane ring block decoders inside each step.
//
// Writer: a chunk's position depends on the sizes before it, but every chunk except a stream's last is full and none is larger than
// the codec's bound, so chunk k is compressed at its WORST-CASE position k * (8 + maxCompressedLength(chunk)) by persistent wavefronts
// drawing chunks from one list; a wavefront per stream then writes the length fields and moves the chunks left into place, in order.
//
// What the one-shot form adds: the offset of the stream-level IOExceptions (the position where the failing read began); for the
// Snappy reader a negative chunk length other than -1 is ACHIP_D_HDP_NEGATIVE_LENGTH (Java goes on with whatever its buffer holds from the
// chunk before: an exception whose kind depends on stale state; the LZ4 reader takes any negative length for the end of the stream, as
// Java does); a Snappy chunk that ends inside its length
// preamble is ACHIP_D_SNAPPY_TRUNCATED (Java reads stale buffer bytes); a Snappy chunk that announces more than the destination has
// left AND more than the wavefront's buffer holds (max(bufferSize, 256 KiB) + 8) is not decoded to look for errors in it
// (ACHIP_D_HDP_NOT_CONSUMED, what Java reports for a well-formed one).
#include "lz4_decode_body.h"
#include "snappy_decode_body.h"
#include "lz4_compress_mw.h"
#include "snappy_compress_mw.h"
#include "achip_launch.h"
#include "achip_lists.h"
#include "achip_window.h"

namespace achip {

namespace hdp {
constexpr int IN_RING = 2048, OUT_RING = 4096;
constexpr int32_t STREAM_EOF = -1000000;  // internal: end of stream
using lists::CAPACITY;

__host__ __device__ __forceinline__ int32_t input_max_size(bool snappy, int32_t bufferSize)
{
    const int32_t lz4Overhead = (int32_t)(bufferSize * 0.01) > 10 ? (int32_t)(bufferSize * 0.01) : 10;
    return bufferSize - (snappy ? bufferSize / 6 + 32 : lz4Overhead);
}
__host__ __device__ __forceinline__ int64_t block_bound(bool snappy, int64_t n)
{
    return snappy ? 32 + n + n / 6 : n + n / 255 + 16;  // M/snappy/SnappyRawCompressor.java:69 ; M/lz4/Lz4RawCompressor.java:64-67
}

__device__ __forceinline__ int32_t rd_be(const uint8_t* p)
{
    return (int32_t)(((uint32_t)p[0] << 24) + ((uint32_t)p[1] << 16) + ((uint32_t)p[2] << 8) + (uint32_t)p[3]);
}
__device__ __forceinline__ void wr_be(uint8_t* p, int32_t v)
{
    p[0] = (uint8_t)((uint32_t)v >> 24);
    p[1] = (uint8_t)((uint32_t)v >> 16);
    p[2] = (uint8_t)((uint32_t)v >> 8);
    p[3] = (uint8_t)v;
}

// ---------------------------------------------------------------------------------------------------------------------
// the general reader: one wavefront per stream (everything wave-uniform)
struct Reader {
    const uint8_t* in;
    int32_t n, pos;
    int32_t blockLen, chunkOff, chunkLen;  // uncompressedBlockLength, uncompressedChunkOffset / Length
    uint8_t* internal;                     // the stream's own buffer (`uncompressedChunk`)
    int32_t internalLen;                   // its Java length
    int32_t internalMax;                   // what this wavefront can hold
    const uint8_t* chunk;                  // `compressed`
    int64_t eo;
    uint8_t* lds;
    int lane;
    bool snappy;
};

// readBigEndianInt :142-156
__device__ __forceinline__ int32_t read_be(Reader& r, int32_t& v)
{
    if (r.pos >= r.n) {
        return STREAM_EOF;
    }
    if (r.n - r.pos < 4) {
        r.eo = r.pos;
        return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_TRUNCATED_INT);
    }
    v = rd_be(r.in + r.pos);
    r.pos += 4;
    return v == -1 ? STREAM_EOF : 0;
}

// the common head of bufferCompressedData (Lz4HadoopInputStream.java:100-127) and readNextChunk (SnappyHadoopInputStream.java:91-113);
// returns the chunk's compressed length, STREAM_EOF or a status
__device__ __forceinline__ int32_t next_chunk(Reader& r)
{
    r.blockLen -= r.chunkOff;
    r.chunkOff = 0;
    r.chunkLen = 0;
    while (r.blockLen == 0) {
        int32_t v = 0;
        const int32_t e = read_be(r, v);
        if (e == STREAM_EOF) {
            r.blockLen = 0;
            return STREAM_EOF;
        }
        if (e < 0) {
            return e;
        }
        r.blockLen = v;
    }
    int32_t clen = 0;
    const int32_t e = read_be(r, clen);
    if (e != 0) {
        return e;
    }
    if (clen < 0) {
        if (!r.snappy) {  // Lz4HadoopInputStream.java:51-54,65-68: `compressedChunkLength < 0` -- any negative value ends the stream for this read
            return STREAM_EOF;
        }
        r.eo = r.pos - 4;
        return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_NEGATIVE_LENGTH);
    }
    if (clen > r.n - r.pos) {  // readInput :129-140
        r.eo = r.pos;
        return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_EOF_BLOCK_DATA);
    }
    r.chunk = r.in + r.pos;
    r.pos += clen;
    return clen;
}

// the LZ4 block decoder as Lz4JavaDecompressor.decompress(byte[], ...) : returns the length or a status (eo = the codec's offset)
__device__ __forceinline__ int32_t lz4_decode(Reader& r, const uint8_t* src, int32_t len, uint8_t* dst, int32_t cap)
{
    using FR = Rings<64, IN_RING, OUT_RING, 1>;
    FR R;
    R.init(r.lds, r.lds + IN_RING, src, len, dst, r.lane);
    int32_t bst = 0, beo = 0, bop = 0;
    wave_mem_order();
    lz4_block_decode<64, IN_RING, OUT_RING, 1>(R, src, len, cap, bst, beo, bop);
    wave_mem_order();
    if (bst != 0) {
        r.eo = beo;
        return bst;
    }
    return bop;
}
__device__ __forceinline__ int32_t snappy_decode(Reader& r, const uint8_t* src, int32_t len, uint8_t* dst, int32_t cap)
{
    int32_t bst = 0, beo = 0, bop = 0;
    wave_mem_order();
    snappy_buffer_decode<64, IN_RING, OUT_RING, 1>(r.lds, r.lds + IN_RING, nullptr, src, len, dst, cap, r.lane, bst, beo, bop);
    wave_mem_order();
    if (bst != 0) {
        r.eo = beo;
        return bst;
    }
    return bop;
}

// Lz4HadoopInputStream.read(byte[], int, int) :61-82 ; single = read() :47-58 (returns 0 for "a byte")
__device__ int32_t lz4_read(Reader& r, uint8_t* dst, int32_t length, bool single)
{
    while (r.chunkOff >= r.chunkLen) {
        const int32_t clen = next_chunk(r);
        if (clen < 0) {
            return clen;
        }
        if (!single && length >= r.blockLen) {  // favor writing directly to the user buffer
            const int32_t w = lz4_decode(r, r.chunk, clen, dst, length);
            if (w < 0) {
                return w;
            }
            r.chunkLen = w;
            r.chunkOff = w;
            return w;
        }
        const int32_t w = lz4_decode(r, r.chunk, clen, r.internal, r.internalLen);
        if (w < 0) {
            return w;
        }
        r.chunkLen = w;
    }
    if (single) {
        r.chunkOff++;
        return 0;
    }
    const int32_t size = length < r.chunkLen - r.chunkOff ? length : r.chunkLen - r.chunkOff;
    wave_mem_order();
    group_copy<64>(dst, r.internal + r.chunkOff, size, r.lane);
    wave_mem_order();
    r.chunkOff += size;
    return size;
}

// SnappyHadoopInputStream.read(byte[], int, int) :57-73 over readNextChunk :91-141 ; single = read() :44-54
__device__ int32_t snappy_read(Reader& r, uint8_t* dst, int32_t length, bool single)
{
    if (r.chunkOff >= r.chunkLen) {
        bool direct = false;
        const int32_t clen = next_chunk(r);
        if (clen != STREAM_EOF) {
            if (clen < 0) {
                return clen;
            }
            int32_t beo = 0;
            const int32_t announced = snappy_announced(r.chunk, clen, beo);
            if (announced < 0) {
                r.eo = beo;
                return announced;
            }
            r.chunkLen = announced;
            if (r.chunkLen > r.blockLen) {
                r.eo = r.pos - clen;
                return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_CHUNK_EXCEEDS_BLOCK);
            }
            direct = !single;
            uint8_t* target = single ? r.internal : dst;
            int32_t cap = single ? r.internalLen : length;
            if (r.chunkLen > cap) {
                if (r.internalLen < r.chunkLen) {
                    if (r.chunkLen > r.internalMax - 8) {  // (beyond this wavefront's buffer: see the file header)
                        r.eo = r.pos;
                        return mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_HDP_NOT_CONSUMED);
                    }
                    r.internalLen = r.chunkLen + 8;
                }
                direct = false;
                target = r.internal;
                cap = r.internalLen;
            }
            const int32_t w = snappy_decode(r, r.chunk, clen, target, cap);
            if (w < 0) {
                return w;
            }
            if (w != r.chunkLen) {
                r.eo = r.pos - clen;
                return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_LENGTH_MISMATCH);
            }
        }
        if (r.chunkLen == 0) {
            return STREAM_EOF;
        }
        if (direct) {
            r.chunkOff += r.chunkLen;
            return r.chunkLen;
        }
    }
    if (single) {
        r.chunkOff++;
        return 0;
    }
    const int32_t size = length < r.chunkLen - r.chunkOff ? length : r.chunkLen - r.chunkOff;
    wave_mem_order();
    group_copy<64>(dst, r.internal + r.chunkOff, size, r.lane);
    wave_mem_order();
    r.chunkOff += size;
    return size;
}

// T/HadoopCodecDecompressor.java:40-60
template <bool SNAPPY>
__device__ int32_t decompress_item(const uint8_t* in, int32_t inLen, uint8_t* out, int32_t outCap, uint8_t* internal, int32_t internalMax, int32_t bufferSize, uint8_t* lds, int lane,
                                   int32_t& doneOut, int64_t& eo)
{
    Reader r;
    r.in = in;
    r.n = inLen;
    r.pos = 0;
    r.blockLen = 0;
    r.chunkOff = 0;
    r.chunkLen = 0;
    r.internal = internal;
    r.internalLen = SNAPPY ? 0 : bufferSize + 8;
    r.internalMax = internalMax;
    r.chunk = in;
    r.eo = 0;
    r.lds = lds;
    r.lane = lane;
    r.snappy = SNAPPY;
    int32_t done = 0;
    int32_t result = 0;
    while (done < outCap) {
        const int32_t size = SNAPPY ? snappy_read(r, out + done, outCap - done, false) : lz4_read(r, out + done, outCap - done, false);
        if (size == STREAM_EOF) {
            break;
        }
        if (size < 0) {
            result = size;
            break;
        }
        done += size;
    }
    if (result == 0) {
        const int32_t b = SNAPPY ? snappy_read(r, nullptr, 0, true) : lz4_read(r, nullptr, 0, true);
        if (b >= 0) {
            r.eo = r.pos;
            result = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_HDP_NOT_CONSUMED);
        }
        else if (b != STREAM_EOF) {
            result = b;
        }
    }
    doneOut = done;
    eo = r.eo;
    return result;
}

template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_serial_decompress_kernel(BatchArgs a, uint8_t* internals, int32_t internalMax, int32_t bufferSize, int32_t* nextItem, const int32_t* only)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[IN_RING + OUT_RING];
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    uint8_t* internal = internals + (size_t)blockIdx.x * (size_t)internalMax;
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            item = atomicAdd(nextItem, 1);
        }
        __syncthreads();
        const int32_t s = item;
        if (s >= a.nBlocks) {
            return;
        }
        if (only != nullptr && only[s] == 0) {
            continue;  // done by the chunk-parallel path
        }
        int32_t done = 0;
        int64_t eo = 0;
        const int32_t st = decompress_item<SNAPPY>(a.srcBase + a.srcOff[s], a.srcLen[s], a.dstBase + a.dstOff[s], a.dstCap[s], internal, internalMax, bufferSize, lds, lane, done, eo);
        if (lane == 0) {
            a.outLen[s] = st == 0 ? done : 0;
            a.status[s] = st;
            a.errOffset[s] = st == 0 ? 0 : eo;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the general reader over a WINDOW (achip_window_decompress_batch): the same Java loops, a unit at a time.  At every unit boundary the reader is a fresh
// one over what is left of the window and of the destination, so whatever it reports is what the one-shot reader reports there; the end of the input in
// front of a whole unit is a stop, not an error.
struct WindowEnd {
    int32_t consumed, produced, stop;
    int64_t need;
    int32_t status;
    int64_t eo;
};

__device__ __forceinline__ bool is_truncation(int32_t st)
{
    return st == mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_TRUNCATED_INT) || st == mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_EOF_BLOCK_DATA);
}

// A block that does not fit what the destination has left: is it whole?  The reader's loop over its chunks without delivering a byte -- an LZ4 chunk is
// decoded into the stream's own buffer (what it produces is known no other way), a Snappy chunk announces it.  0: whole (a chunk the reader would refuse
// ends the unit too); STREAM_EOF or a truncation status: the window ends inside it.
template <bool SNAPPY>
__device__ int32_t skip_unit(Reader& r)
{
    for (;;) {
        const int32_t clen = next_chunk(r);
        if (clen < 0) {
            return clen == STREAM_EOF || is_truncation(clen) ? clen : 0;
        }
        int32_t w;
        if (SNAPPY) {
            int32_t beo = 0;
            w = snappy_announced(r.chunk, clen, beo);
            if (w <= 0 || w > r.blockLen) {
                return 0;
            }
        }
        else {
            w = lz4_decode(r, r.chunk, clen, r.internal, r.internalLen);
            if (w < 0) {
                return 0;
            }
        }
        r.chunkLen = w;
        r.chunkOff = w;
        if (r.blockLen == r.chunkOff) {
            return 0;
        }
    }
}

template <bool SNAPPY>
__device__ void window_item(const uint8_t* in, int32_t inLen, uint8_t* out, int32_t outCap, bool last, uint8_t* internal, int32_t internalMax, int32_t bufferSize, uint8_t* lds,
                            int lane, int32_t base, int32_t done, WindowEnd& e)
{
    Reader r;
    r.internal = internal;
    r.internalMax = internalMax;
    r.lds = lds;
    r.lane = lane;
    r.snappy = SNAPPY;
    e.need = 0;
    e.status = 0;
    e.eo = 0;
    for (;;) {
        // a unit boundary: a fresh reader over what is left of the window
        auto fresh = [&]() {
            r.in = in + base;
            r.n = inLen - base;
            r.pos = 0;
            r.blockLen = 0;
            r.chunkOff = 0;
            r.chunkLen = 0;
            r.internalLen = SNAPPY ? 0 : bufferSize + 8;
            r.chunk = r.in;
            r.eo = 0;
        };
        fresh();
        e.consumed = base;
        e.produced = done;
        if (r.n == 0) {
            e.stop = ACHIP_STOP_END;
            return;
        }
        const int32_t room = outCap - done;
        const int32_t u = r.n >= 4 ? rd_be(r.in) : 0;
        if (r.n >= 4 && u == 0) {
            base += 4;  // a zero length word
            continue;
        }
        const bool fits = u <= room;
        if (!fits) {
            const int32_t whole = skip_unit<SNAPPY>(r);
            if (whole == 0) {
                e.stop = ACHIP_STOP_NEED_ROOM;
                e.need = u;
                return;
            }
            if (!last) {
                e.stop = ACHIP_STOP_NEED_INPUT;
                e.need = whole == mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_EOF_BLOCK_DATA) ? (int64_t)r.pos + rd_be(r.in + r.pos - 4) : 0;
                return;
            }
            fresh();  // the stream ends inside this block: the reader decides, as in the one-shot call
        }
        int32_t result = 0, got = 0;
        bool closed = false;  // HadoopCodecDecompressor's one more read() behind its loop has been made
        for (;;) {
            if (got >= room) {  // (the loop ends here)
                const int32_t b = SNAPPY ? snappy_read(r, nullptr, 0, true) : lz4_read(r, nullptr, 0, true);
                if (b >= 0) {
                    r.eo = r.pos;
                    result = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_HDP_NOT_CONSUMED);
                }
                else {
                    result = b;
                }
                closed = true;
                break;
            }
            const int32_t size = SNAPPY ? snappy_read(r, out + done + got, room - got, false) : lz4_read(r, out + done + got, room - got, false);
            if (size < 0) {
                result = size;
                break;
            }
            got += size;
            if (r.blockLen == r.chunkOff && r.chunkOff >= r.chunkLen) {
                result = 0;  // the block is complete
                break;
            }
        }
        if (result == 0) {
            done += got;
            base += r.pos;
            continue;
        }
        bool ended = false;
        if (result == STREAM_EOF && last) {  // the reader's stream ends here: the one more read() decides, as in the one-shot call
            ended = true;
            if (!closed) {
                const int32_t b = SNAPPY ? snappy_read(r, nullptr, 0, true) : lz4_read(r, nullptr, 0, true);
                if (b >= 0) {
                    r.eo = r.pos;
                    result = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_HDP_NOT_CONSUMED);
                }
                else {
                    result = b;
                }
            }
            if (result == STREAM_EOF) {
                e.consumed = inLen;
                e.produced = done + got;
                e.stop = ACHIP_STOP_END;
                return;
            }
        }
        if (!ended && (result == STREAM_EOF || (is_truncation(result) && !last))) {
            e.stop = ACHIP_STOP_NEED_INPUT;
            e.need = result == mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_HDP_EOF_BLOCK_DATA) ? (int64_t)r.pos + rd_be(r.in + r.pos - 4) : 0;
            return;
        }
        if (!fits && result == mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_HDP_NOT_CONSUMED)) {
            e.stop = ACHIP_STOP_NEED_ROOM;
            e.need = u;
            return;
        }
        e.stop = ACHIP_STOP_FAILED;
        e.status = result;
        e.eo = (int64_t)base + r.eo;
        return;
    }
}

template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_serial_window_kernel(BatchArgs a, WindowArgs w, uint8_t* internals, int32_t internalMax, int32_t bufferSize, int32_t* nextItem,
                                                                  const int32_t* only, const int32_t* startPos, const int32_t* startOut)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[IN_RING + OUT_RING];
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    uint8_t* internal = internals + (size_t)blockIdx.x * (size_t)internalMax;
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            item = atomicAdd(nextItem, 1);
        }
        __syncthreads();
        const int32_t s = item;
        if (s >= a.nBlocks) {
            return;
        }
        if (only[s] == 0) {
            continue;  // finished by the chunk-parallel path
        }
        WindowEnd e;
        window_item<SNAPPY>(a.srcBase + a.srcOff[s], a.srcLen[s], a.dstBase + a.dstOff[s], a.dstCap[s], (w.flags[s] & ACHIP_WINDOW_LAST) != 0, internal, internalMax, bufferSize, lds,
                            lane, startPos[s], startOut[s], e);
        if (lane == 0) {
            win::report(a, w, s, e.consumed, e.produced, e.stop, e.need, e.status, e.eo);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the chunk-parallel reader
struct ChunkList : lists::ChunkBatch {  // per chunk: a batch for the block decoders (counters [16..]: probe statistics of the decoders' choice, [32] serial cursor) ...
    int32_t* cExpect;   // ... and the block length it has to produce
    // per stream
    int32_t* sFirst;
    int32_t* sCount;
    int32_t* sOut;      // plaintext bytes if every chunk decodes as declared
    int32_t* sSerial;   // 1: the serial kernel takes the stream
    void carve(lists::Carver& k, int64_t nStreams)
    {
        int32_t* counterWords = k.take<int32_t>(lists::COUNTER_WORDS);
        sFirst = k.take<int32_t>(nStreams);
        sCount = k.take<int32_t>(nStreams);
        sOut = k.take<int32_t>(nStreams);
        sSerial = k.take<int32_t>(nStreams);
        ChunkBatch::carve(k, counterWords);
        cExpect = k.take<int32_t>(CAPACITY);
    }
};

// A window's walk (achip_window_decompress_batch): where it stopped and why, and what it may list.
struct WindowWalk {
    bool last;           // ACHIP_WINDOW_LAST: an incomplete tail is the reader's truncation error, not a stop
    int32_t maxChunks;   // the list has room for this many
    int32_t* cUnit;      // per listed chunk: where its unit begins in the window
    int32_t pos;         // out: the end of the units walked
    int32_t stop;        // out: ACHIP_STOP_END / _NEED_INPUT / _NEED_ROOM (the list is full: need 0), or win::STOP_SERIAL
    int64_t need;
};

// The Java loops over one stream without the chunk bodies; returns false when the stream is not of the simple shape (the serial kernel
// then decodes it).  FILL = false: count the chunks; true: write their descriptors.
// WINDOW: the stream is a window.  The walk stops in front of the first unit that is not whole, does not fit or is not of the simple shape, says which in
// `w` and returns true: the units in front of it are listed.
template <bool SNAPPY, bool FILL, bool WINDOW = false>
__device__ bool walk_stream(const BatchArgs& a, const ChunkList& L, int32_t stream, int32_t first, int32_t& countOut, int32_t& outOut, WindowWalk* w = nullptr)
{
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[stream];
    const int32_t inLen = a.srcLen[stream];
    const int32_t outCap = a.dstCap[stream];
    int32_t pos = 0, o = 0, n = 0;
    countOut = 0;
    outOut = 0;
#define WALK_STOP(at, why, want)   \
    {                              \
        if (WINDOW) {              \
            w->pos = (at);         \
            w->stop = (why);       \
            w->need = (want);      \
            countOut = n;          \
            outOut = o;            \
        }                          \
        return WINDOW;             \
    }
    while (pos < inLen) {
        const int32_t unit = pos;
        if (WINDOW && n >= w->maxChunks) WALK_STOP(unit, ACHIP_STOP_NEED_ROOM, 0);
        if (inLen - pos < 4) WALK_STOP(unit, w->last ? win::STOP_SERIAL : ACHIP_STOP_NEED_INPUT, 0);
        const int32_t u = rd_be(in + pos);
        pos += 4;
        if (u == 0) {
            continue;  // `while (uncompressedBlockLength == 0)`
        }
        if (u < 0 || inLen - pos < 4) WALK_STOP(unit, u < 0 || w->last ? win::STOP_SERIAL : ACHIP_STOP_NEED_INPUT, 0);
        const int32_t clen = rd_be(in + pos);
        pos += 4;
        if (WINDOW && clen >= 0 && clen > inLen - pos && !w->last) WALK_STOP(unit, ACHIP_STOP_NEED_INPUT, (int64_t)clen + 8);
        if (clen < 0 || clen > inLen - pos || u > outCap - o) WALK_STOP(unit, win::STOP_SERIAL, 0);
        if (SNAPPY) {
            int32_t beo = 0;
            if (snappy_announced(in + pos, clen, beo) != u) WALK_STOP(unit, win::STOP_SERIAL, 0);
        }
        if (FILL) {
            const int32_t c = first + n;
            L.cSrcOff[c] = a.srcOff[stream] + pos;
            L.cSrcLen[c] = clen;
            L.cDstOff[c] = a.dstOff[stream] + o;
            L.cDstCap[c] = outCap - o;  // (what the Java reader hands its block decoder: the rest of the caller's buffer)
            L.cExpect[c] = u;
            if (WINDOW) {
                w->cUnit[c] = unit;
            }
        }
        n++;
        o += u;
        pos += clen;
    }
#undef WALK_STOP
    if (WINDOW) {
        w->pos = pos;
        w->stop = ACHIP_STOP_END;
        w->need = 0;
    }
    countOut = n;
    outOut = o;
    return true;
}

template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_walk_kernel(BatchArgs a, ChunkList L)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    int32_t n = 0, out = 0;
    const bool simple = walk_stream<SNAPPY, false>(a, L, stream, 0, n, out);
    const int32_t first = simple && n > 0 ? atomicAdd(L.counters, n) : 0;
    const bool fits = simple && (int64_t)first + n <= CAPACITY;
    L.sFirst[stream] = first;
    L.sCount[stream] = fits ? n : 0;
    L.sOut[stream] = out;
    L.sSerial[stream] = fits ? 0 : 1;
    if (fits && n > 0) {
        walk_stream<SNAPPY, true>(a, L, stream, first, n, out);
    }
    else if (simple && !fits) {  // the part of this stream's range that lies inside the arrays: empty blocks nobody looks at
        for (int64_t c = first; c < (int64_t)first + n && c < CAPACITY; c++) {
            L.cSrcOff[c] = 0;
            L.cSrcLen[c] = 0;
            L.cDstOff[c] = 0;
            L.cDstCap[c] = 0;
            L.cExpect[c] = -1;
        }
    }
}

__global__ __launch_bounds__(64) void hadoop_fold_kernel(BatchArgs a, ChunkList L)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks || L.sSerial[stream] != 0) {
        return;
    }
    const int32_t first = L.sFirst[stream], n = L.sCount[stream];
    bool ok = true;
    for (int32_t k = 0; k < n; k++) {
        ok = ok && L.cStatus[first + k] == 0 && L.cOutLen[first + k] == L.cExpect[first + k];
    }
    if (ok) {
        a.outLen[stream] = L.sOut[stream];
        a.status[stream] = 0;
        a.errOffset[stream] = 0;
    }
    else {
        L.sSerial[stream] = 1;  // a chunk failed or did not produce its block's length: the Java loops decide what that means
    }
}

// ---- the window forms of walk and fold (achip_window_decompress_batch) ----
struct WindowList : ChunkList {
    int32_t* cUnit;   // per chunk: where its unit begins in its window
    int32_t* sPos;    // per window: where the walk stopped; after the fold: where the serial kernel starts ...
    int32_t* sStart;  // ... and with how many bytes delivered
    int32_t* sStop;
    int64_t* sNeed;
    void carve(lists::Carver& k, int64_t nStreams)
    {
        ChunkList::carve(k, nStreams);
        sNeed = k.take<int64_t>(nStreams);
        sPos = k.take<int32_t>(nStreams);
        sStart = k.take<int32_t>(nStreams);
        sStop = k.take<int32_t>(nStreams);
        cUnit = k.take<int32_t>(CAPACITY);
    }
};

// a lane per window: the leading units of the writer's shape that are whole and fit go on the list -- as many as the list has room for
template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_window_walk_kernel(BatchArgs a, WindowList L, WindowArgs w)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    L.sFirst[stream] = 0;
    L.sCount[stream] = 0;
    L.sOut[stream] = 0;
    L.sPos[stream] = 0;
    L.sNeed[stream] = 0;
    if (a.srcLen[stream] < 0 || a.dstCap[stream] < 0) {
        L.sStop[stream] = ACHIP_STOP_FAILED;
        L.sSerial[stream] = 0;
        return;
    }
    WindowWalk ww;
    ww.last = (w.flags[stream] & ACHIP_WINDOW_LAST) != 0;
    ww.maxChunks = 0x7FFFFFFF;
    ww.cUnit = L.cUnit;
    int32_t n = 0, out = 0;
    walk_stream<SNAPPY, false, true>(a, L, stream, 0, n, out, &ww);
    const int32_t first = n > 0 ? atomicAdd(L.counters, n) : 0;
    if ((int64_t)first + n > CAPACITY) {  // the list takes what fits; with no room at all the serial kernel makes the progress
        ww.maxChunks = first < CAPACITY ? CAPACITY - first : 0;
        walk_stream<SNAPPY, false, true>(a, L, stream, 0, n, out, &ww);
        if (n == 0) {
            ww.stop = win::STOP_SERIAL;
        }
    }
    if (n > 0) {
        walk_stream<SNAPPY, true, true>(a, L, stream, first, n, out, &ww);
    }
    L.sFirst[stream] = first;
    L.sCount[stream] = n;
    L.sOut[stream] = out;
    L.sPos[stream] = ww.pos;
    L.sStop[stream] = ww.stop;
    L.sNeed[stream] = ww.need;
    L.sSerial[stream] = 0;
}

// a lane per window: the prefix of its listed chunks that decoded to their blocks' lengths is delivered; behind it the walk's stop stands, or the serial
// kernel goes on (sSerial, from sPos / sStart)
__global__ __launch_bounds__(64) void hadoop_window_fold_kernel(BatchArgs a, WindowList L, WindowArgs w)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    if (L.sStop[stream] == ACHIP_STOP_FAILED) {
        win::report(a, w, stream, 0, 0, ACHIP_STOP_FAILED, 0, mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT), 0);
        return;
    }
    const int32_t first = L.sFirst[stream], n = L.sCount[stream];
    int32_t pos = L.sPos[stream], out = L.sOut[stream], stop = L.sStop[stream];
    for (int32_t k = 0; k < n; k++) {
        if (L.cStatus[first + k] != 0 || L.cOutLen[first + k] != L.cExpect[first + k]) {
            pos = L.cUnit[first + k];
            out = (int32_t)(L.cDstOff[first + k] - a.dstOff[stream]);
            stop = win::STOP_SERIAL;  // the Java loops decide what this chunk means
            break;
        }
    }
    if (stop == win::STOP_SERIAL) {
        L.sSerial[stream] = 1;
        L.sPos[stream] = pos;
        L.sStart[stream] = out;
        return;
    }
    win::report(a, w, stream, pos, out, stop, L.sNeed[stream], 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// the writer
using BlockList = lists::WriterList;  // (bSize: a chunk's compressed bytes, or the block encoder's status)

template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_plan_kernel(BatchArgs a, BlockList L, int32_t bufferSize)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    const int32_t inLen = a.srcLen[stream];
    const int32_t chunk = input_max_size(SNAPPY, bufferSize);
    int32_t st = 0;
    int64_t chunks = 0;
    if (inLen < 0 || chunk <= 0) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    else {
        chunks = ((int64_t)inLen + chunk - 1) / chunk;
        const int64_t rest = (int64_t)inLen % chunk;
        const int64_t bound = ((int64_t)inLen / chunk) * (8 + block_bound(SNAPPY, chunk)) + (rest > 0 ? 8 + block_bound(SNAPPY, rest) : 0);
        if (bound > 0x7FFFFFFF) {
            st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
        }
        else if ((int64_t)a.dstCap[stream] < bound) {
            st = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_HDP_MAX_OUTPUT);
        }
    }
    if (!lists::plan_entries(L, stream, st == 0 ? (int32_t)chunks : 0)) {  // (more than a million chunks in one call)
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_UNSUPPORTED);
    }
    L.sStatus[stream] = st;
}

// The window form of the plan (achip_window_compress_batch): the full blocks the window holds and the destination has worst-case room for are taken, the
// partial tail only under ACHIP_WINDOW_LAST; taken[] is what the encode and compact kernels see as the input's length.
template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_window_plan_kernel(BatchArgs a, BlockList L, int32_t bufferSize, WindowArgs w, int32_t* taken)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    const int32_t inLen = a.srcLen[stream], cap = a.dstCap[stream];
    const int32_t chunk = input_max_size(SNAPPY, bufferSize);
    int32_t st = 0, stop = ACHIP_STOP_END;
    int64_t blocks = 0, consumed = 0, need = 0;
    if (inLen < 0 || cap < 0 || chunk <= 0) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    else {
        const int64_t worst = 8 + block_bound(SNAPPY, chunk);
        const int64_t full = inLen / chunk, rest = inLen % chunk;
        blocks = full < cap / worst ? full : cap / worst;
        consumed = blocks * chunk;
        if (blocks < full) {
            stop = ACHIP_STOP_NEED_ROOM;
            need = worst;
        }
        else if (rest > 0 && (w.flags[stream] & ACHIP_WINDOW_LAST) == 0) {
            stop = ACHIP_STOP_NEED_INPUT;
            need = chunk;
        }
        else if (rest > 0 && cap - blocks * worst < 8 + block_bound(SNAPPY, rest)) {
            stop = ACHIP_STOP_NEED_ROOM;
            need = 8 + block_bound(SNAPPY, rest);
        }
        else if (rest > 0) {
            blocks++;
            consumed += rest;
        }
    }
    if (!lists::plan_entries(L, stream, st == 0 ? (int32_t)blocks : 0)) {  // (more than a million chunks in one call)
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_UNSUPPORTED);
    }
    L.sStatus[stream] = st;
    taken[stream] = st == 0 ? (int32_t)consumed : 0;
    w.consumed[stream] = st == 0 ? consumed : 0;
    w.stop[stream] = st == 0 ? stop : ACHIP_STOP_FAILED;
    w.need[stream] = st == 0 ? need : 0;
}

// LZ4: a wavefront per workgroup around its table in LDS.  Snappy (round 3): the two tiers of the block encoder (snappy_compress.hip) -- a 32 KB
// table allows five workgroups per CU, so a workgroup is four independent persistent wavefronts: wavefront 0 with the table in LDS, the others with a
// table slab each in memory, all drawing chunks from the one counter.
template <bool SNAPPY>
__global__ __launch_bounds__(SNAPPY ? 256 : 64) void hadoop_encode_kernel(BatchArgs a, BlockList L, int32_t bufferSize, uint16_t* slabs)
{
    // the codec's hash table: Snappy 16384 x u16; LZ4 4096 entries, u16 for chunks <= 64 KiB, i32 beyond
    __shared__ __attribute__((aligned(16))) uint8_t tableBytes[SNAPPY ? snc::MAX_HASH_TABLE_SIZE * 2 : lz4c::MAX_TABLE_SIZE * 4];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint16_t* const snappyTable = !SNAPPY || wave == 0 ? (uint16_t*)tableBytes : slabs + ((size_t)blockIdx.x * 3 + (wave - 1)) * snc::MAX_HASH_TABLE_SIZE;
    const int32_t total = L.counters[1];
    const int32_t chunk = input_max_size(SNAPPY, bufferSize);
    const int64_t worst = 8 + block_bound(SNAPPY, chunk);
    for (;;) {
        int32_t b = 0;
        if (lane == 0) {
            b = atomicAdd(L.counters + 2, 1);
        }
        b = __builtin_amdgcn_readfirstlane(b);
        if (b >= total) {
            return;
        }
        const int32_t stream = L.bStream[b];
        if (stream < 0) {
            continue;
        }
        const int32_t k = L.bIndex[b];
        const int64_t pos = (int64_t)k * chunk;
        const int32_t inLen = a.srcLen[stream];
        const int32_t length = (int32_t)(inLen - pos < chunk ? inLen - pos : chunk);
        const uint8_t* block = a.srcBase + a.srcOff[stream] + pos;
        uint8_t* out = a.dstBase + a.dstOff[stream] + (int64_t)k * worst + 8;
        const int32_t cap = (int32_t)block_bound(SNAPPY, length);
        int32_t cst = 0, compressed = 0;
        if (SNAPPY) {
            if (wave == 0) {  // (two calls: the table's address space is part of the code)
                snappy_compress_buffer_mw((uint16_t*)tableBytes, block, length, out, cap, lane, cst, compressed);
            }
            else {
                snappy_compress_buffer_mw(snappyTable, block, length, out, cap, lane, cst, compressed);
            }
        }
        else if (length <= 65536) {
            compressed = lz4_compress_block_mw<uint16_t>(block, length, out, cap, (uint16_t*)tableBytes, lane, cst);
        }
        else {
            compressed = lz4_compress_block_mw<int32_t>(block, length, out, cap, (int32_t*)tableBytes, lane, cst);
        }
        wave_mem_order();
        if (lane == 0) {
            L.bSize[b] = cst == 0 ? compressed : cst;
        }
    }
}

template <bool SNAPPY>
__global__ __launch_bounds__(64) void hadoop_compact_kernel(BatchArgs a, BlockList L, int32_t bufferSize)
{
    const int lane = threadIdx.x;
    const int32_t chunk = input_max_size(SNAPPY, bufferSize);
    const int64_t worst = 8 + block_bound(SNAPPY, chunk);
    const int32_t stream = blockIdx.x;  // a wavefront per stream
    int32_t st = L.sStatus[stream];
    int32_t o = 0;
    if (st == 0) {
        uint8_t* out = a.dstBase + a.dstOff[stream];
        const int32_t inLen = a.srcLen[stream];
        const int32_t first = L.sFirst[stream], n = L.sCount[stream];
        for (int32_t k = 0; k < n; k++) {
            const int32_t size = L.bSize[first + k];
            if (size < 0) {
                st = size;  // (the block encoder's status)
                break;
            }
            const int64_t from = (int64_t)k * worst + 8;
            const int64_t pos = (int64_t)k * chunk;
            const int32_t length = (int32_t)(inLen - pos < chunk ? inLen - pos : chunk);
            wave_mem_order();
            if (from != (int64_t)o + 8) {
                group_copy<64>(out + o + 8, out + from, size, lane);  // to the left; every lane loads before it stores
                wave_mem_order();
            }
            if (lane == 0) {  // writeNextChunk :107-118 (written after the move: the fields of chunk k may lie inside chunk k - 1's worst-case slot)
                wr_be(out + o, length);
                wr_be(out + o + 4, size);
            }
            wave_mem_order();
            o += 8 + size;
        }
    }
    if (lane == 0) {
        a.outLen[stream] = st == 0 ? o : 0;
        a.status[stream] = st;
        a.errOffset[stream] = 0;
    }
}

}  // namespace hdp

namespace {
constexpr int HDP_SERIAL_WAVES = 1024;
int64_t hdp_internal_bytes(int32_t bufferSize)
{
    const int64_t b = bufferSize > 262144 ? bufferSize : 262144;
    return (b + 8 + 63) & ~(int64_t)63;
}
}  // namespace

// the reader's scratch: its lists, then the serial kernel's buffers, one per wavefront
static uint8_t* carve_hadoop_reader(lists::Carver& k, hdp::ChunkList& L, int64_t nStreams, int32_t bufferSize)
{
    L.carve(k, nStreams);
    return k.take<uint8_t>((nStreams < HDP_SERIAL_WAVES ? nStreams : HDP_SERIAL_WAVES) * hdp_internal_bytes(bufferSize));
}

int64_t hadoop_decompress_scratch_bytes(int32_t nStreams, int32_t bufferSize)
{
    lists::Carver k(nullptr);
    hdp::ChunkList L;
    carve_hadoop_reader(k, L, nStreams < 1 ? 1 : nStreams, bufferSize);
    return k.used();
}

// variant 0: a wavefront per stream only.  The others list the chunks and hand them to launch_listed_decode (achip_launch.h): 1, or no `aux`:
// without a synchronisation; 2: always through the two-pass decoders -- their record arena is sized by the chunk count, which only
// the device knows, so the host reads it back (one synchronisation) and asks `aux` for the arena; 3 (the default): the length probe of the
// block API's auto mode decides between the two.
hipError_t launch_hadoop_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize, int variant, const AuxScratch* aux, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    hdp::ChunkList L;
    uint8_t* internals = carve_hadoop_reader(k, L, a.nBlocks, bufferSize);
    int32_t* counters = L.counters;
    hipError_t e = hipMemsetAsync(counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const int64_t internalMax = hdp_internal_bytes(bufferSize);
    const unsigned serialGrid = (unsigned)(a.nBlocks < HDP_SERIAL_WAVES ? a.nBlocks : HDP_SERIAL_WAVES);
    if (variant == 0) {  // one wavefront per stream only
        if (snappy) hipLaunchKernelGGL(hdp::hadoop_serial_decompress_kernel<true>, dim3(serialGrid), dim3(64), 0, stream, a, internals, (int32_t)internalMax, bufferSize, counters + 32, (const int32_t*)nullptr);
        else hipLaunchKernelGGL(hdp::hadoop_serial_decompress_kernel<false>, dim3(serialGrid), dim3(64), 0, stream, a, internals, (int32_t)internalMax, bufferSize, counters + 32, (const int32_t*)nullptr);
        return hipGetLastError();
    }
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    if (snappy) hipLaunchKernelGGL(hdp::hadoop_walk_kernel<true>, dim3(perStream), dim3(64), 0, stream, a, L);
    else hipLaunchKernelGGL(hdp::hadoop_walk_kernel<false>, dim3(perStream), dim3(64), 0, stream, a, L);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, counters, lists::CAPACITY);
    // records per chunk as for 64 KiB blocks, scaled to the streams' chunk size
    const bool sync = (variant == 2 || variant == 3) && aux != nullptr && aux->get != nullptr;
    const ListedWant want{sync, variant == 3, true, ((int64_t)(bufferSize > 65536 ? bufferSize : 65536) + 65535) / 65536, -1};
    bool decoded = false;
    e = launch_listed_decode(L.as_batch(a, lists::CAPACITY), snappy ? 1 : 0, stream, counters, counters + 16, aux, ks, want, &decoded);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hdp::hadoop_fold_kernel, dim3(perStream), dim3(64), 0, stream, a, L);
    // streams of any other shape, and those a chunk of which did not decode as declared
    if (snappy) hipLaunchKernelGGL(hdp::hadoop_serial_decompress_kernel<true>, dim3(serialGrid), dim3(64), 0, stream, a, internals, (int32_t)internalMax, bufferSize, counters + 32, (const int32_t*)L.sSerial);
    else hipLaunchKernelGGL(hdp::hadoop_serial_decompress_kernel<false>, dim3(serialGrid), dim3(64), 0, stream, a, internals, (int32_t)internalMax, bufferSize, counters + 32, (const int32_t*)L.sSerial);
    return hipGetLastError();
}

// ---- windows (achip_window_decompress_batch / _compress_batch) ----
static uint8_t* carve_hadoop_window_reader(lists::Carver& k, hdp::WindowList& L, int64_t nStreams, int32_t bufferSize)
{
    L.carve(k, nStreams);
    return k.take<uint8_t>((nStreams < HDP_SERIAL_WAVES ? nStreams : HDP_SERIAL_WAVES) * hdp_internal_bytes(bufferSize));
}

int64_t hadoop_window_decompress_scratch_bytes(int32_t nStreams, int32_t bufferSize)
{
    lists::Carver k(nullptr);
    hdp::WindowList L;
    carve_hadoop_window_reader(k, L, nStreams < 1 ? 1 : nStreams, bufferSize);
    return k.used();
}

// walk -> seal -> the listed chunks through the block decoders (as the one-shot reader's variants 1 .. 3) -> fold -> the wavefront-per-stream kernel for the
// windows the fold could not finish
hipError_t launch_hadoop_window_decompress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize, int variant,
                                           const AuxScratch* aux, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    hdp::WindowList L;
    uint8_t* internals = carve_hadoop_window_reader(k, L, a.nBlocks, bufferSize);
    int32_t* counters = L.counters;
    hipError_t e = hipMemsetAsync(counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const int64_t internalMax = hdp_internal_bytes(bufferSize);
    const unsigned serialGrid = (unsigned)(a.nBlocks < HDP_SERIAL_WAVES ? a.nBlocks : HDP_SERIAL_WAVES);
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    if (snappy) hipLaunchKernelGGL(hdp::hadoop_window_walk_kernel<true>, dim3(perStream), dim3(64), 0, stream, a, L, w);
    else hipLaunchKernelGGL(hdp::hadoop_window_walk_kernel<false>, dim3(perStream), dim3(64), 0, stream, a, L, w);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, counters, lists::CAPACITY);
    const bool sync = (variant == 2 || variant == 3) && aux != nullptr && aux->get != nullptr;
    const ListedWant want{sync, variant == 3, true, ((int64_t)(bufferSize > 65536 ? bufferSize : 65536) + 65535) / 65536, -1};
    bool decoded = false;
    e = launch_listed_decode(L.as_batch(a, lists::CAPACITY), snappy ? 1 : 0, stream, counters, counters + 16, aux, ks, want, &decoded);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hdp::hadoop_window_fold_kernel, dim3(perStream), dim3(64), 0, stream, a, L, w);
    if (snappy) hipLaunchKernelGGL(hdp::hadoop_serial_window_kernel<true>, dim3(serialGrid), dim3(64), 0, stream, a, w, internals, (int32_t)internalMax, bufferSize, counters + 32, (const int32_t*)L.sSerial, (const int32_t*)L.sPos, (const int32_t*)L.sStart);
    else hipLaunchKernelGGL(hdp::hadoop_serial_window_kernel<false>, dim3(serialGrid), dim3(64), 0, stream, a, w, internals, (int32_t)internalMax, bufferSize, counters + 32, (const int32_t*)L.sSerial, (const int32_t*)L.sPos, (const int32_t*)L.sStart);
    return hipGetLastError();
}

namespace {
constexpr int HADOOP_SNAPPY_WORKGROUPS = 256 * 5;  // five 32 KB LDS tables per CU, four wavefronts around each
constexpr int64_t HADOOP_SNAPPY_SLAB_WORDS = (int64_t)HADOOP_SNAPPY_WORKGROUPS * 3 * snc::MAX_HASH_TABLE_SIZE;
// the writer's scratch: its list, then the Snappy encoder's table slabs
uint16_t* carve_hadoop_writer(lists::Carver& k, hdp::BlockList& L, int64_t nStreams)
{
    L.carve(k, k.take<int32_t>(lists::COUNTER_WORDS), nStreams, false);
    return k.take<uint16_t>(HADOOP_SNAPPY_SLAB_WORDS);
}
}

int64_t hadoop_compress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    hdp::BlockList L;
    carve_hadoop_writer(k, L, nStreams < 1 ? 1 : nStreams);
    return k.used();
}

hipError_t launch_hadoop_compress(const BatchArgs& a, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    hdp::BlockList L;
    uint16_t* const slabs = carve_hadoop_writer(k, L, a.nBlocks);
    hipError_t e = hipMemsetAsync(L.counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    const unsigned encodeGrid = snappy ? HADOOP_SNAPPY_WORKGROUPS : 256 * 10;  // (LZ4: chunks beyond 64 KiB take the 16 KB table: ten wavefronts per CU)
    const unsigned compactGrid = (unsigned)a.nBlocks;
    if (snappy) {
        hipLaunchKernelGGL(hdp::hadoop_plan_kernel<true>, dim3(perStream), dim3(64), 0, stream, a, L, bufferSize);
        hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, lists::CAPACITY);
        hipLaunchKernelGGL(hdp::hadoop_encode_kernel<true>, dim3(encodeGrid), dim3(256), 0, stream, a, L, bufferSize, slabs);
        hipLaunchKernelGGL(hdp::hadoop_compact_kernel<true>, dim3(compactGrid), dim3(64), 0, stream, a, L, bufferSize);
    }
    else {
        hipLaunchKernelGGL(hdp::hadoop_plan_kernel<false>, dim3(perStream), dim3(64), 0, stream, a, L, bufferSize);
        hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, lists::CAPACITY);
        hipLaunchKernelGGL(hdp::hadoop_encode_kernel<false>, dim3(encodeGrid), dim3(64), 0, stream, a, L, bufferSize, slabs);
        hipLaunchKernelGGL(hdp::hadoop_compact_kernel<false>, dim3(compactGrid), dim3(64), 0, stream, a, L, bufferSize);
    }
    return hipGetLastError();
}

int64_t hadoop_window_compress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    hdp::BlockList L;
    carve_hadoop_writer(k, L, nStreams < 1 ? 1 : nStreams);
    k.take<int32_t>(nStreams < 1 ? 1 : nStreams);
    return k.used();
}

// the window plan, then the one-shot writer's encode and compact kernels over what the plan took
hipError_t launch_hadoop_window_compress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    hdp::BlockList L;
    uint16_t* const slabs = carve_hadoop_writer(k, L, a.nBlocks);
    int32_t* const taken = k.take<int32_t>(a.nBlocks);
    hipError_t e = hipMemsetAsync(L.counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    BatchArgs t = a;
    t.srcLen = taken;
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    const unsigned encodeGrid = snappy ? HADOOP_SNAPPY_WORKGROUPS : 256 * 10;
    const unsigned compactGrid = (unsigned)a.nBlocks;
    if (snappy) {
        hipLaunchKernelGGL(hdp::hadoop_window_plan_kernel<true>, dim3(perStream), dim3(64), 0, stream, a, L, bufferSize, w, taken);
        hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, lists::CAPACITY);
        hipLaunchKernelGGL(hdp::hadoop_encode_kernel<true>, dim3(encodeGrid), dim3(256), 0, stream, t, L, bufferSize, slabs);
        hipLaunchKernelGGL(hdp::hadoop_compact_kernel<true>, dim3(compactGrid), dim3(64), 0, stream, t, L, bufferSize);
    }
    else {
        hipLaunchKernelGGL(hdp::hadoop_window_plan_kernel<false>, dim3(perStream), dim3(64), 0, stream, a, L, bufferSize, w, taken);
        hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, lists::CAPACITY);
        hipLaunchKernelGGL(hdp::hadoop_encode_kernel<false>, dim3(encodeGrid), dim3(64), 0, stream, t, L, bufferSize, slabs);
        hipLaunchKernelGGL(hdp::hadoop_compact_kernel<false>, dim3(compactGrid), dim3(64), 0, stream, t, L, bufferSize);
    }
    hipLaunchKernelGGL(win::writer_verdict_kernel, dim3(perStream), dim3(64), 0, stream, a, w);
    return hipGetLastError();
}

}  // namespace achip
