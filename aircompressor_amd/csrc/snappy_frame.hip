// snappy_frame.hip -- batched x-snappy-framed stream decode / encode for gfx950.
//
// Replaces the read-to-the-end use of SnappyFramedInputStream (M/snappy/SnappyFramedInputStream.java:52-73 stream header,
// :135-214 ensureBuffer, :226-305 chunk headers) and the write-all-then-close use of SnappyFramedOutputStream
// (M/snappy/SnappyFramedOutputStream.java:73-96, :113-145, :200-255) over the HIP block codec.  An item of the batch is
// a whole stream.  One wavefront per item, persistent grid: the chunk walk is a serial chain (a chunk's position is known
// only after the one before it), so the wavefront runs the Java loop itself -- same checks in the same order -- and puts
// its 64 lanes into each step: the ring block decoder of snappy_decode_body.h (64 lanes per chunk), 64 x 16-byte copies
// for stored chunks, the row-parallel CRC-32C of achip_crc32c.h for the masked checksums, the batch-probing block encoder
// of snappy_compress_body.h.  Throughput comes from many streams per batch.
// What the one-shot form adds to the Java classes: the destination capacity (ACHIP_D_SNF_OUTPUT_TOO_SMALL / _MAX_OUTPUT); the
// offset reported with the stream-level IOExceptions, which carry none (the position of the chunk header); the capacity handed
// to the block decoder (the Java reader's buffer of max(65541, everything seen so far) bytes, limited by what the destination
// has left); a chunk that ends inside its length preamble is ACHIP_D_SNAPPY_TRUNCATED (Java would read stale buffer bytes).
#include "snappy_decode_body.h"
#include "snappy_compress_mw.h"
#include "achip_crc32c.h"
#include "achip_launch.h"
#include "achip_lists.h"
#include "achip_window.h"
#include "achip_bounds.h"

namespace achip {

namespace snf {
constexpr int COMPRESSED_DATA_FLAG = 0x00, UNCOMPRESSED_DATA_FLAG = 0x01, STREAM_IDENTIFIER_FLAG = 0xff;
constexpr int MAX_BLOCK_SIZE = 65536;
constexpr int IN_RING = 2048, OUT_RING = 4096;

#define SNF_FAIL(detail, off)                          \
    {                                                  \
        eo = (int64_t)(off);                           \
        return mk_status(ACHIP_CLASS_MALFORMED, detail); \
    }

// readUncompressedLength of a chunk's data, for decompress_item alone: a restatement of snappy_read_uncompressed_length (achip_device.h; walk_stream below
// calls that one) kept because with the call snappyframed_decompress_kernel -- one instruction more -- read 1 024 streams of 4 MiB in 63.51 ms against 63.04
// and 408.12 against 407.16 (medians of three; the old code's runs lay within 0.27 and 0.64), profiles/twopass_refactor_ab.txt.  A change there belongs here too.
__device__ __forceinline__ int32_t read_uncompressed_length(const uint8_t* in, int32_t len, int32_t& expectedOut, int32_t& eoOut)
{
    uint32_t expected = 0;
    int32_t nread = 0;
    for (int i = 0; i < 5; i++) {
        if (nread >= len) {
            eoOut = len - nread;
            return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_SNAPPY_TRUNCATED);
        }
        const uint32_t b = in[nread++];
        expected |= (b & 0x7f) << (7 * i);
        if ((b & 0x80) == 0) {
            break;
        }
        if (i == 4) {
            eoOut = nread;
            return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_SNAPPY_LEN_HIGH_BIT);
        }
    }
    if ((int32_t)expected < 0) {
        eoOut = 0;
        return mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_SNAPPY_INVALID_LENGTH);
    }
    expectedOut = (int32_t)expected;
    return 0;
}

// VERIFY: SnappyFramedInputStream's verifyChecksums (:74-79, :188-193).  false: the checksum field is not looked at and no CRC is computed.
template <bool VERIFY>
__device__ int32_t decompress_item(const Crc32cTables& tables, const uint8_t* __restrict__ in, int32_t inLen, uint8_t* out, int32_t outCap, uint8_t* lds, int lane,
                                   int32_t& opOut, int64_t& eo)
{
    eo = 0;
    opOut = 0;
    if (inLen < 10) SNF_FAIL(ACHIP_D_SNF_EOF_STREAM_HEADER, 0);  // :66-69
    if (ld8(in) != 0x50614E73000006FFull || in[8] != 0x70 || in[9] != 0x59) SNF_FAIL(ACHIP_D_SNF_BAD_STREAM_HEADER, 0);  // ff 06 00 00 "sNaPpY" :70-72
    int32_t pos = 10;
    int32_t o = 0;
    int32_t javaInput = MAX_BLOCK_SIZE + 5, javaUncompressed = MAX_BLOCK_SIZE + 5;  // allocateBuffersBasedOnSize(MAX_BLOCK_SIZE + 5) :61
    for (;;) {
        const int32_t chunk = pos;
        if (pos == inLen) {
            break;  // readBlockHeader: end of stream :295-297
        }
        if (inLen - pos < 4) SNF_FAIL(ACHIP_D_SNF_EOF_BLOCK_HEADER, chunk);  // :299-301
        const uint32_t header = ld4(in + pos);
        const int flag = (int)(header & 0xFF);
        const int32_t length = (int32_t)(header >> 8);
        pos += 4;
        bool skip = false;
        int32_t minLength;
        if (flag == COMPRESSED_DATA_FLAG || flag == UNCOMPRESSED_DATA_FLAG) {  // getFrameMetaData :234-277
            minLength = 5;
        }
        else if (flag == STREAM_IDENTIFIER_FLAG) {
            if (length != 6) SNF_FAIL(ACHIP_D_SNF_STREAM_ID_LENGTH, chunk);
            skip = true;
            minLength = 6;
        }
        else {
            if (flag <= 0x7f) SNF_FAIL(ACHIP_D_SNF_UNSKIPPABLE, chunk);
            skip = true;
            minLength = 0;
        }
        if (length < minLength) SNF_FAIL(ACHIP_D_SNF_INVALID_LENGTH, chunk);
        if (skip) {  // :151-154; skip stops quietly at the end of the stream
            pos += length < inLen - pos ? length : inLen - pos;
            continue;
        }
        if (length > javaInput) {  // :156-158
            javaInput = length;
            javaUncompressed = javaUncompressed < length ? length : javaUncompressed;
        }
        if (inLen - pos < length) SNF_FAIL(ACHIP_D_SNF_EOF_FRAME, chunk);  // :160-163
        const uint32_t stored = ld4(in + pos);                             // getFrameData :279-288
        const uint8_t* data = in + pos + 4;
        const int32_t dlen = length - 4;
        int32_t produced;
        if (flag == COMPRESSED_DATA_FLAG) {  // :167-177
            int32_t ulen = 0, beo = 0;
            const int32_t pst = read_uncompressed_length(data, dlen, ulen, beo);
            if (pst != 0) {
                eo = (int64_t)beo;
                return pst;
            }
            javaUncompressed = javaUncompressed < ulen ? ulen : javaUncompressed;
            if (ulen > outCap - o) {
                eo = (int64_t)chunk;
                return mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_SNF_OUTPUT_TOO_SMALL);
            }
            const int32_t limit = javaUncompressed < outCap - o ? javaUncompressed : outCap - o;
            int32_t bst = 0, bop = 0;
            wave_mem_order();
            snappy_buffer_decode<64, IN_RING, OUT_RING, 1>(lds, lds + IN_RING, nullptr, data, dlen, out + o, limit, lane, bst, beo, bop);
            wave_mem_order();
            if (bst != 0) {
                eo = (int64_t)beo;  // the block codec's exception propagates with its own offset
                return bst;
            }
            produced = bop;
        }
        else {  // raw :178-186
            if (dlen > outCap - o) {
                eo = (int64_t)chunk;
                return mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_SNF_OUTPUT_TOO_SMALL);
            }
            wave_mem_order();
            group_copy<64>(out + o, data, dlen, lane);
            wave_mem_order();
            produced = dlen;
        }
        if constexpr (VERIFY) {
            if (stored != crc32c_mask(wave_crc32c(tables, out + o, produced, lane))) SNF_FAIL(ACHIP_D_SNF_CHECKSUM, chunk);  // :188-193
        }
        o += produced;
        pos += length;
    }
    opOut = o;
    return 0;
}
#undef SNF_FAIL

}  // namespace snf

template <bool VERIFY>
__device__ __forceinline__ void snappyframed_decompress_items(const BatchArgs& a, int32_t* nextItem, const int32_t* only)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[snf::IN_RING + snf::OUT_RING];
    __shared__ Crc32cTables tables;
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    if constexpr (VERIFY) {
        crc32c_tables_init(tables, lane);
    }
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            item = atomicAdd(nextItem, 1);
        }
        __syncthreads();
        const int32_t block = item;
        if (block >= a.nBlocks) {
            return;
        }
        if (only != nullptr && only[block] == 0) {
            continue;  // done by the chunk-parallel path
        }
        int32_t op = 0;
        int64_t eo = 0;
        const int32_t st = snf::decompress_item<VERIFY>(tables, a.srcBase + a.srcOff[block], a.srcLen[block], a.dstBase + a.dstOff[block], a.dstCap[block], lds, lane, op, eo);
        if (lane == 0) {
            a.outLen[block] = st == 0 ? op : 0;
            a.status[block] = st;
            a.errOffset[block] = st == 0 ? 0 : eo;
        }
    }
}

__global__ __launch_bounds__(64) void snappyframed_decompress_kernel(BatchArgs a, int32_t* nextItem, const int32_t* only)
{
    snappyframed_decompress_items<true>(a, nextItem, only);
}

// verifyChecksums = false (achip_ctx_set_snappyframed_verify_checksums)
__global__ __launch_bounds__(64) void snappyframed_decompress_noverify_kernel(BatchArgs a, int32_t* nextItem, const int32_t* only)
{
    snappyframed_decompress_items<false>(a, nextItem, only);
}

namespace snf {
constexpr int64_t SLAB_BYTES = (32 + MAX_BLOCK_SIZE + MAX_BLOCK_SIZE / 6 + 63) / 64 * 64;  // maxCompressedLength(65536), rounded

// The constructor's arguments (SnappyFramedOutputStream.java:77-91; achip_ctx_set_snappyframed_writer), the same for every lane of a launch: blockSize in
// (0, 65536] cuts the input, a chunk is kept compressed at (double)compressed / (double)length <= minRatio (:213, a correctly rounded fp64 division: this
// file is built without fast-math), and without checksums the CRC field is 0 and no CRC is computed (:203).
struct WriterParams {
    int32_t blockSize;
    int32_t checksums;
    double minRatio;
};

// new SnappyFramedOutputStream(c, out, writeChecksums, blockSize, minCompressionRatio); write(all); close()  -- M/snappy/SnappyFramedOutputStream.java:73-96, 113-145, 158-171
__device__ int32_t compress_item(const WriterParams& p, const Crc32cTables& tables, uint16_t* table, const uint8_t* __restrict__ in, int32_t inLen, uint8_t* out, int32_t outCap,
                                 uint8_t* slab, int lane, int32_t& opOut)
{
    const int32_t blockSize = p.blockSize;
    opOut = 0;
    if (inLen < 0) {
        return mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    const int64_t bound = bound::snappyframed(inLen, blockSize);  // achip_snappyframed_max_compressed_length_for
    if (bound > 0x7FFFFFFF) {
        return mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    if ((int64_t)outCap < bound) {
        return mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_SNF_MAX_OUTPUT);
    }
    if (lane == 0) {  // constructor :94
        st8(out, 0x50614E73000006FFull);
        out[8] = 0x70;
        out[9] = 0x59;
    }
    int32_t o = 10;
    for (int64_t pos = 0; pos < inLen; pos += blockSize) {  // full blocks straight from the input, the rest through the buffer :126-145, :186-192
        const int32_t length = (int32_t)(inLen - pos < blockSize ? inLen - pos : blockSize);
        const uint8_t* block = in + pos;
        const uint32_t crc = p.checksums != 0 ? crc32c_mask(wave_crc32c(tables, block, length, lane)) : 0u;  // writeCompressed :203
        int32_t cst = 0, compressed = 0;
        snappy_compress_buffer_mw(table, block, length, slab, (int32_t)SLAB_BYTES, lane, cst, compressed);  // :206-211
        wave_mem_order();
        if (cst != 0) {
            return cst;
        }
        const bool keep = ((double)compressed / (double)length) <= p.minRatio;  // :213
        const uint8_t* data = keep ? slab : block;
        const int32_t dlen = keep ? compressed : length;
        if (lane == 0) {  // writeBlock :241-254
            const uint32_t headerLength = (uint32_t)dlen + 4u;
            st4(out + o, (keep ? (uint32_t)COMPRESSED_DATA_FLAG : (uint32_t)UNCOMPRESSED_DATA_FLAG) | (headerLength << 8));
            st4(out + o + 4, crc);
        }
        group_copy<64>(out + o + 8, data, dlen, lane);
        wave_mem_order();
        o += 8 + dlen;
    }
    opOut = o;
    return 0;
}
}  // namespace snf

__global__ __launch_bounds__(64) void snappyframed_compress_kernel(BatchArgs a, snf::WriterParams p, uint8_t* slabs, int32_t* nextItem, const int32_t* only)
{
    __shared__ uint16_t table[snc::MAX_HASH_TABLE_SIZE];
    __shared__ Crc32cTables tables;
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    if (p.checksums != 0) {
        crc32c_tables_init(tables, lane);
    }
    uint8_t* slab = slabs + (size_t)blockIdx.x * snf::SLAB_BYTES;
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            item = atomicAdd(nextItem, 1);
        }
        __syncthreads();
        const int32_t block = item;
        if (block >= a.nBlocks) {
            return;
        }
        if (only != nullptr && only[block] == 0) {
            continue;  // done by the block-parallel path
        }
        int32_t op = 0;
        const int32_t st = snf::compress_item(p, tables, table, a.srcBase + a.srcOff[block], a.srcLen[block], a.dstBase + a.dstOff[block], a.dstCap[block], slab, lane, op);
        if (lane == 0) {
            a.outLen[block] = st == 0 ? op : 0;
            a.status[block] = st;
            a.errOffset[block] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Block-parallel writer (the default).  The blocks of a stream are independent; only a chunk's position depends on the
// sizes of the chunks before it.  But every block except a stream's last is full, and a chunk is never larger than its block
// stored raw, so block k can be written at its WORST-CASE position 10 + k * (8 + blockSize) without knowing anything else:
//   plan     one lane per stream checks the arguments and appends its blocks to one list;
//   encode   persistent wavefronts (two tiers, as in snappy_compress.hip) take blocks from the list: masked CRC-32C, the block
//            encoder into a private slab, the ratio rule (0.85 unless set), chunk header + body to the worst-case position, the chunk's size noted;
//   compact  one wavefront per stream writes the stream header and moves the chunks left into place, in order (a move to the
//            left with all loads of a round before its stores is safe at any distance).
// Streams whose blocks do not fit into the list go to the one-wavefront-per-stream kernel above.
namespace snf {
__device__ __forceinline__ int64_t worst_chunk(int32_t blockSize) { return 8 + (int64_t)blockSize; }
using BlockList = lists::WriterList;  // (bSize: a chunk's bytes, header included; counters [32]: the serial kernel's cursor)

__global__ __launch_bounds__(64) void snappyframed_plan_kernel(BatchArgs a, BlockList L, int32_t blockSize, int32_t capacity)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    const int32_t inLen = a.srcLen[stream];
    int32_t st = 0;
    int64_t blocks = 0;
    if (inLen < 0) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    else {
        blocks = ((int64_t)inLen + blockSize - 1) / blockSize;
        const int64_t bound = bound::snappyframed(inLen, blockSize);  // achip_snappyframed_max_compressed_length_for
        if (bound > 0x7FFFFFFF) {
            st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
        }
        else if ((int64_t)a.dstCap[stream] < bound) {
            st = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_SNF_MAX_OUTPUT);
        }
    }
    const bool fits = lists::plan_entries(L, stream, st == 0 ? (int32_t)blocks : 0, capacity);
    L.sStatus[stream] = st;
    L.sSerial[stream] = fits ? 0 : 1;  // (its stream goes the other way)
}

// WINDOW (achip_window_compress_batch): the stream identifier is there only where head[stream] says so, and a.srcLen is what the window plan took
template <bool WINDOW>
__device__ __forceinline__ void encode_blocks(const BatchArgs& a, const BlockList& L, const WriterParams& p, uint8_t* outSlabs, uint16_t* tableSlabs, const int32_t* head)
{
    __shared__ uint16_t ldsTable[snc::MAX_HASH_TABLE_SIZE];
    __shared__ Crc32cTables tables;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int32_t blockSize = p.blockSize;
    if (p.checksums != 0) {
        crc32c_tables_init(tables, lane);  // (all four wavefronts write the same values between the same barriers)
    }
    uint8_t* const slab = outSlabs + ((size_t)blockIdx.x * 4 + wave) * SLAB_BYTES;
    uint16_t* const tableSlab = tableSlabs + ((size_t)blockIdx.x * 3 + (wave > 0 ? wave - 1 : 0)) * snc::MAX_HASH_TABLE_SIZE;
    const int32_t total = L.counters[1];
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
        const int64_t pos = (int64_t)k * blockSize;
        const int32_t inLen = a.srcLen[stream];
        const int32_t length = (int32_t)(inLen - pos < blockSize ? inLen - pos : blockSize);
        const uint8_t* block = a.srcBase + a.srcOff[stream] + pos;
        uint8_t* out = a.dstBase + a.dstOff[stream] + (WINDOW ? head[stream] : 10) + (int64_t)k * worst_chunk(blockSize);
        const uint32_t crc = p.checksums != 0 ? crc32c_mask(wave_crc32c(tables, block, length, lane)) : 0u;  // writeCompressed :203
        int32_t cst = 0, compressed = 0;
        if (wave == 0) {
            snappy_compress_buffer_mw(ldsTable, block, length, slab, (int32_t)SLAB_BYTES, lane, cst, compressed);  // :206-211
        }
        else {
            snappy_compress_buffer_mw(tableSlab, block, length, slab, (int32_t)SLAB_BYTES, lane, cst, compressed);
        }
        wave_mem_order();
        const bool keep = ((double)compressed / (double)length) <= p.minRatio;  // :213
        const uint8_t* data = keep ? slab : block;
        const int32_t dlen = keep ? compressed : length;
        if (lane == 0) {  // writeBlock :241-254
            const uint32_t headerLength = (uint32_t)dlen + 4u;
            st4(out, (keep ? (uint32_t)COMPRESSED_DATA_FLAG : (uint32_t)UNCOMPRESSED_DATA_FLAG) | (headerLength << 8));
            st4(out + 4, crc);
            L.bSize[b] = 8 + dlen;
        }
        group_copy<64>(out + 8, data, dlen, lane);
        wave_mem_order();
    }
}

__global__ __launch_bounds__(256) void snappyframed_encode_kernel(BatchArgs a, BlockList L, WriterParams p, uint8_t* outSlabs, uint16_t* tableSlabs)
{
    encode_blocks<false>(a, L, p, outSlabs, tableSlabs, nullptr);
}

__global__ __launch_bounds__(256) void snappyframed_window_encode_kernel(BatchArgs a, BlockList L, WriterParams p, uint8_t* outSlabs, uint16_t* tableSlabs, const int32_t* head)
{
    encode_blocks<true>(a, L, p, outSlabs, tableSlabs, head);
}

template <bool WINDOW>
__device__ __forceinline__ void compact_streams(const BatchArgs& a, const BlockList& L, int32_t blockSize, const int32_t* head)
{
    const int lane = threadIdx.x;
    for (;;) {
        int32_t stream = 0;
        if (lane == 0) {
            stream = atomicAdd(L.counters + 3, 1);
        }
        stream = __builtin_amdgcn_readfirstlane(stream);
        if (stream >= a.nBlocks) {
            return;
        }
        if (L.sSerial[stream] != 0) {
            continue;
        }
        const int32_t st = L.sStatus[stream];
        int32_t o = 0;
        if (st == 0) {
            uint8_t* out = a.dstBase + a.dstOff[stream];
            const int32_t lead = WINDOW ? head[stream] : 10;
            if (lane == 0 && lead != 0) {  // constructor :94
                st8(out, 0x50614E73000006FFull);
                out[8] = 0x70;
                out[9] = 0x59;
            }
            o = lead;
            const int32_t first = L.sFirst[stream], n = L.sCount[stream];
            for (int32_t k = 0; k < n; k++) {
                const int32_t size = L.bSize[first + k];
                const int64_t from = lead + (int64_t)k * worst_chunk(blockSize);
                if (from != o) {
                    wave_mem_order();
                    group_copy<64>(out + o, out + from, size, lane);  // to the left; every lane loads before it stores
                    wave_mem_order();
                }
                o += size;
            }
        }
        if (lane == 0) {
            a.outLen[stream] = st == 0 ? o : 0;
            a.status[stream] = st;
            a.errOffset[stream] = 0;
        }
    }
}

__global__ __launch_bounds__(64) void snappyframed_compact_kernel(BatchArgs a, BlockList L, int32_t blockSize)
{
    compact_streams<false>(a, L, blockSize, nullptr);
}

__global__ __launch_bounds__(64) void snappyframed_window_compact_kernel(BatchArgs a, BlockList L, int32_t blockSize, const int32_t* head)
{
    compact_streams<true>(a, L, blockSize, head);
}

// The window form of the plan (achip_window_compress_batch): the stream identifier under ACHIP_WINDOW_FIRST, the full blocks the window holds and the
// destination has worst-case room for, the partial tail only under ACHIP_WINDOW_LAST; taken[] is what the encode kernel sees as the input's length.
// A window takes at most its share of the block list, capacity / windows blocks (at least one): with small blocks a call can hold more blocks than the list has
// entries, and such a window stops behind its share with NEED_ROOM, need 0 -- the caller's loop calls again, as for any other stop with progress.  Only a call of
// more windows than the list has entries still fails (ACHIP_D_UNSUPPORTED).
__global__ __launch_bounds__(64) void snappyframed_window_plan_kernel(BatchArgs a, BlockList L, WindowArgs w, int32_t blockSize, int32_t capacity, int32_t* taken, int32_t* head)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    const int32_t inLen = a.srcLen[stream], cap = a.dstCap[stream];
    const int32_t flags = w.flags[stream];
    int32_t st = 0, stop = ACHIP_STOP_END, lead = (flags & ACHIP_WINDOW_FIRST) != 0 ? 10 : 0;
    int64_t blocks = 0, consumed = 0, need = 0;
    if (inLen < 0 || cap < 0) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    else {
        const int64_t worst = worst_chunk(blockSize);
        const int64_t full = inLen / blockSize, rest = inLen % blockSize;
        const int64_t missing = cap < lead ? lead : 0;  // not even the stream identifier fits: nothing is written
        const int64_t room = cap < lead ? 0 : cap - lead;
        const int64_t share = capacity / a.nBlocks > 1 ? capacity / a.nBlocks : 1;
        blocks = full < room / worst ? full : room / worst;
        const bool listFull = blocks > share || (blocks == share && blocks == full && rest > 0 && (flags & ACHIP_WINDOW_LAST) != 0 && room - blocks * worst >= 8 + rest);
        blocks = blocks < share ? blocks : share;
        consumed = blocks * blockSize;
        if (listFull) {  // (there is input and room for more: the list's share is what ends the call)
            stop = ACHIP_STOP_NEED_ROOM;
            need = 0;
        }
        else if (blocks < full) {
            stop = ACHIP_STOP_NEED_ROOM;
            need = missing + worst;
        }
        else if (rest > 0 && (flags & ACHIP_WINDOW_LAST) == 0) {
            stop = missing != 0 ? ACHIP_STOP_NEED_ROOM : ACHIP_STOP_NEED_INPUT;
            need = missing != 0 ? missing : blockSize;
        }
        else if (rest > 0 && room - blocks * worst < 8 + rest) {
            stop = ACHIP_STOP_NEED_ROOM;
            need = missing + 8 + rest;
        }
        else if (rest > 0) {
            blocks++;
            consumed += rest;
        }
        else if (missing != 0) {
            stop = ACHIP_STOP_NEED_ROOM;
            need = missing;
        }
        if (missing != 0) {
            lead = 0;
        }
    }
    if (!lists::plan_entries(L, stream, st == 0 ? (int32_t)blocks : 0, capacity)) {  // (more windows in one call than the list has entries)
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_UNSUPPORTED);
    }
    L.sStatus[stream] = st;
    L.sSerial[stream] = 0;
    taken[stream] = st == 0 ? (int32_t)consumed : 0;
    head[stream] = lead;
    w.consumed[stream] = st == 0 ? consumed : 0;
    w.stop[stream] = st == 0 ? stop : ACHIP_STOP_FAILED;
    w.need[stream] = st == 0 ? need : 0;
}
}  // namespace snf

namespace {
constexpr int SNF_COMPRESS_WAVES = 256 * 3;    // one wavefront per stream: 44 KB of LDS each
constexpr int SNF_ENCODE_WORKGROUPS = 256 * 3; // four wavefronts around one LDS table + the CRC tables
// the writer's scratch: the counters, the serial kernel's slabs, the encode kernel's output and table slabs, the list
struct SnfWriterScratch {
    uint8_t* serialSlabs;
    uint8_t* outSlabs;
    uint16_t* tableSlabs;
    snf::BlockList L;
    void carve(lists::Carver& k, int64_t nStreams)
    {
        int32_t* counterWords = k.take<int32_t>(lists::COUNTER_WORDS);
        serialSlabs = k.take<uint8_t>((int64_t)SNF_COMPRESS_WAVES * snf::SLAB_BYTES);
        outSlabs = k.take<uint8_t>((int64_t)SNF_ENCODE_WORKGROUPS * 4 * snf::SLAB_BYTES);
        tableSlabs = k.take<uint16_t>((int64_t)SNF_ENCODE_WORKGROUPS * 3 * snc::MAX_HASH_TABLE_SIZE);
        L.carve(k, counterWords, nStreams, true);
    }
};
}  // namespace

int64_t snappyframed_compress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    SnfWriterScratch().carve(k, nStreams < 1 ? 1 : nStreams);
    return k.used();
}

namespace {
snf::WriterParams writer_params(const KernelSettings& ks)
{
    snf::WriterParams p;
    p.blockSize = ks.snfBlockSize;
    p.checksums = ks.snfWriteChecksums;
    p.minRatio = snf_ratio(ks.snfMinRatioBits);  // (the ratio crosses the C ABI as its bit pattern)
    return p;
}
int32_t list_entries(const KernelSettings& ks)
{
    return ks.snfListEntries > 0 && ks.snfListEntries < lists::CAPACITY ? ks.snfListEntries : lists::CAPACITY;
}
unsigned encode_grid(const KernelSettings& ks)
{
    return (unsigned)(ks.snfEncodeWorkgroups > 0 && ks.snfEncodeWorkgroups < SNF_ENCODE_WORKGROUPS ? ks.snfEncodeWorkgroups : SNF_ENCODE_WORKGROUPS);
}
}  // namespace

hipError_t launch_snappyframed_compress(const BatchArgs& a, hipStream_t stream, void* scratch, int variant, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    const snf::WriterParams p = writer_params(ks);
    lists::Carver k(scratch);
    SnfWriterScratch S;
    S.carve(k, a.nBlocks);
    const snf::BlockList& L = S.L;
    int32_t* counters = L.counters;
    hipError_t e = hipMemsetAsync(counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const unsigned serialGrid = (unsigned)(a.nBlocks < SNF_COMPRESS_WAVES ? a.nBlocks : SNF_COMPRESS_WAVES);
    if (variant == 0) {  // one wavefront per stream
        hipLaunchKernelGGL(snappyframed_compress_kernel, dim3(serialGrid), dim3(64), 0, stream, a, p, S.serialSlabs, counters + 32, (const int32_t*)nullptr);
        return hipGetLastError();
    }
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    const int32_t capacity = list_entries(ks);
    hipLaunchKernelGGL(snf::snappyframed_plan_kernel, dim3(perStream), dim3(64), 0, stream, a, L, p.blockSize, capacity);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, counters, capacity);
    hipLaunchKernelGGL(snf::snappyframed_encode_kernel, dim3(encode_grid(ks)), dim3(256), 0, stream, a, L, p, S.outSlabs, S.tableSlabs);
    hipLaunchKernelGGL(snf::snappyframed_compact_kernel, dim3((unsigned)(a.nBlocks < 2048 ? a.nBlocks : 2048)), dim3(64), 0, stream, a, L, p.blockSize);
    hipLaunchKernelGGL(snappyframed_compress_kernel, dim3(serialGrid), dim3(64), 0, stream, a, p, S.serialSlabs, counters + 32, (const int32_t*)L.sSerial);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Chunk-parallel reader (the default).  A stream's chunks are independent of each other except for where they start and
// where their plaintext goes, and both follow from the chunk headers alone (a compressed chunk announces its plaintext
// length in its preamble).  So:
//   walk    one LANE per stream runs the Java loop over the chunk headers only (same checks, same order, everything that
//           does not need the chunk's body) and writes one descriptor per data chunk -- source, destination, the capacity
//           the Java reader would hand its block decoder -- into a batch assembled on the device;
//   decode  that batch goes through the batched Snappy block decoders (rings / lane-per-block, chosen on the device as for
//           any other batch): a 64 KiB chunk is exactly the unit those kernels are built for;
//   verify  one wavefront per chunk copies a stored chunk or takes the decoded one and checks the masked CRC-32C;
//   fold    one lane per stream looks at its chunks in stream order: the first chunk that failed (block codec error before
//           checksum error) gives the stream's status, else the error the walk stopped at, else the length.
// A stream whose chunks do not fit into the descriptor arrays is left to the one-wavefront-per-stream kernel below.
namespace snf {
using lists::CAPACITY;

struct ChunkList : lists::ChunkBatch {  // per chunk: a batch for the block decoders (counters [2]: verify cursor, [16..]: probe statistics, [32]: serial cursor) ...
    // ... and what the verify / fold steps need
    uint32_t* cCrc;
    int32_t* cRawLen;   // >= 0: a stored chunk of this many bytes (the decoders see an empty input and are overruled); -1: compressed
    int32_t* cPos;      // position of the chunk header in its stream
    // per stream
    int32_t* sFirst;
    int32_t* sCount;
    int32_t* sStatus;   // what the walk stopped at (0: end of stream)
    int64_t* sErrOff;
    int32_t* sOut;      // plaintext bytes if every chunk decodes
    int32_t* sSerial;   // 1: handled by the serial kernel
    void carve(lists::Carver& k, int64_t nStreams)
    {
        int32_t* counterWords = k.take<int32_t>(lists::COUNTER_WORDS);
        sErrOff = k.take<int64_t>(nStreams);
        sFirst = k.take<int32_t>(nStreams);
        sCount = k.take<int32_t>(nStreams);
        sStatus = k.take<int32_t>(nStreams);
        sOut = k.take<int32_t>(nStreams);
        sSerial = k.take<int32_t>(nStreams);
        ChunkBatch::carve(k, counterWords);
        cCrc = k.take<uint32_t>(CAPACITY);
        cRawLen = k.take<int32_t>(CAPACITY);
        cPos = k.take<int32_t>(CAPACITY);
    }
};

__device__ __forceinline__ uint32_t rd_bytes(const uint8_t* p, int n)  // little-endian, n <= 4 (cold: byte loads)
{
    uint32_t v = 0;
    for (int i = 0; i < n; i++) {
        v |= (uint32_t)p[i] << (8 * i);
    }
    return v;
}

// A window's walk (achip_window_decompress_batch): what it may list, where it stopped and why.
struct WindowWalk {
    bool first, last;    // ACHIP_WINDOW_FIRST: the stream identifier leads the window; _LAST: an incomplete tail is the reader's truncation error, not a stop
    int32_t maxChunks;   // the list has room for this many
    int32_t pos;         // out: the end of the chunks walked
    int32_t stop;        // out: ACHIP_STOP_*
    int64_t need;
};

// The Java loop over one stream without the chunk bodies.  FILL = false: count the data chunks; true: write their descriptors.
// WINDOW: the stream is a window that begins at a chunk.  The walk stops in front of the first chunk that is not whole or does not fit and says so in `w`; a chunk
// the reader refuses is reported with its offset in the window, and the reader is a fresh one at every chunk (its buffers do not remember the chunks before).
template <bool FILL, bool WINDOW = false>
__device__ void walk_stream(const BatchArgs& a, const ChunkList& L, int32_t stream, int32_t first, int32_t& countOut, int32_t& stOut, int64_t& eoOut, int32_t& outOut,
                            WindowWalk* w = nullptr)
{
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[stream];
    const int32_t inLen = a.srcLen[stream];
    const int32_t outCap = a.dstCap[stream];
    countOut = 0;
    outOut = 0;
    stOut = 0;
    eoOut = 0;
    // the walk ends in front of the chunk at `at`: with a status (offset `off`), or -- a window -- with a stop
#define WALK_END(at, why, want, st, off)    \
    {                                       \
        stOut = (st);                       \
        eoOut = (int64_t)(off);             \
        outOut = o;                         \
        countOut = n;                       \
        if (WINDOW) {                       \
            w->pos = (at);                  \
            w->stop = (why);                \
            w->need = (want);               \
        }                                   \
        return;                             \
    }
#define WALK_FAIL(detail, off) WALK_END(off, ACHIP_STOP_FAILED, 0, mk_status(ACHIP_CLASS_MALFORMED, detail), off)
    int32_t o = 0;
    int32_t n = 0;
    int32_t pos = 0;
    if (!WINDOW || w->first) {
        if (WINDOW && inLen < 10 && !w->last) WALK_END(0, ACHIP_STOP_NEED_INPUT, 10, 0, 0);
        if (inLen < 10) WALK_FAIL(ACHIP_D_SNF_EOF_STREAM_HEADER, 0);
        if (rd_bytes(in, 4) != 0x000006FFu || rd_bytes(in + 4, 4) != 0x50614E73u || in[8] != 0x70 || in[9] != 0x59) WALK_FAIL(ACHIP_D_SNF_BAD_STREAM_HEADER, 0);
        pos = 10;
    }
    int32_t javaInput = MAX_BLOCK_SIZE + 5, javaUncompressed = MAX_BLOCK_SIZE + 5;
    for (;;) {
        const int32_t chunk = pos;
        if (pos == inLen) {
            break;
        }
        if (WINDOW) {
            if (n >= w->maxChunks) WALK_END(chunk, ACHIP_STOP_NEED_ROOM, 0, 0, 0);
            if (inLen - pos < 4 && !w->last) WALK_END(chunk, ACHIP_STOP_NEED_INPUT, 0, 0, 0);
            javaInput = MAX_BLOCK_SIZE + 5;
            javaUncompressed = MAX_BLOCK_SIZE + 5;
        }
        if (inLen - pos < 4) WALK_FAIL(ACHIP_D_SNF_EOF_BLOCK_HEADER, chunk);
        const uint32_t header = rd_bytes(in + pos, 4);
        const int flag = (int)(header & 0xFF);
        const int32_t length = (int32_t)(header >> 8);
        pos += 4;
        if (WINDOW && length > inLen - pos && !w->last) WALK_END(chunk, ACHIP_STOP_NEED_INPUT, (int64_t)length + 4, 0, 0);
        bool skip = false;
        int32_t minLength;
        if (flag == COMPRESSED_DATA_FLAG || flag == UNCOMPRESSED_DATA_FLAG) {
            minLength = 5;
        }
        else if (flag == STREAM_IDENTIFIER_FLAG) {
            if (length != 6) WALK_FAIL(ACHIP_D_SNF_STREAM_ID_LENGTH, chunk);
            skip = true;
            minLength = 6;
        }
        else {
            if (flag <= 0x7f) WALK_FAIL(ACHIP_D_SNF_UNSKIPPABLE, chunk);
            skip = true;
            minLength = 0;
        }
        if (length < minLength) WALK_FAIL(ACHIP_D_SNF_INVALID_LENGTH, chunk);
        if (skip) {
            pos += length < inLen - pos ? length : inLen - pos;
            continue;
        }
        if (length > javaInput) {
            javaInput = length;
            javaUncompressed = javaUncompressed < length ? length : javaUncompressed;
        }
        if (inLen - pos < length) WALK_FAIL(ACHIP_D_SNF_EOF_FRAME, chunk);
        const uint32_t stored = rd_bytes(in + pos, 4);
        const int32_t dlen = length - 4;
        int32_t produced, limit, rawLen;
        if (flag == COMPRESSED_DATA_FLAG) {
            int32_t ulen = 0, beo = 0, preamble = 0;
            const int32_t pst = snappy_read_uncompressed_length(in + pos + 4, dlen, ulen, preamble, beo);
            if (pst != 0) WALK_END(chunk, ACHIP_STOP_FAILED, 0, pst, WINDOW ? chunk + beo : beo);  // the block codec's own exception, before any byte is decoded
            javaUncompressed = javaUncompressed < ulen ? ulen : javaUncompressed;
            if (ulen > outCap - o) WALK_END(chunk, ACHIP_STOP_NEED_ROOM, ulen, WINDOW ? 0 : mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_SNF_OUTPUT_TOO_SMALL), chunk);
            limit = javaUncompressed < outCap - o ? javaUncompressed : outCap - o;
            produced = ulen;
            rawLen = -1;
        }
        else {
            if (dlen > outCap - o) WALK_END(chunk, ACHIP_STOP_NEED_ROOM, dlen, WINDOW ? 0 : mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_SNF_OUTPUT_TOO_SMALL), chunk);
            limit = 0;
            produced = dlen;
            rawLen = dlen;
        }
        if (FILL) {
            const int32_t c = first + n;
            L.cSrcOff[c] = a.srcOff[stream] + pos + 4;
            L.cSrcLen[c] = rawLen >= 0 ? 0 : dlen;
            L.cDstOff[c] = a.dstOff[stream] + o;
            L.cDstCap[c] = limit;
            L.cCrc[c] = stored;
            L.cRawLen[c] = rawLen;
            L.cPos[c] = chunk;
        }
        n++;
        o += produced;
        pos += length;
    }
#undef WALK_FAIL
#undef WALK_END
    if (WINDOW) {
        w->pos = pos;
        w->stop = ACHIP_STOP_END;
        w->need = 0;
    }
    countOut = n;
    outOut = o;
}

__global__ __launch_bounds__(64) void snappyframed_walk_kernel(BatchArgs a, ChunkList L)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    int32_t n = 0, st = 0, out = 0;
    int64_t eo = 0;
    walk_stream<false>(a, L, stream, 0, n, st, eo, out);
    const int32_t first = n > 0 ? atomicAdd(L.counters, n) : 0;
    const bool fits = (int64_t)first + n <= CAPACITY;
    L.sFirst[stream] = first;
    L.sCount[stream] = fits ? n : 0;
    L.sStatus[stream] = st;
    L.sErrOff[stream] = eo;
    L.sOut[stream] = out;
    L.sSerial[stream] = fits ? 0 : 1;
    if (fits && n > 0) {
        walk_stream<true>(a, L, stream, first, n, st, eo, out);
    }
    else if (!fits) {  // the part of this stream's range that lies inside the arrays: empty blocks nobody looks at
        for (int64_t c = first; c < (int64_t)first + n && c < CAPACITY; c++) {
            L.cSrcOff[c] = 0;
            L.cSrcLen[c] = 0;
            L.cDstOff[c] = 0;
            L.cDstCap[c] = 0;
            L.cCrc[c] = 0;
            L.cRawLen[c] = -1;
            L.cPos[c] = 0;
        }
    }
}

// VERIFY = false (verifyChecksums off): what is left of the step is the copy of the stored chunks
template <bool VERIFY>
__device__ __forceinline__ void verify_chunks(const BatchArgs& a, const ChunkList& L)
{
    __shared__ Crc32cTables tables;
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    if constexpr (VERIFY) {
        crc32c_tables_init(tables, lane);
    }
    const int32_t total = L.counters[1];
    for (;;) {
        __syncthreads();
        if (lane == 0) {
            item = atomicAdd(L.counters + 2, 1);
        }
        __syncthreads();
        const int32_t c = item;
        if (c >= total) {
            return;
        }
        const int32_t rawLen = L.cRawLen[c];
        uint8_t* dst = a.dstBase + L.cDstOff[c];
        int32_t produced;
        if (rawLen >= 0) {
            group_copy<64>(dst, a.srcBase + L.cSrcOff[c], rawLen, lane);
            wave_sync();  // (the checksum below reads what the other lanes copied)
            produced = rawLen;
        }
        else {
            if (!VERIFY || L.cStatus[c] != 0) {
                continue;  // the block decoder's verdict stands
            }
            produced = L.cOutLen[c];
        }
        bool ok = true;
        if constexpr (VERIFY) {
            ok = L.cCrc[c] == crc32c_mask(wave_crc32c(tables, dst, produced, lane));
        }
        if (lane == 0) {
            L.cStatus[c] = ok ? 0 : mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_SNF_CHECKSUM);
            L.cErrOff[c] = ok ? 0 : (int64_t)L.cPos[c];
        }
    }
}

__global__ __launch_bounds__(64) void snappyframed_verify_kernel(BatchArgs a, ChunkList L)
{
    verify_chunks<true>(a, L);
}

__global__ __launch_bounds__(64) void snappyframed_stored_kernel(BatchArgs a, ChunkList L)
{
    verify_chunks<false>(a, L);
}

__global__ __launch_bounds__(64) void snappyframed_fold_kernel(BatchArgs a, ChunkList L)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks || L.sSerial[stream] != 0) {
        return;
    }
    int32_t st = L.sStatus[stream];
    int64_t eo = L.sErrOff[stream];
    const int32_t first = L.sFirst[stream], n = L.sCount[stream];
    for (int32_t k = 0; k < n; k++) {
        const int32_t cs = L.cStatus[first + k];
        if (cs != 0) {
            st = cs;
            eo = L.cErrOff[first + k];
            break;
        }
    }
    a.outLen[stream] = st == 0 ? L.sOut[stream] : 0;
    a.status[stream] = st;
    a.errOffset[stream] = st == 0 ? 0 : eo;
}
// ---- the window forms of walk and fold (achip_window_decompress_batch) ----
struct WindowList : ChunkList {
    int32_t* sPos;   // per window: where the walk stopped ...
    int32_t* sStop;  // ... and why
    int64_t* sNeed;
    void carve(lists::Carver& k, int64_t nStreams)
    {
        ChunkList::carve(k, nStreams);
        sNeed = k.take<int64_t>(nStreams);
        sPos = k.take<int32_t>(nStreams);
        sStop = k.take<int32_t>(nStreams);
    }
};

// a lane per window: every chunk header the window holds; the data chunks that are whole and fit go on the list -- as many as the list has room for
__global__ __launch_bounds__(64) void snappyframed_window_walk_kernel(BatchArgs a, WindowList L, WindowArgs w)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    int32_t n = 0, st = 0, out = 0, first = 0;
    int64_t eo = 0;
    WindowWalk ww;
    ww.first = (w.flags[stream] & ACHIP_WINDOW_FIRST) != 0;
    ww.last = (w.flags[stream] & ACHIP_WINDOW_LAST) != 0;
    ww.maxChunks = 0x7FFFFFFF;
    ww.pos = 0;
    ww.stop = ACHIP_STOP_FAILED;
    ww.need = 0;
    if (a.srcLen[stream] < 0 || a.dstCap[stream] < 0) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
    }
    else {
        walk_stream<false, true>(a, L, stream, 0, n, st, eo, out, &ww);
        first = n > 0 ? atomicAdd(L.counters, n) : 0;
        if ((int64_t)first + n > CAPACITY) {  // the list takes what fits
            ww.maxChunks = first < CAPACITY ? CAPACITY - first : 0;
            walk_stream<false, true>(a, L, stream, 0, n, st, eo, out, &ww);
        }
        if (n > 0) {
            walk_stream<true, true>(a, L, stream, first, n, st, eo, out, &ww);
        }
    }
    L.sFirst[stream] = first;
    L.sCount[stream] = n;
    L.sStatus[stream] = st;
    L.sErrOff[stream] = eo;
    L.sOut[stream] = out;
    L.sSerial[stream] = 0;
    L.sPos[stream] = ww.pos;
    L.sStop[stream] = ww.stop;
    L.sNeed[stream] = ww.need;
}

// a lane per window: everything in front of the first chunk that failed (block codec error before checksum error) is delivered; behind the last chunk the
// walk's stop or status stands
__global__ __launch_bounds__(64) void snappyframed_window_fold_kernel(BatchArgs a, WindowList L, WindowArgs w)
{
    const int32_t stream = blockIdx.x * 64 + threadIdx.x;
    if (stream >= a.nBlocks) {
        return;
    }
    const int32_t first = L.sFirst[stream], n = L.sCount[stream];
    for (int32_t k = 0; k < n; k++) {
        const int32_t cs = L.cStatus[first + k];
        if (cs != 0) {
            const int64_t at = L.cPos[first + k];  // (a checksum error reports the chunk, a block codec error its own offset: here behind the chunk's position)
            const int64_t eo = cs == mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_SNF_CHECKSUM) ? at : at + L.cErrOff[first + k];
            win::report(a, w, stream, at, (int32_t)(L.cDstOff[first + k] - a.dstOff[stream]), ACHIP_STOP_FAILED, 0, cs, eo);
            return;
        }
    }
    win::report(a, w, stream, L.sPos[stream], L.sOut[stream], L.sStop[stream], L.sNeed[stream], L.sStatus[stream], L.sErrOff[stream]);
}
}  // namespace snf

int64_t snappyframed_decompress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    snf::ChunkList().carve(k, nStreams < 1 ? 1 : nStreams);
    return k.used();
}

// variant 0: a wavefront per stream.  The others list the chunks and hand them to launch_listed_decode (achip_launch.h): 1, or no `aux`: without a
// synchronisation; 2: always through the two-pass decoder -- the host reads the chunk count back (one synchronisation) and asks `aux`
// for the record arena; 3 (the default): the element-length probe of the block API's auto mode decides between the two.  A chunk holds at most
// 64 KiB: the block codec's arena per block.
hipError_t launch_snappyframed_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, int variant, const AuxScratch* aux, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    snf::ChunkList L;
    L.carve(k, a.nBlocks);
    int32_t* counters = L.counters;
    hipError_t e = hipMemsetAsync(counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const int32_t maxWaves = 256 * 8;
    const bool verify = ks.snfVerifyChecksums != 0;
    const auto serial = verify ? snappyframed_decompress_kernel : snappyframed_decompress_noverify_kernel;
    if (variant == 0) {  // one wavefront per stream
        const unsigned grid = (unsigned)(a.nBlocks < maxWaves ? a.nBlocks : maxWaves);
        hipLaunchKernelGGL(serial, dim3(grid), dim3(64), 0, stream, a, counters + 32, (const int32_t*)nullptr);
        return hipGetLastError();
    }
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    hipLaunchKernelGGL(snf::snappyframed_walk_kernel, dim3(perStream), dim3(64), 0, stream, a, L);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, counters, lists::CAPACITY);
    const bool sync = (variant == 2 || variant == 3) && aux != nullptr && aux->get != nullptr;
    const ListedWant want{sync, variant == 3, true, 1, -1};
    bool decoded = false;
    e = launch_listed_decode(L.as_batch(a, lists::CAPACITY), 1, stream, counters, counters + 16, aux, ks, want, &decoded);
    if (e != hipSuccess) return e;
    const auto check = verify ? snf::snappyframed_verify_kernel : snf::snappyframed_stored_kernel;  // verify off: no CRC pass, the stored chunks' copy alone
    hipLaunchKernelGGL(check, dim3(maxWaves), dim3(64), 0, stream, a, L);
    hipLaunchKernelGGL(snf::snappyframed_fold_kernel, dim3(perStream), dim3(64), 0, stream, a, L);
    // streams that did not fit into the lists
    {
        const unsigned grid = (unsigned)(a.nBlocks < maxWaves ? a.nBlocks : maxWaves);
        hipLaunchKernelGGL(serial, dim3(grid), dim3(64), 0, stream, a, counters + 32, (const int32_t*)L.sSerial);
    }
    return hipGetLastError();
}

// ---- windows (achip_window_decompress_batch / _compress_batch) ----
int64_t snappyframed_window_decompress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    snf::WindowList().carve(k, nStreams < 1 ? 1 : nStreams);
    return k.used();
}

// walk -> seal -> the listed chunks through the Snappy block decoders (as the one-shot reader's variants 1 .. 3) -> verify -> fold.  Every verdict over a
// window follows from its chunk headers and its chunks' decodes: no wavefront-per-stream kernel behind the fold.
hipError_t launch_snappyframed_window_decompress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, int variant, const AuxScratch* aux, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    lists::Carver k(scratch);
    snf::WindowList L;
    L.carve(k, a.nBlocks);
    int32_t* counters = L.counters;
    hipError_t e = hipMemsetAsync(counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    const int32_t maxWaves = 256 * 8;
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    hipLaunchKernelGGL(snf::snappyframed_window_walk_kernel, dim3(perStream), dim3(64), 0, stream, a, L, w);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, counters, lists::CAPACITY);
    const bool sync = (variant == 2 || variant == 3) && aux != nullptr && aux->get != nullptr;
    const ListedWant want{sync, variant == 3, true, 1, -1};
    bool decoded = false;
    e = launch_listed_decode(L.as_batch(a, lists::CAPACITY), 1, stream, counters, counters + 16, aux, ks, want, &decoded);
    if (e != hipSuccess) return e;
    const auto check = ks.snfVerifyChecksums != 0 ? snf::snappyframed_verify_kernel : snf::snappyframed_stored_kernel;
    hipLaunchKernelGGL(check, dim3(maxWaves), dim3(64), 0, stream, a, (const snf::ChunkList&)L);
    hipLaunchKernelGGL(snf::snappyframed_window_fold_kernel, dim3(perStream), dim3(64), 0, stream, a, L, w);
    return hipGetLastError();
}

namespace {
struct SnfWindowWriterScratch : SnfWriterScratch {
    int32_t* taken;
    int32_t* head;
    void carve(lists::Carver& k, int64_t nStreams)
    {
        SnfWriterScratch::carve(k, nStreams);
        taken = k.take<int32_t>(nStreams);
        head = k.take<int32_t>(nStreams);
    }
};
}  // namespace

int64_t snappyframed_window_compress_scratch_bytes(int32_t nStreams)
{
    lists::Carver k(nullptr);
    SnfWindowWriterScratch().carve(k, nStreams < 1 ? 1 : nStreams);
    return k.used();
}

// the window plan, then the block-parallel writer's encode and compact over what the plan took
hipError_t launch_snappyframed_window_compress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, const KernelSettings& ks)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    const snf::WriterParams p = writer_params(ks);
    const int32_t capacity = list_entries(ks);
    lists::Carver k(scratch);
    SnfWindowWriterScratch S;
    S.carve(k, a.nBlocks);
    const snf::BlockList& L = S.L;
    hipError_t e = hipMemsetAsync(L.counters, 0, 4096, stream);
    if (e != hipSuccess) return e;
    BatchArgs t = a;
    t.srcLen = S.taken;
    const unsigned perStream = (unsigned)((a.nBlocks + 63) / 64);
    hipLaunchKernelGGL(snf::snappyframed_window_plan_kernel, dim3(perStream), dim3(64), 0, stream, a, L, w, p.blockSize, capacity, S.taken, S.head);
    hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, capacity);
    hipLaunchKernelGGL(snf::snappyframed_window_encode_kernel, dim3(encode_grid(ks)), dim3(256), 0, stream, t, L, p, S.outSlabs, S.tableSlabs, (const int32_t*)S.head);
    hipLaunchKernelGGL(snf::snappyframed_window_compact_kernel, dim3((unsigned)(a.nBlocks < 2048 ? a.nBlocks : 2048)), dim3(64), 0, stream, t, L, p.blockSize, (const int32_t*)S.head);
    hipLaunchKernelGGL(win::writer_verdict_kernel, dim3(perStream), dim3(64), 0, stream, a, w);
    return hipGetLastError();
}

}  // namespace achip
