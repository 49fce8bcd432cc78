// lzo_compress.hip -- batched LZO1X block encode for gfx950, byte-identical with the Java encoder (M/lzo/LzoRawCompressor.java:70-390).
//
// LzoRawCompressor.compress is the LZ4 Java encoder's search loop with another emit stage: the same 5-byte multiplicative hash, computeTableSize, skip schedule,
// catch-up, `input - 2` insert and re-probe, and `count`; MAX_DISTANCE is 49151 and the commands are LZO's.  So the search is the LZ4 encoder's own code
// (lz4_compress_body.h: lz4_table_init, lz4_probe_step with MAXD = 49151, lz4_catch_up_mem, wave_count) and this file holds what differs: the prologue's
// statuses and the emit stage (the batch loop itself is lz4_batch_search.h, included by both encoders).  A wavefront per block, the blocks of a launch dealt round over a grid the chip holds at once; the
// 4 096-entry table (32-bit entries: blocks of any length) in LDS.
#include "lz4_compress_body.h"
#include "achip_bounds.h"
#include "achip_launch.h"

namespace achip {

namespace lzoc {
constexpr int MAX_DISTANCE = 0xC000 - 1;  // :45
constexpr int MAX_INPUT_SIZE = 0x7E000000;  // :29
}  // namespace lzoc

// [command][zeros zero bytes][last]: the shape of every extended length (:293-302, :366-377); the lanes share the zeros.  Returns the position behind it.
__device__ __forceinline__ int32_t lzo_put_extended(uint8_t* out, int32_t o, uint32_t command, int32_t zeros, int32_t last, int lane)
{
    if (lane == 0) {
        out[o] = (uint8_t)command;
        out[o + 1 + zeros] = (uint8_t)last;
    }
    for (int32_t i = lane; i < zeros; i += 64) {
        out[o + 1 + i] = 0;
    }
    return o + 2 + zeros;
}

// encodeLiteralLength :278-309; returns the position behind the length (a count below 4 goes into the previous command's trailer, two bytes back)
__device__ __forceinline__ int32_t lzo_put_literal_length(uint8_t* out, int32_t o, bool firstLiteral, int32_t length, int lane)
{
    if (firstLiteral && length < 0xFF - 17) {
        if (lane == 0) {
            out[o] = (uint8_t)(length + 17);
        }
        return o + 1;
    }
    if (length < 4) {
        if (lane == 0) {
            out[o - 2] = (uint8_t)(out[o - 2] | length);
        }
        return o;
    }
    length -= 3;
    if (length > 15) {
        const int32_t remaining = length - 15;  // (>= 1)
        const int32_t zeros = (remaining - 1) / 255;
        return lzo_put_extended(out, o, 0, zeros, remaining - 255 * zeros, lane);
    }
    if (lane == 0) {
        out[o] = (uint8_t)length;
    }
    return o + 1;
}

// emitCopy :311-352 with encodeMatchLength :360-380 and encodeOffset :354-358 (1 <= matchOffset <= MAX_DISTANCE: the probe step accepts no other)
__device__ __forceinline__ int32_t lzo_put_copy(uint8_t* out, int32_t o, int32_t matchOffset, int32_t matchLength, int lane)
{
    if (matchLength <= 8 && matchOffset <= 2048) {  // 0bMMMP_PPLL 0bPPPP_PPPP
        matchLength--;
        matchOffset--;
        if (lane == 0) {
            out[o] = (uint8_t)((matchLength << 5) | ((matchOffset & 7) << 2));
            out[o + 1] = (uint8_t)(matchOffset >> 3);
        }
        return o + 2;
    }
    matchLength -= 2;
    int32_t base = 7;
    uint32_t command = 0x18;          // 0b0001_1MMM: offsets from 32768
    if (matchOffset < (1 << 15)) {
        command = 0x10;               // 0b0001_0MMM: 16385 .. 32767
        if (matchOffset <= (1 << 14)) {
            command = 0x20;           // 0b001M_MMMM: this command encodes matchOffset - 1
            base = 31;
            matchOffset--;
        }
    }
    if (matchLength <= base) {
        if (lane == 0) {
            out[o] = (uint8_t)(command | (uint32_t)matchLength);
        }
        o++;
    }
    else {
        int32_t remaining = matchLength - base;  // (>= 1)
        const int32_t pairs = (remaining - 1) / 510;
        remaining -= 510 * pairs;
        const int32_t one = remaining > 255 ? 1 : 0;
        o = lzo_put_extended(out, o, command, 2 * pairs + one, remaining - 255 * one, lane);
    }
    if (lane == 0) {
        out[o] = (uint8_t)((uint32_t)matchOffset << 2);
        out[o + 1] = (uint8_t)((uint32_t)matchOffset >> 6);
    }
    return o + 2;
}

// emitLastLiteral :236-255
__device__ __forceinline__ int32_t lzo_put_last_literals(const uint8_t* in, uint8_t* out, int32_t o, bool firstLiteral, int32_t anchor, int32_t inputLimit, int lane)
{
    const int32_t length = inputLimit - anchor;
    o = lzo_put_literal_length(out, o, firstLiteral, length, lane);
    group_copy<64>(out + o, in + anchor, length, lane);
    o += length;
    if (lane == 0) {  // the stop command: 0b0001_HMMM with a zero offset
        out[o] = 0x11;
        out[o + 1] = 0;
        out[o + 2] = 0;
    }
    return o + 3;
}

// the statuses of :84-90 -- in the reference's order: the output bound is checked before "nothing compresses to nothing"
__device__ __forceinline__ int32_t lzo_block_status(int32_t inLen, int32_t outCap)
{
    if ((uint32_t)inLen > (uint32_t)lzoc::MAX_INPUT_SIZE) {
        return mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_LZO_MAX_INPUT);
    }
    if ((int64_t)outCap < bound::lzo(inLen)) {
        return mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_LZO_MAX_OUTPUT);
    }
    return 0;
}

// One block by one wavefront: the batch loop of lz4_compress_block -- its own text, lz4_batch_search.h: the 64 lanes evaluate the next 64 steps of the search loop
// :127-146 at once -- around the LZO emit stage.
__device__ int32_t lzo_compress_block(const uint8_t* __restrict__ in, int32_t inLen, uint8_t* out, int32_t* table, int lane)
{
    using namespace lz4c;  // (the search's constants are the LZ4 encoder's: :26-47 restate them value for value, MAX_DISTANCE apart)
    if (inLen == 0) {  // :93-95
        return 0;
    }
    int32_t output = 0;
    int32_t anchor = 0;
    bool firstLiteral = true;
    if (inLen >= MIN_LENGTH) {  // :104
        const int32_t tableSize = lz4_table_init(inLen, table, lane);
        __syncthreads();
        const int32_t mask = tableSize - 1;
        const int hashBits = 32 - __builtin_clz((uint32_t)mask | 1u);
        const int32_t matchFindLimit = inLen - MATCH_FIND_LIMIT;
        const int32_t matchLimit = inLen - LAST_LITERAL_SIZE;
        const int32_t accel = 1;  // (LzoRawCompressor has no acceleration parameter)
#define BATCH_SEARCH_PROBE(role, pos, k) lz4_probe_step<int32_t, false, lzoc::MAX_DISTANCE>(in, table, mask, hashBits, matchFindLimit, scanStart, accel, role, pos, k, lane)
#define BATCH_SEARCH_EMIT_STATE
#define BATCH_SEARCH_EMIT_LITERALS /* emitLiteral :257-276 */                                      \
    const int32_t literalLength = input - anchor;                                                  \
    output = lzo_put_literal_length(out, output, firstLiteral, literalLength, lane);               \
    group_copy<64>(out + output, in + anchor, literalLength, lane);                                \
    output += literalLength;                                                                       \
    firstLiteral = false;
#define BATCH_SEARCH_EMIT_NO_LITERALS /* :192 another match, no literal run: nothing goes into the previous command's trailer */
#define BATCH_SEARCH_EMIT_MATCH output = lzo_put_copy(out, output, input - matchIndex, matchLength + MIN_MATCH, lane); /* :169 */
#include "lz4_batch_search.h"
#undef BATCH_SEARCH_PROBE
#undef BATCH_SEARCH_EMIT_STATE
#undef BATCH_SEARCH_EMIT_LITERALS
#undef BATCH_SEARCH_EMIT_NO_LITERALS
#undef BATCH_SEARCH_EMIT_MATCH
    }
    return lzo_put_last_literals(in, out, output, firstLiteral, anchor, inLen, lane);  // :105, :135, :198
}

__global__ __launch_bounds__(64) void lzo_compress_kernel(BatchArgs a)
{
    __shared__ int32_t table[lz4c::MAX_TABLE_SIZE];
    const int lane = threadIdx.x;
    for (int64_t block = blockIdx.x; block < a.nBlocks; block += gridDim.x) {  // (uniform)
        const int32_t inLen = uni(a.srcLen[block]);
        const int32_t st = lzo_block_status(inLen, uni(a.dstCap[block]));
        int32_t output = 0;
        if (st == 0) {
            output = lzo_compress_block(a.srcBase + a.srcOff[block], inLen, a.dstBase + a.dstOff[block], table, lane);
        }
        if (lane == 0) {
            a.outLen[block] = output;
            a.status[block] = st;
            a.errOffset[block] = 0;
        }
        wave_sync();  // (the table is the next block's)
    }
}

hipError_t launch_lzo_compress(const BatchArgs& a, hipStream_t stream)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    // 16 KiB of LDS a wavefront: ten a CU, 2 560 on the chip
    hipLaunchKernelGGL(lzo_compress_kernel, dim3((unsigned)(a.nBlocks < 2560 ? a.nBlocks : 2560)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace achip
