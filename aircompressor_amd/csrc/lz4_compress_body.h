// lz4_compress_body.h -- the LZ4 block encoder of one wavefront (lz4_compress.hip has the design notes): constants, token / run-length
// helpers, the pieces every form of the encoder is made of (prologue, catch-up, emitMatch, emitLastLiteral, the batch-probe step) and
// lz4_compress_block.  Shared by the batched block encoder, the LZ4 frame writer (lz4_compress.hip) and the Hadoop block-stream
// writer (hadoop_streams.hip).
#pragma once
#include "achip_enc_wave.h"

namespace achip {

namespace lz4c {
constexpr int HASH_LOG = 12;
constexpr int MAX_TABLE_SIZE = 1 << HASH_LOG;
constexpr int MIN_TABLE_SIZE = 16;
constexpr int MIN_MATCH = 4;
constexpr int LAST_LITERAL_SIZE = 5;
constexpr int MATCH_FIND_LIMIT = 12;
constexpr int MIN_LENGTH = 13;
constexpr int ML_MASK = 15;
constexpr int RUN_MASK = 15;
constexpr int MAX_DISTANCE = 65535;
constexpr int SKIP_TRIGGER = 6;
}  // namespace lz4c

__device__ __forceinline__ int32_t lz4_hash(uint64_t v, int32_t mask)  // :50-62
{
    return (int32_t)(((v * 889523592379ULL) >> 28) & (uint64_t)(uint32_t)mask);
}

// encodeRunLength :282-302 ; lane 0 writes, all lanes return the new offset
__device__ __forceinline__ int32_t lz4_run_length_size(int32_t length)
{
    return length >= lz4c::RUN_MASK ? 2 + (length - lz4c::RUN_MASK) / 255 : 1;
}

__device__ __forceinline__ void lz4_write_run_length(uint8_t* out, int32_t o, int32_t length, uint32_t tokenLow)
{
    if (length >= lz4c::RUN_MASK) {
        out[o++] = (uint8_t)((lz4c::RUN_MASK << 4) | tokenLow);
        int32_t remaining = length - lz4c::RUN_MASK;
        while (remaining >= 255) {
            out[o++] = 255;
            remaining -= 255;
        }
        out[o++] = (uint8_t)remaining;
    }
    else {
        out[o++] = (uint8_t)((length << 4) | tokenLow);
    }
}

// sum of the first m probe advances of one search (:113-125): adv(0) = 1, adv(k) = (63 + k) >> 6 for k >= 1
__device__ __forceinline__ int32_t lz4_scan_offset(int32_t m)
{
    if (m <= 65) {
        return m;
    }
    const int32_t n = 62 + m;
    const int32_t q = n >> 6, r = n & 63;
    return 1 + 32 * q * (q - 1) + q * (r + 1);
}
__device__ __forceinline__ int32_t lz4_scan_advance(int32_t k) { return k == 0 ? 1 : (63 + k) >> 6; }

// ---- acceleration (Lz4Compressor.create(int), M/lz4/Lz4Compressor.java:33-41) ----
// :115 with `acceleration << SKIP_TRIGGER` for `1 << SKIP_TRIGGER`, liblz4's rule: adv(0) = 1, adv(k) = (64a + k - 1) >> 6 = a + ((k - 1) >> 6) for k >= 1, which
// is the schedule above with a - 1 more per advance from the second probe on.  The encoders take it as a compile-time form (ACCEL) with the value as an
// argument: the ACCEL = false instantiations are the kernels as they were.
// In 32 bits: a batch's first probe lies at most at matchFindLimit (the probe before it was valid), its other 63 lanes at most 63 advances behind it, an
// advance is at most 65537 + 2^31 / 64 / 65537 + 1 -- 0x7E000000 + 64 * 66000 < 2^31.
__device__ __forceinline__ int32_t lz4_scan_offset(int32_t m, int32_t a) { return m == 0 ? 0 : lz4_scan_offset(m) + (m - 1) * (a - 1); }
__device__ __forceinline__ int32_t lz4_scan_advance(int32_t k, int32_t a) { return k == 0 ? 1 : ((63 + k) >> 6) + (a - 1); }
// the probes of one search as a mask of the 64 positions from its start on: bit 0 and the bits 1 + j * a (inside a window the advance has not grown yet)
__device__ __forceinline__ uint64_t lz4_probe_pattern(int32_t a)
{
    uint64_t p = 1;
    for (int32_t b = 1; b < 64; b += a) {
        p |= 1ull << b;
    }
    return p;
}

// ---- the pieces every LZ4 block encoder is made of: the serial kernel (lz4_compress_kernels.h), lz4_compress_block below, lz4_compress_block_mw ----

// The block's prologue, in two steps.  The statuses of :64-67 / :83-89: 0 for a block that is encoded ...
__device__ __forceinline__ int32_t lz4_block_status(int32_t inLen, int32_t outCap)
{
    const int64_t bound = (int64_t)inLen + inLen / 255 + 16;
    int32_t st = 0;
    if ((uint32_t)inLen > 0x7E000000u) {
        st = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_LZ4_MAX_INPUT);
    }
    else if ((int64_t)outCap < bound) {
        st = mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_LZ4_MAX_OUTPUT);
    }
    return st;
}
// ... and for such a block computeTableSize :304-311 and the table clear; returns the table size.  The caller puts its own sync behind it (__syncthreads, or
// wave_sync where the wavefront may share its workgroup with others).
template <typename TableT>
__device__ __forceinline__ int32_t lz4_table_init(int32_t inLen, TableT* table, int lane)
{
    using namespace lz4c;
    int32_t tableSize = inLen <= 1 ? 0 : (int32_t)((0x80000000u >> __builtin_clz((uint32_t)(inLen - 1))) << 1);
    tableSize = tableSize < MIN_TABLE_SIZE ? MIN_TABLE_SIZE : (tableSize > MAX_TABLE_SIZE ? MAX_TABLE_SIZE : tableSize);
    for (int i = lane; i < tableSize; i += 64) {
        table[i] = 0;
    }
    return tableSize;
}

// catch up :141-144 from memory -- one lane per candidate byte, first mismatch by ballot, at most `room` bytes.  Moves both positions back and returns the
// number of trips it took (every one but the last compared 64 bytes; the counting build of lz4_compress_mw.h counts the second trips).
__device__ __forceinline__ int32_t lz4_catch_up_mem(const uint8_t* in, int32_t& input, int32_t& matchIndex, int32_t room, int lane)
{
    int32_t trips = 0;
    while (room > 0) {
        const bool eq = lane < room && in[input - 1 - lane] == in[matchIndex - 1 - lane];
        const unsigned long long ne = ~__ballot(eq);
        const int run = ne ? __builtin_ctzll(ne) : 64;
        input -= run;
        matchIndex -= run;
        room -= run;
        trips++;
        if (run < 64) {
            break;
        }
    }
    return trips;
}

// emitMatch :209-235 behind a literal run already in place: lane 0 writes the token at tokenPos and the offset and length bytes at `at`; every lane
// returns the output position behind them
__device__ __forceinline__ int32_t lz4_emit_match(uint8_t* out, int32_t tokenPos, int32_t literalLength, int32_t offset, int32_t matchLength, int32_t at, int lane)
{
    using namespace lz4c;
    if (lane == 0) {
        lz4_write_run_length(out, tokenPos, literalLength, matchLength >= ML_MASK ? ML_MASK : (uint32_t)matchLength);
        out[at] = (uint8_t)offset;
        out[at + 1] = (uint8_t)((uint32_t)offset >> 8);
        if (matchLength >= ML_MASK) {
            int32_t o = at + 2;
            int32_t remaining = matchLength - ML_MASK;
            while (remaining >= 510) {
                out[o++] = 255;
                out[o++] = 255;
                remaining -= 510;
            }
            if (remaining >= 255) {
                out[o++] = 255;
                remaining -= 255;
            }
            out[o++] = (uint8_t)remaining;
        }
    }
    return at + 2 + (matchLength >= ML_MASK ? 1 + (matchLength - ML_MASK) / 255 : 0);
}

// emitLastLiteral :269-280: the bytes from `anchor` to the block's end; returns the new output position
__device__ __forceinline__ int32_t lz4_emit_last_literals(const uint8_t* in, uint8_t* out, int32_t output, int32_t anchor, int32_t inputLimit, int lane)
{
    const int32_t length = inputLimit - anchor;
    if (lane == 0) {
        lz4_write_run_length(out, output, length, 0);
    }
    output += lz4_run_length_size(length);
    group_copy<64>(out + output, in + anchor, length, lane);
    return output + length;
}

// ---- the batch-probe step: 64 steps of the search loop :113-138 at once ----
// A lane is idle (role 0), inserts `pos` without probing (role 1: the `input - 2` insert behind a match, position 0 of a block) or probes (role 2): at `pos` as
// the caller gives it (k < 0: the re-probe right behind a match), or at probe k >= 0 of the search that began at scanStart -- the skip schedule's position.
// Every probe is evaluated against the table as the serial loop would have left it for it: its candidate is the latest earlier lane of the batch with the same
// hash, else the table's entry.  The first hit is the winner; a search probe whose successor passes matchFindLimit (:127-129) ends the batch before it.  The
// table takes the latest position of every hash among the lanes up to the winner (without one: up to the last valid lane).  The caller syncs behind the step
// and reads `pos` / `cand` at the winner's lane.
struct Lz4ProbeStep {
    int winner;        // first lane that hit, -1: none
    int firstInvalid;  // first lane whose probe would run off the end, 64: none
    int32_t pos;       // this lane's position
    int32_t cand;      // ... and its candidate
};

// (MAXD: the farthest candidate a probe accepts -- the LZO encoder, lzo_compress.hip, runs the same step with its own MAX_DISTANCE)
template <typename TableT, bool ACCEL, int MAXD = lz4c::MAX_DISTANCE>
__device__ __forceinline__ Lz4ProbeStep lz4_probe_step(const uint8_t* in, TableT* table, int32_t mask, int hashBits, int32_t matchFindLimit, int32_t scanStart, int32_t accel,
                                                       int role, int32_t pos, int32_t k, int lane)
{
    using namespace lz4c;
    bool valid = true;
    if (k >= 0) {
        if constexpr (ACCEL) {
            pos = scanStart + lz4_scan_offset(k, accel);
            valid = pos + lz4_scan_advance(k, accel) <= matchFindLimit;
        }
        else {
            pos = scanStart + lz4_scan_offset(k);
            valid = pos + lz4_scan_advance(k) <= matchFindLimit;
        }
    }
    const unsigned long long invalidMask = __ballot(role == 2 && !valid);
    const int firstInvalid = invalidMask ? __builtin_ctzll(invalidMask) : 64;
    const bool active = role != 0 && lane < firstInvalid;
    const unsigned long long activeMask = __ballot(active);

    // ---- evaluate every probe against the table state it would see ----
    uint64_t x = 0;
    int32_t h = 0;
    int32_t cand = 0;
    if (active) {
        x = ld8(in + pos);
        h = lz4_hash(x, mask);
        cand = (int32_t)table[h];
    }
    const unsigned long long same = wave_match_any((uint32_t)h, hashBits, activeMask);
    const unsigned long long earlier = same & ((1ull << lane) - 1ull);
    {  // every lane takes part in the shuffle (a lane outside the branch could not be read from)
        const bool fromBatch = active && earlier != 0;
        const int32_t latest = __shfl(pos, fromBatch ? 63 - __builtin_clzll(earlier) : lane);
        if (fromBatch) {
            cand = latest;
        }
    }
    bool hit = false;
    if (active && role == 2) {
        hit = ld4(in + cand) == (uint32_t)x && cand + MAXD >= pos;
    }
    const unsigned long long hitMask = __ballot(hit);
    const int winner = hitMask ? __builtin_ctzll(hitMask) : -1;
    const int lastWriter = winner >= 0 ? winner : firstInvalid - 1;  // lanes 0..lastWriter update the table
    // ---- write back: the latest position of every hash among lanes 0..lastWriter ----
    {
        const unsigned long long upTo = lastWriter >= 63 ? ~0ull : ((1ull << (lastWriter + 1)) - 1ull);
        const unsigned long long later = same & upTo & ~((2ull << lane) - 1ull);
        if (active && lane <= lastWriter && later == 0) {
            table[h] = (TableT)pos;
        }
    }
    return {winner, firstInvalid, pos, cand};
}

// The batch-probe encoder of one block (M/lz4/Lz4RawCompressor.java:74-187) by one wavefront; `table` is MAX_TABLE_SIZE
// entries of LDS.  Returns the compressed length; stOut receives 0 or the status.  The batched block encoder's batch-probe kernels
// (lz4_compress_kernels.h).
template <typename TableT, bool ACCEL = false>
__device__ int32_t lz4_compress_block(const uint8_t* __restrict__ in, int32_t inLen, uint8_t* __restrict__ out, int32_t outCap, TableT* table, int lane, int32_t& stOut, int32_t accel = 1)
{
    using namespace lz4c;
    int32_t output = 0;
    const int32_t st = lz4_block_status(inLen, outCap);
    if (st == 0) {
        const int32_t tableSize = lz4_table_init(inLen, table, lane);
        __syncthreads();
        const int32_t mask = tableSize - 1;
        const int hashBits = 32 - __builtin_clz((uint32_t)mask | 1u);
        const int32_t inputLimit = inLen;
        const int32_t matchFindLimit = inputLimit - MATCH_FIND_LIMIT;
        const int32_t matchLimit = inputLimit - LAST_LITERAL_SIZE;
        int32_t anchor = 0;

        if (inLen >= MIN_LENGTH) {
#define BATCH_SEARCH_PROBE(role, pos, k) lz4_probe_step<TableT, ACCEL>(in, table, mask, hashBits, matchFindLimit, scanStart, accel, role, pos, k, lane)
#define BATCH_SEARCH_EMIT_STATE     \
    int32_t literalLength = 0;      \
    int32_t tokenPos;
#define BATCH_SEARCH_EMIT_LITERALS                                                                         \
    literalLength = input - anchor;                                                                        \
    tokenPos = output;                                                                                     \
    const int32_t litPos = tokenPos + lz4_run_length_size(literalLength);                                  \
    group_copy<64>(out + litPos, in + anchor, literalLength, lane); /* emitLiteral :194-207 */            \
    output = litPos + literalLength;
#define BATCH_SEARCH_EMIT_NO_LITERALS tokenPos = output++; /* zero-literal token :181-183 */
#define BATCH_SEARCH_EMIT_MATCH output = lz4_emit_match(out, tokenPos, literalLength, input - matchIndex, matchLength, output, lane);
#include "lz4_batch_search.h"
#undef BATCH_SEARCH_PROBE
#undef BATCH_SEARCH_EMIT_STATE
#undef BATCH_SEARCH_EMIT_LITERALS
#undef BATCH_SEARCH_EMIT_NO_LITERALS
#undef BATCH_SEARCH_EMIT_MATCH
        }
        output = lz4_emit_last_literals(in, out, output, anchor, inputLimit, lane);
    }
    stOut = st;
    return output;
}

}  // namespace achip

