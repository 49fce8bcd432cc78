// decoded_size.hip -- what a batch decodes to, found on the device without decoding it (achip_decoded_size_batch), and the planner that turns
// the sizes into the dstOff[] / dstCap[] the decoders take (achip_plan_outputs).  DESIGN 10b has the contract (R1 exact, R2 never a wrong size).
//
//   LZ4 raw blocks    the token walk of M/lz4/Lz4RawDecompressor.java:59-195 without the rules that depend on the output limit (:82-96, :168-171: a caller
//                     of this pass has no limit yet) -- no record, no byte written.  A lane per block for batches that fill the chip, a wavefront per block
//                     (64 token positions per trip over WaveStage, the real sequences a chain of lane reads: lz4_parse_wave_kernel's shape) below that.
//   Snappy raw blocks the varint preamble, M/snappy/SnappyRawDecompressor.java:277-321 (achip_snappy_uncompressed_length's rules), a lane per block.
//   Zstd              a wavefront per item walks frames and blocks (M/zstd/ZstdFrameDecompressor.java:135-210): RAW / RLE sizes from the block header, a
//                     compressed block = the literals header's regenerated size + the match lengths of its sequence section (:312-516 without the execution).
//                     The frame header's content size is NOT used: the decoder never compares it with what the blocks produce, so a size taken from it could
//                     be one the decoder succeeds with another length for (R2).
//   containers        a lane per stream runs the reader's loop over the headers.  Where the loop needs the size of an LZ4 block (LZ4 frames without a content
//                     size, Hadoop LZ4 chunks) the blocks are first LISTED as a batch (achip_lists.h), sized by the LZ4 kernels above, and the loop then runs with
//                     the listed sizes at hand (the fold); a block the list does not hold -- the list was full, or the stream is not of the shape the listing
//                     assumed -- is walked by the lane itself.
//   planner           reduce, scan of the partial sums by one workgroup, scan: three launches, no workgroup waits for another.
#include "achip_waveparse.h"
#include "lzo_decode_body.h"
#include "lz4_frame_head.h"
#include "zstd_default_tables.h"
#include "achip_launch.h"
#include "achip_lists.h"
#include "achip_plan.h"

namespace achip {

namespace ds {

__device__ __forceinline__ int32_t item_count(const SizeArgs& s) { return s.nBlocksDev != nullptr ? *s.nBlocksDev : s.nBlocks; }

__device__ __forceinline__ void put_result(const SizeArgs& s, int64_t item, int64_t size, int32_t st, int64_t eo)
{
    s.outSize[item] = st == 0 ? size : 0;
    s.status[item] = st;
    s.errOffset[item] = st == 0 ? 0 : eo;
}

// ---------------------------------------------------------------------------------------------------------------------
// LZ4

struct Lz4Walk {
    int32_t ip;
    int32_t st, eo;
    int64_t op;
};

#define DS_LZ4_FAIL(detail, off)                         \
    {                                                    \
        w.st = mk_status(ACHIP_CLASS_MALFORMED, detail); \
        w.eo = (int32_t)(off);                           \
        return true;                                     \
    }

// One sequence of the Java loop (w.ip < inLimit on entry); true: the walk is over (w.st says how).  A block that ends behind a match -- the decoder takes it with
// room to spare and refuses it with exact room, :168-171 -- ends the walk with status 0: R2 holds, R1 does not speak of it.
// HISTORY: a block of an LZ4 frame with linked blocks (lz4frame_size_item): `history` bytes of the frame's content lie in front of it and an offset may reach them.
template <bool HISTORY = false>
__device__ __forceinline__ bool lz4_size_step(const uint8_t* __restrict__ in, int32_t inLimit, Lz4Walk& w, int64_t history = 0)
{
    int32_t ip = w.ip;
    uint64_t x = 0;  // the token and the bytes behind it
    if (ip + 8 <= inLimit) {
        x = ld8(in + ip);
    }
    else {
        for (int i = 0; ip + i < inLimit; i++) {
            x |= (uint64_t)in[ip + i] << (8 * i);
        }
    }
    const int32_t token = (int32_t)(x & 0xFF);
    ip++;
    int32_t lit = token >> 4;  // :62-77
    if (lit == 0xF) {
        if (ip >= inLimit) DS_LZ4_FAIL(ACHIP_D_LZ4_MALFORMED, ip);
        int32_t v = (int32_t)((x >> 8) & 0xFF);
        ip++;
        lit = (int32_t)((uint32_t)lit + (uint32_t)v);
        while (v == 255 && ip < inLimit - 15) {
            v = in[ip++];
            lit = (int32_t)((uint32_t)lit + (uint32_t)v);
        }
    }
    if (lit < 0) DS_LZ4_FAIL(ACHIP_D_LZ4_MALFORMED, ip);
    const int64_t litEnd = (int64_t)ip + lit;
    if (litEnd > inLimit - 8) {  // :82-96 the last literals
        if (litEnd != inLimit) DS_LZ4_FAIL(ACHIP_D_LZ4_INPUT_NOT_CONSUMED, ip);
        w.op += lit;
        w.ip = inLimit;
        return true;
    }
    w.op += lit;
    ip = (int32_t)litEnd;
    const uint32_t y = ld4(in + ip);  // the offset and the byte behind it (litEnd <= inLimit - 8)
    const int32_t offset = (int32_t)(y & 0xFFFF);  // :113-119
    ip += 2;
    if (offset == 0 || (int64_t)offset > (HISTORY ? w.op + history : w.op)) DS_LZ4_FAIL(ACHIP_D_LZ4_OFFSET_OUTSIDE, ip);
    int32_t ml = token & 0xF;  // :122-138
    if (ml == 0xF) {
        if (ip > inLimit - 5) DS_LZ4_FAIL(ACHIP_D_LZ4_MALFORMED, ip);
        int32_t v = (int32_t)((y >> 16) & 0xFF);
        ip++;
        ml = (int32_t)((uint32_t)ml + (uint32_t)v);
        while (v == 255) {
            if (ip > inLimit - 5) DS_LZ4_FAIL(ACHIP_D_LZ4_MALFORMED, ip);
            v = in[ip++];
            ml = (int32_t)((uint32_t)ml + (uint32_t)v);
        }
    }
    ml = (int32_t)((uint32_t)ml + 4u);
    if (ml < 0) DS_LZ4_FAIL(ACHIP_D_LZ4_MALFORMED, ip);
    w.op += ml;
    w.ip = ip;
    return ip >= inLimit;
}
#undef DS_LZ4_FAIL

// a whole block by one lane
template <bool HISTORY = false>
__device__ __forceinline__ void lz4_size_serial(const uint8_t* __restrict__ in, int32_t inLimit, int64_t& size, int32_t& st, int32_t& eo, int64_t history = 0)
{
    Lz4Walk w;
    w.ip = 0;
    w.st = 0;
    w.eo = 0;
    w.op = 0;
    if (inLimit <= 0) {  // :48-50
        w.st = mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_LZ4_INPUT_EMPTY);
    }
    else {
        while (!lz4_size_step<HISTORY>(in, inLimit, w, history)) {
        }
    }
    st = w.st;
    eo = w.eo;
    size = w.st == 0 ? w.op : 0;
}

}  // namespace ds

__global__ __launch_bounds__(64) void lz4_size_lane_kernel(SizeArgs s)
{
    const int64_t block = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (block >= ds::item_count(s)) {
        return;
    }
    int64_t size = 0;
    int32_t st = 0, eo = 0;
    ds::lz4_size_serial(s.srcBase + s.srcOff[block], s.srcLen[block], size, st, eo);
    ds::put_result(s, block, size, st, eo);
}

// LZO: the decoder's own walk (lzo_decode_body.h) with a capacity of INT32_MAX, a lane per item -- no record, no byte written
__global__ __launch_bounds__(64) void lzo_size_kernel(SizeArgs s)
{
    const int64_t item = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (item >= ds::item_count(s)) {
        return;
    }
    const uint8_t* __restrict__ in = s.srcBase + s.srcOff[item];
    const int32_t inLimit = s.srcLen[item];
    lzod::Walk w;
    w.begin();
    int32_t ml, off, lit, litPos;
    while (lzod::step(in, inLimit, 0x7FFFFFFF, w, ml, off, lit, litPos) != lzod::STEP_DONE) {
    }
    ds::put_result(s, item, w.op, w.st, w.eo);
}

// A wavefront per block, the blocks of a launch dealt round over its workgroups (a batch listed on the device has a count the host does not know).  Lane p reads the
// window's bytes as if a sequence began at position p; the chain from position 0 picks the real ones (wave_chain); a scan gives them their output positions for the
// offset check.  A sequence with a second extension byte, a failing check, or one near the block's end stops the chain and goes through lz4_size_step, every lane
// computing the same.
__global__ __launch_bounds__(64) void lz4_size_wave_kernel(SizeArgs s)
{
    __shared__ __attribute__((aligned(16))) uint8_t stageLds[WaveStage<wp::LZ4_STAGE>::CAP + 16];
    const int lane = threadIdx.x;
    const int32_t count = uni(ds::item_count(s));
    for (int64_t block = blockIdx.x; block < count; block += gridDim.x) {  // (uniform)
        const uint8_t* __restrict__ in = s.srcBase + s.srcOff[block];
        const int32_t inLimit = uni(s.srcLen[block]);
        WaveStage<wp::LZ4_STAGE> W;
        W.init(stageLds, in, inLimit, lane);
        ds::Lz4Walk w;
        w.ip = 0;
        w.st = 0;
        w.eo = 0;
        w.op = 0;
        bool done = false;  // (uniform)
        if (inLimit <= 0) {
            w.st = mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_LZ4_INPUT_EMPTY);
            done = true;
        }
        while (!done) {  // (uniform)
            bool general = true;
            // nothing a window looks at can reach the block's last bytes (lz4_parse_wave_kernel's margin): none of the Java loop's end-of-input branches is near
            if ((int64_t)w.ip + wp::LZ4_STAGE + 24 <= (int64_t)inLimit) {
                const int32_t base = w.ip;
                const uint8_t* const stage = W.window(base);
                // what a sequence at position `lane` of the window would be (as in lz4_parse_wave_kernel; stated here again, not shared: read through a common
                // helper this kernel sized the corpus batch of 8 192 blocks in 1.1858 ms against 1.1802, the old code's three runs within 0.0012 --
                // profiles/twopass_refactor_ab.txt)
                uint32_t x;
                __builtin_memcpy(&x, stage + lane, 4);
                const uint32_t token = x & 0xFF, e1 = (x >> 8) & 0xFF;
                const bool litExt = (token >> 4) == 0xF;
                const int32_t lit = (int32_t)(litExt ? 15u + e1 : (token >> 4));
                const int32_t q = lane + (litExt ? 2 : 1) + lit;  // the offset field (<= 334)
                uint32_t y;
                __builtin_memcpy(&y, stage + q, 4);
                const int32_t offset = (int32_t)(y & 0xFFFF);
                const uint32_t e2 = (y >> 16) & 0xFF;
                const bool mlExt = (token & 0xF) == 0xF;
                const int32_t ml = (int32_t)(mlExt ? 15u + e2 : (token & 0xF)) + 4;
                const int32_t next = q + (mlExt ? 3 : 2);
                const bool stop = (litExt && e1 == 255) || (mlExt && e2 == 255);
                const unsigned long long stopMask = __ballot(stop);
                unsigned long long members = 0;
                int32_t cur = 0;
                wave_chain(next, stop, stopMask, lane, members, cur);
                const bool member = ((members >> lane) & 1ull) != 0;
                const int32_t endRel = sx::wave_scan_incl(member ? lit + ml : 0, lane);  // (at most 64 x 542)
                const bool wrong = member && (offset == 0 || (int64_t)offset > w.op + endRel - ml);
                const unsigned long long wrongMask = __ballot(wrong);
                if (wrongMask != 0) {  // (uniform) the chain ends in front of the failing sequence: the step below reports it
                    const int first = __builtin_ctzll(wrongMask);
                    members &= (1ull << first) - 1ull;
                    cur = first;
                }
                if (members != 0) {  // (uniform)
                    const int last = 63 - __builtin_clzll(members);
                    w.op += sx::wave_bcast(endRel, last);
                    w.ip = base + cur;
                    general = false;
                }
            }
            if (general) {
                done = ds::lz4_size_step(in, inLimit, w);
            }
        }
        if (lane == 0) {
            ds::put_result(s, block, w.op, w.st, w.eo);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Snappy: readUncompressedLength, M/snappy/SnappyRawDecompressor.java:277-321 (achip_device.h snappy_announced)
__global__ __launch_bounds__(64) void snappy_size_kernel(SizeArgs s)
{
    const int64_t block = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (block >= s.nBlocks) {
        return;
    }
    int32_t eo = 0;
    const int32_t r = snappy_announced(s.srcBase + s.srcOff[block], s.srcLen[block], eo);
    ds::put_result(s, block, r, r < 0 ? r : 0, eo);
}

// ---------------------------------------------------------------------------------------------------------------------
// Zstd: a wavefront per item, everything wave-uniform (zstd_decompress.hip's walk without its output)
// The walk below is zstd_decompress.hip's (zstd_decompress_item and what it calls, without the output), stated here again, not shared: a change there belongs here
// too.  On a walk shared with the decoder (one template over frames, blocks and sections, a sink per caller) this kernel sized 65 536 text frames in 212.19 ms
// against 205.60, the old code's three runs within 0.49 (profiles/zstd_grammar_ab.txt).  R3 of tests/decoded_size_cases.py holds the two together: a fault
// reported here is the fault the decoder reports.
namespace ds {
using namespace zd;

// the literals section's header (:708-858): returns the section's bytes or -1; *litSize = what it regenerates.  Its streams are not looked at (a fault in them is
// the payload decode's to find); a treeless section needs a table from an earlier section as in the decoder (haveHuf: one was announced).
__device__ int32_t zstd_literals_header(Ctx& c, bool& haveHuf, int32_t input, int32_t blockSize, int32_t* litSize)
{
    const int32_t inputAddress = input;
    const int32_t inputLimit = input + blockSize;
    const int32_t b0 = (int32_t)rd_le(c, input, 1);
    const int32_t literalsBlockType = b0 & 3;
    const int32_t type = (b0 >> 2) & 3;
    if (literalsBlockType == 0) {  // decodeRawLiterals :812-858
        int32_t literalSize;
        if (type == 0 || type == 2) {
            literalSize = b0 >> 3;
            input += 1;
        }
        else if (type == 1) {
            literalSize = (int32_t)rd_le(c, input, 2) >> 4;
            input += 2;
        }
        else {
            literalSize = (int32_t)rd_le(c, input, 3) >> 4;
            input += 3;
        }
        ZVERIFY(c, input + literalSize <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
        *litSize = literalSize;
        return input + literalSize - inputAddress;
    }
    if (literalsBlockType == 1) {  // decodeRleLiterals :776-810
        int32_t outputSize;
        if (type == 0 || type == 2) {
            outputSize = b0 >> 3;
            input += 1;
        }
        else if (type == 1) {
            outputSize = (int32_t)rd_le(c, input, 2) >> 4;
            input += 2;
        }
        else {
            ZVERIFY(c, blockSize >= 4, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
            outputSize = (int32_t)(rd_le(c, input, 4) & 0xFFFFFF) >> 4;
            input += 3;
        }
        ZVERIFY(c, outputSize <= MAX_BLOCK_SIZE, ACHIP_D_ZSTD_LITERALS_TOO_LARGE, input);
        *litSize = outputSize;
        return input + 1 - inputAddress;
    }
    if (literalsBlockType == 3) {  // decodeCompressedLiterals :708-774
        ZVERIFY(c, haveHuf, ACHIP_D_ZSTD_DICT_CORRUPTED, input);
    }
    ZVERIFY(c, blockSize >= 5, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
    int32_t compressedSize, uncompressedSize, headerSize;
    if (type == 0 || type == 1) {
        const uint32_t header = (uint32_t)rd_le(c, input, 4);
        headerSize = 3;
        uncompressedSize = (int32_t)((header >> 4) & 0x3FF);
        compressedSize = (int32_t)((header >> 14) & 0x3FF);
    }
    else if (type == 2) {
        const uint32_t header = (uint32_t)rd_le(c, input, 4);
        headerSize = 4;
        uncompressedSize = (int32_t)((header >> 4) & 0x3FFF);
        compressedSize = (int32_t)((header >> 18) & 0x3FFF);
    }
    else {
        const uint64_t header = rd_le(c, input, 5);
        headerSize = 5;
        uncompressedSize = (int32_t)((header >> 4) & 0x3FFFF);
        compressedSize = (int32_t)((header >> 22) & 0x3FFFF);
    }
    ZVERIFY(c, uncompressedSize <= MAX_BLOCK_SIZE, ACHIP_D_ZSTD_LITERALS_TOO_LARGE, input);
    ZVERIFY(c, headerSize + compressedSize <= blockSize, ACHIP_D_ZSTD_CORRUPTED, input);
    if (literalsBlockType == 2) {
        haveHuf = true;
    }
    *litSize = uncompressedSize;
    return headerSize + compressedSize;
}

struct SeqTables {
    int32_t log[3];  // -1: none yet in this frame
    const FseTable* cur[3];
};

// computeLiteralsTable / computeOffsetsTable / computeMatchLengthTable :609-676 ; returns the new input or -1
__device__ int32_t zstd_seq_table(Ctx& c, TableShared& sh, SeqTables& t, int which, int32_t type, int32_t input, int32_t inputLimit, const FseTable* dflt, int32_t dfltLog,
                                  int32_t maxSymbol, int32_t maxLog)
{
    if (type == 1) {
        ZVERIFY(c, input < inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
        const int32_t value = (int8_t)rd_le(c, input++, 1);
        ZVERIFY(c, value <= maxSymbol, ACHIP_D_ZSTD_VALUE_TOO_LARGE, input);
        ZVERIFY(c, value >= 0, ACHIP_D_ZSTD_CORRUPTED, input);
        __syncthreads();
        if (c.lane == 0) {
            sh.fse[which].e[0] = (uint32_t)value << 16;
        }
        __syncthreads();
        t.cur[which] = &sh.fse[which];
        t.log[which] = 0;
    }
    else if (type == 0) {
        t.cur[which] = dflt;
        t.log[which] = dfltLog;
    }
    else if (type == 3) {
        ZVERIFY(c, t.log[which] >= 0, ACHIP_D_ZSTD_TABLE_MISSING, input);
    }
    else {
        int32_t log = 0;
        const int32_t n = read_fse_table(c, sh, sh.fse[which], input, inputLimit, maxSymbol, maxLog, &log);
        if (n < 0) return -1;
        input += n;
        t.cur[which] = &sh.fse[which];
        t.log[which] = log;
    }
    return input;
}

// decompressSequences :312-516 without the execution: the sum of the match lengths of the sequences the Java loop decodes, or -1.  The bits are consumed
// exactly as there (all three codes of a sequence, the offset's extra bits included: they move the stream).
__device__ int64_t zstd_match_bytes(Ctx& c, TableShared& sh, SeqTables& t, const FseTable* dflt, int32_t inputAddress, int32_t inputLimit)
{
    int32_t input = inputAddress;
    ZVERIFY(c, inputLimit - inputAddress >= 1, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
    int32_t sequenceCount = (int32_t)rd_le(c, input++, 1);
    if (sequenceCount == 0) {
        return 0;
    }
    if (sequenceCount == 255) {
        ZVERIFY(c, input + 2 <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
        sequenceCount = (int32_t)rd_le(c, input, 2) + 0x7F00;
        input += 2;
    }
    else if (sequenceCount > 127) {
        ZVERIFY(c, input < inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
        sequenceCount = ((sequenceCount - 128) << 8) + (int32_t)rd_le(c, input++, 1);
    }
    ZVERIFY(c, input + 4 <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
    const int32_t type = (int32_t)rd_le(c, input++, 1);
    input = zstd_seq_table(c, sh, t, 0, type >> 6, input, inputLimit, &dflt[0], 6, 35, 9);
    if (input < 0) return -1;
    input = zstd_seq_table(c, sh, t, 1, (type >> 4) & 3, input, inputLimit, &dflt[1], 5, 28, 8);
    if (input < 0) return -1;
    input = zstd_seq_table(c, sh, t, 2, (type >> 2) & 3, input, inputLimit, &dflt[2], 6, 52, 9);
    if (input < 0) return -1;
    Bits b;
    {
        int32_t eo = 0;
        const int32_t d = bit_init(c, b, input, inputLimit, &eo);
        if (d != 0) ZFAIL(c, d, eo);
    }
    __syncthreads();
    const FseTable* llt = t.cur[0];
    const FseTable* oft = t.cur[1];
    const FseTable* mlt = t.cur[2];
    int32_t llState = (int32_t)peek_bits(b.consumed, b.bits, t.log[0]);
    b.consumed += t.log[0];
    int32_t ofState = (int32_t)peek_bits(b.consumed, b.bits, t.log[1]);
    b.consumed += t.log[1];
    int32_t mlState = (int32_t)peek_bits(b.consumed, b.bits, t.log[2]);
    b.consumed += t.log[2];
    int64_t matchBytes = 0;
    while (sequenceCount > 0) {
        sequenceCount--;
        b.overflow = false;
        bit_load(c, b);
        if (b.overflow) {
            ZVERIFY(c, sequenceCount == 0, ACHIP_D_ZSTD_SEQUENCES_NOT_CONSUMED, input);
            break;
        }
        const uint32_t lle = llt->e[llState], mle = mlt->e[mlState], ofe = oft->e[ofState];
        const int32_t llCode = FSE_SYMBOL(lle), mlCode = FSE_SYMBOL(mle), ofCode = FSE_SYMBOL(ofe);
        const int32_t llBits = LL_BITS[llCode], mlBits = ML_BITS[mlCode], ofBits = ofCode;
        if (ofCode > 0) {
            b.consumed += ofBits;
        }
        int32_t matchLength = ML_BASE[mlCode];
        if (mlCode > 31) {
            matchLength += (int32_t)peek_bits(b.consumed, b.bits, mlBits);
            b.consumed += mlBits;
        }
        if (llCode > 15) {
            b.consumed += llBits;
        }
        if (llBits + mlBits + ofBits > 64 - 7 - (9 + 9 + 8)) {
            bit_load(c, b);
        }
        int32_t nb = FSE_NBITS(lle);
        llState = FSE_NEWSTATE(lle) + (int32_t)peek_bits(b.consumed, b.bits, nb);
        b.consumed += nb;
        nb = FSE_NBITS(mle);
        mlState = FSE_NEWSTATE(mle) + (int32_t)peek_bits(b.consumed, b.bits, nb);
        b.consumed += nb;
        nb = FSE_NBITS(ofe);
        ofState = FSE_NEWSTATE(ofe) + (int32_t)peek_bits(b.consumed, b.bits, nb);
        b.consumed += nb;
        llState &= 511;  // (a state past the table comes from corrupt tables only: the LDS reads stay in range, as in the decoder)
        mlState &= 511;
        ofState &= 511;
        matchBytes += matchLength;
    }
    return matchBytes;
}

// ZstdFrameDecompressor.decompress :135-210 ; the bytes its frames decode to, or -1 (c.detail, c.errOff)
__device__ int64_t zstd_size_item(Ctx& c, TableShared& sh, const FseTable* dflt)
{
    const int32_t inputLimit = c.inLen;
    int32_t input = 0;
    int64_t output = 0;
    bool haveHuf = false;  // (persists across frames, like the Java Huffman object)
    while (input < inputLimit) {
        SeqTables t;
        t.log[0] = t.log[1] = t.log[2] = -1;
        t.cur[0] = t.cur[1] = t.cur[2] = nullptr;
        ZVERIFY(c, inputLimit - input >= 4, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);  // verifyMagic :949-962 (a skippable frame is a bad magic to this reader)
        const uint32_t magic = (uint32_t)rd_le(c, input, 4);
        if (magic != 0xFD2FB528u) {
            ZFAIL(c, magic == 0xFD2FB527u ? ACHIP_D_ZSTD_V07_MAGIC : ACHIP_D_ZSTD_BAD_MAGIC, input);
        }
        input += 4;
        const int32_t headerAddress = input;  // readFrameHeader :860-940
        ZVERIFY(c, input < inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
        const int32_t fhd = (int32_t)rd_le(c, input++, 1);
        const bool singleSegment = (fhd & 0x20) != 0;
        const int32_t dictDesc = fhd & 3;
        const int32_t csDesc = fhd >> 6;
        const int32_t headerSize = 1 + (singleSegment ? 0 : 1) + (dictDesc == 0 ? 0 : (1 << (dictDesc - 1))) + (csDesc == 0 ? (singleSegment ? 1 : 0) : (1 << csDesc));
        ZVERIFY(c, headerSize <= inputLimit - headerAddress, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
        int32_t windowSize = -1;
        if (!singleSegment) {
            const int32_t wd = (int32_t)rd_le(c, input++, 1);
            const uint32_t base = 1u << ((10 + (wd >> 3)) & 31);
            windowSize = (int32_t)(base + (uint32_t)(((int32_t)base / 8) * (wd & 7)));
        }
        if (dictDesc != 0) {
            ZFAIL(c, ACHIP_D_ZSTD_DICTIONARY, input + (1 << (dictDesc - 1)));
        }
        input = headerAddress + headerSize;
        const bool hasChecksum = (fhd & 4) != 0;
        bool lastBlock;
        do {
            ZVERIFY(c, input + 3 <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
            const int32_t header = (int32_t)rd_le(c, input, 3);
            input += 3;
            lastBlock = (header & 1) != 0;
            const int32_t blockType = (header >> 1) & 3;
            const int32_t blockSize = (header >> 3) & 0x1FFFFF;
            if (blockType == 0) {  // decodeRawBlock :223-229
                ZVERIFY(c, (int64_t)input + blockSize <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
                output += blockSize;
                input += blockSize;
            }
            else if (blockType == 1) {  // decodeRleBlock :231-263
                ZVERIFY(c, input + 1 <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
                output += blockSize;
                input += 1;
            }
            else if (blockType == 2) {  // decodeCompressedBlock :265-310
                ZVERIFY(c, (int64_t)input + blockSize <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
                ZVERIFY(c, blockSize <= MAX_BLOCK_SIZE, ACHIP_D_ZSTD_BLOCK_TOO_LARGE, input);
                ZVERIFY(c, blockSize >= 3, ACHIP_D_ZSTD_BLOCK_TOO_SMALL, input);
                int32_t litSize = 0;
                const int32_t n = zstd_literals_header(c, haveHuf, input, blockSize, &litSize);
                if (n < 0) return -1;
                ZVERIFY(c, windowSize <= MAX_WINDOW_SIZE, ACHIP_D_ZSTD_WINDOW_TOO_LARGE, input + n);
                const int64_t matchBytes = zstd_match_bytes(c, sh, t, dflt, input + n, input + blockSize);
                if (matchBytes < 0) return -1;
                output += litSize + matchBytes;
                input += blockSize;
            }
            else {
                ZFAIL(c, ACHIP_D_ZSTD_INVALID_BLOCK_TYPE, input);
            }
        } while (!lastBlock);
        if (hasChecksum) {
            ZVERIFY(c, input + 4 <= inputLimit, ACHIP_D_ZSTD_NOT_ENOUGH_INPUT, input);
            input += 4;
        }
    }
    return output;
}
}  // namespace ds

__global__ __launch_bounds__(64) void zstd_size_kernel(SizeArgs s, const zd::FseTable* __restrict__ dflt)
{
    __shared__ zd::TableShared sh;
    const int lane = threadIdx.x;
    for (int64_t item = blockIdx.x; item < s.nBlocks; item += gridDim.x) {  // (uniform)
        __syncthreads();
        zd::Ctx c;
        c.in = s.srcBase + s.srcOff[item];
        c.inLen = uni(s.srcLen[item]);
        c.out = nullptr;
        c.outCap = 0;
        c.lit = nullptr;
        c.R = nullptr;
        c.lane = lane;
        c.detail = 0;
        c.errOff = 0;
        const int64_t r = ds::zstd_size_item(c, sh, dflt);
        if (lane == 0) {
            ds::put_result(s, item, r, r >= 0 ? 0 : mk_status(ACHIP_CLASS_MALFORMED, c.detail), c.errOff);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// containers
namespace ds {
using lists::CAPACITY;

// the LZ4 blocks the streams' loops want sized, as a batch for the LZ4 kernels above
struct SizeList {
    int32_t* counters;  // [0] entries allocated, [1] entries in the list (sealed)
    int32_t* sFirst;    // per stream
    int32_t* sCount;    // (0: the stream's entries did not fit -- its lane walks them itself)
    int64_t* cSrcOff;   // per entry
    int32_t* cSrcLen;
    int64_t* cSize;
    int32_t* cStatus;
    int64_t* cErrOff;
    void carve(lists::Carver& k, int64_t nStreams)
    {
        counters = k.take<int32_t>(lists::COUNTER_WORDS);
        sFirst = k.take<int32_t>(nStreams);
        sCount = k.take<int32_t>(nStreams);
        cSrcOff = k.take<int64_t>(CAPACITY);
        cSize = k.take<int64_t>(CAPACITY);
        cErrOff = k.take<int64_t>(CAPACITY);
        cSrcLen = k.take<int32_t>(CAPACITY);
        cStatus = k.take<int32_t>(CAPACITY);
    }
};

// How a stream's loop learns the size of an LZ4 block at srcBase + off.  Listing: the block becomes an entry (FILL) or is counted, and the loop goes on as if the
// block decoded to `assume`.
template <bool FILL>
struct ListingSizer {
    const SizeList& L;
    int32_t first, n;
    __device__ int64_t lz4(const uint8_t*, int64_t off, int32_t len, int64_t assume, int32_t& st, int32_t& eo)
    {
        if (FILL) {
            L.cSrcOff[first + n] = off;
            L.cSrcLen[first + n] = len;
        }
        n++;
        st = 0;
        eo = 0;
        return assume;
    }
    __device__ int64_t lz4_linked(const uint8_t* srcBase, int64_t off, int32_t len, int64_t assume, int64_t, int32_t& st, int32_t& eo) { return lz4(srcBase, off, len, assume, st, eo); }
};
// The fold: the stream's k-th request is its k-th entry if the listing saw the same block there; else the lane walks the block.
struct FoldSizer {
    const SizeList& L;
    int32_t first, count, n;
    __device__ int64_t lz4(const uint8_t* srcBase, int64_t off, int32_t len, int64_t, int32_t& st, int32_t& eo)
    {
        const int32_t k = n++;
        if (k < count && L.cSrcOff[first + k] == off && L.cSrcLen[first + k] == len) {
            st = L.cStatus[first + k];
            eo = (int32_t)L.cErrOff[first + k];
            return L.cSize[first + k];
        }
        int64_t size = 0;
        lz4_size_serial(srcBase + off, len, size, st, eo);
        return size;
    }
    // A block of a linked frame, `history` bytes of the frame's content in front of it.  The list's walk knows no history: a block it sized passed the stricter
    // check at every offset, so the size stands; what it refused for an offset (the first thing it met: everything in front passed) the lane walks again with the
    // history -- which is most blocks of a real linked frame, so such frames are sized at a lane's pace (a parallel walk with histories: when their decode has one).
    __device__ int64_t lz4_linked(const uint8_t* srcBase, int64_t off, int32_t len, int64_t assume, int64_t history, int32_t& st, int32_t& eo)
    {
        int64_t size = lz4(srcBase, off, len, assume, st, eo);
        if (st == mk_status(ACHIP_CLASS_MALFORMED, ACHIP_D_LZ4_OFFSET_OUTSIDE)) {
            lz4_size_serial<true>(srcBase + off, len, size, st, eo, history);
        }
        return size;
    }
};
struct NoSizer {  // (the Snappy containers: the preamble is read in the loop)
    __device__ int64_t lz4(const uint8_t*, int64_t, int32_t, int64_t assume, int32_t& st, int32_t& eo)
    {
        st = 0;
        eo = 0;
        return assume;
    }
    __device__ int64_t lz4_linked(const uint8_t* srcBase, int64_t off, int32_t len, int64_t assume, int64_t, int32_t& st, int32_t& eo) { return lz4(srcBase, off, len, assume, st, eo); }
};

#define DS_FAIL(detail, off)                             \
    {                                                    \
        eo = (int64_t)(off);                             \
        return mk_status(ACHIP_CLASS_MALFORMED, detail); \
    }

// ---- LZ4 frames: Lz4FrameCompression.decompress / decompressFrame / skipFrame, M/lz4/Lz4FrameCompression.java:145-343, without the blocks' bodies.  A frame that
// announces its content size decodes to that or fails (:318); any other frame is the sum of its blocks: a stored block's length, a compressed block's walk.
// acceptLinked (SizeArgs::lz4fLinked, the context's achip_ctx_set_lz4frame_linked_blocks): frames of linked blocks are sized like any other.  The token walk reads
// no match source, but it does compare every offset with the bytes produced so far, as the decoder does -- so a block of a linked frame is walked with the
// frame's content in front of it as its history (FoldSizer::lz4_linked), the decoder's own bound.

template <class Z>
__device__ int32_t lz4frame_size_item(const uint8_t* __restrict__ srcBase, int64_t srcOff, int32_t inLen, bool acceptLinked, Z& z, int64_t& total, int64_t& eo)
{
    using namespace lz4f;
    const uint8_t* __restrict__ in = srcBase + srcOff;
    eo = 0;
    total = 0;
    if (inLen < HEADER_SIZE) DS_FAIL(ACHIP_D_LZ4F_TOO_SHORT, 0);
    int64_t pos = 0;
    while (pos < inLen) {
        if (pos + 4 > inLen) DS_FAIL(ACHIP_D_LZ4F_TRUNC_MAGIC, pos);
        const uint32_t magic = ld4(in + pos);
        if ((magic & SKIPPABLE_MASK) == SKIPPABLE_MAGIC) {  // skipFrame :327-343
            const int64_t spos = pos + 4;
            if (spos + 4 > inLen) DS_FAIL(ACHIP_D_LZ4F_TRUNC_SKIP_SIZE, spos);
            const int64_t frameEnd = spos + 4 + (int64_t)ld4(in + spos);
            if (frameEnd > inLen) DS_FAIL(ACHIP_D_LZ4F_TRUNC_SKIP, spos);
            pos = frameEnd;
            continue;
        }
        if (magic != MAGIC) DS_FAIL(ACHIP_D_LZ4F_BAD_MAGIC, pos);
        // decompressFrame :184-322
        FrameHeader h;
        const int32_t hst = read_frame_header(in, inLen, (int32_t)pos, acceptLinked, h, eo);
        if (hst != 0) {
            return hst;
        }
        const int64_t blockMax = h.blockMax, expectedSize = h.expectedSize;
        const bool blockChecksum = h.blockChecksum, contentSize = h.contentSize, contentChecksum = h.contentChecksum;
        int64_t p = h.firstBlock;
        int64_t o = 0;
        for (;;) {
            if (p + 4 > inLen) DS_FAIL(ACHIP_D_LZ4F_MISSING_BLOCK_SIZE, p);
            const uint32_t header = ld4(in + p);
            p += 4;
            if (header == 0) {
                break;
            }
            const int64_t blockLen = header & 0x7FFFFFFFu;
            if (blockLen > blockMax || p + blockLen > inLen) DS_FAIL(ACHIP_D_LZ4F_BLOCK_PAST_END, p);
            if ((header & UNCOMPRESSED_FLAG) != 0) {
                o += blockLen;
            }
            else if (!contentSize) {
                int32_t bst = 0, beo = 0;
                const int64_t size = h.linked ? z.lz4_linked(srcBase, srcOff + p, (int32_t)blockLen, blockMax, o < 65535 ? o : 65535, bst, beo)
                                              : z.lz4(srcBase, srcOff + p, (int32_t)blockLen, blockMax, bst, beo);
                if (bst != 0) {  // the block codec's exception, its offset relative to the block
                    eo = (int64_t)beo;
                    return bst;
                }
                if (size > blockMax) DS_FAIL(ACHIP_D_LZ4F_BLOCK_EXCEEDS_MAX, p);
                o += size;
            }
            if (blockChecksum) {
                if (p + blockLen + 4 > inLen) DS_FAIL(ACHIP_D_LZ4F_MISSING_BLOCK_CHECKSUM, p + blockLen);
                p += 4;
            }
            p += blockLen;
        }
        if (contentChecksum) {
            if (p + 4 > inLen) DS_FAIL(ACHIP_D_LZ4F_MISSING_CONTENT_CHECKSUM, p);
            p += 4;
        }
        if (contentSize && expectedSize < 0) DS_FAIL(ACHIP_D_LZ4F_CONTENT_SIZE, p);  // (no frame decodes to 2^63 bytes)
        total += contentSize ? expectedSize : o;
        pos = p;
    }
    return 0;
}

// ---- x-snappy-framed: SnappyFramedInputStream read to the end, M/snappy/SnappyFramedInputStream.java:135-305 (snappy_frame.hip's walk_stream without a capacity)
template <class Z>
__device__ int32_t snappyframed_size_item(const uint8_t* __restrict__ srcBase, int64_t srcOff, int32_t inLen, Z&, int64_t& total, int64_t& eo)
{
    constexpr int COMPRESSED_DATA_FLAG = 0x00, UNCOMPRESSED_DATA_FLAG = 0x01, STREAM_IDENTIFIER_FLAG = 0xff;
    const uint8_t* __restrict__ in = srcBase + srcOff;
    eo = 0;
    total = 0;
    if (inLen < 10) DS_FAIL(ACHIP_D_SNF_EOF_STREAM_HEADER, 0);
    if (ld8(in) != 0x50614E73000006FFull || in[8] != 0x70 || in[9] != 0x59) DS_FAIL(ACHIP_D_SNF_BAD_STREAM_HEADER, 0);  // ff 06 00 00 "sNaPpY"
    int32_t pos = 10;
    for (;;) {
        const int32_t chunk = pos;
        if (pos == inLen) {
            return 0;
        }
        if (inLen - pos < 4) DS_FAIL(ACHIP_D_SNF_EOF_BLOCK_HEADER, chunk);
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
            if (length != 6) DS_FAIL(ACHIP_D_SNF_STREAM_ID_LENGTH, chunk);
            skip = true;
            minLength = 6;
        }
        else {
            if (flag <= 0x7f) DS_FAIL(ACHIP_D_SNF_UNSKIPPABLE, chunk);
            skip = true;
            minLength = 0;
        }
        if (length < minLength) DS_FAIL(ACHIP_D_SNF_INVALID_LENGTH, chunk);
        if (skip) {  // (skipping stops quietly at the end of the stream)
            pos += length < inLen - pos ? length : inLen - pos;
            continue;
        }
        if (inLen - pos < length) DS_FAIL(ACHIP_D_SNF_EOF_FRAME, chunk);
        if (flag == COMPRESSED_DATA_FLAG) {
            int32_t beo = 0;
            const int32_t ulen = snappy_announced(in + pos + 4, length - 4, beo);
            if (ulen < 0) {
                eo = (int64_t)beo;
                return ulen;
            }
            total += ulen;
        }
        else {
            total += length - 4;
        }
        pos += length;
    }
}

// ---- Hadoop block streams: Lz4HadoopInputStream / SnappyHadoopInputStream read to the end (M/lz4/Lz4HadoopInputStream.java:47-156, M/snappy/
// SnappyHadoopInputStream.java:44-170; hadoop_streams.hip's Reader without the bodies).  The loop needs every chunk's size to know where the next block length stands:
// the preamble (Snappy), the walk (LZ4 -- the listing assumes a chunk fills its block, which is what every writer produces).
template <bool SNAPPY, class Z>
__device__ int32_t hadoop_size_item(const uint8_t* __restrict__ srcBase, int64_t srcOff, int32_t inLen, Z& z, int64_t& total, int64_t& eo)
{
    const uint8_t* __restrict__ in = srcBase + srcOff;
    eo = 0;
    total = 0;
    int32_t pos = 0;
    int64_t blockLen = 0, chunkLen = 0;  // uncompressedBlockLength; the last chunk's bytes (read to their end)
    auto be = [&](int32_t at) { return (int32_t)(((uint32_t)in[at] << 24) + ((uint32_t)in[at + 1] << 16) + ((uint32_t)in[at + 2] << 8) + (uint32_t)in[at + 3]); };
    for (;;) {
        blockLen -= chunkLen;
        chunkLen = 0;
        while (blockLen == 0) {  // readBigEndianInt :142-156
            if (pos >= inLen) {
                return 0;
            }
            if (inLen - pos < 4) DS_FAIL(ACHIP_D_HDP_TRUNCATED_INT, pos);
            const int32_t v = be(pos);
            pos += 4;
            if (v == -1) {
                return 0;
            }
            blockLen = v;
        }
        if (pos >= inLen) {
            return 0;
        }
        if (inLen - pos < 4) DS_FAIL(ACHIP_D_HDP_TRUNCATED_INT, pos);
        const int32_t clen = be(pos);
        pos += 4;
        if (clen < 0) {
            if (!SNAPPY || clen == -1) {  // (LZ4: any negative length ends the stream, Lz4HadoopInputStream.java:51-54)
                return 0;
            }
            DS_FAIL(ACHIP_D_HDP_NEGATIVE_LENGTH, pos - 4);
        }
        if (clen > inLen - pos) DS_FAIL(ACHIP_D_HDP_EOF_BLOCK_DATA, pos);
        const int32_t chunkPos = pos;
        pos += clen;
        if (SNAPPY) {
            int32_t beo = 0;
            const int32_t announced = snappy_announced(in + chunkPos, clen, beo);
            if (announced < 0) {
                eo = (int64_t)beo;
                return announced;
            }
            if (announced > blockLen) DS_FAIL(ACHIP_D_HDP_CHUNK_EXCEEDS_BLOCK, chunkPos);
            if (announced == 0) {  // SnappyHadoopInputStream.java:66-68: an empty chunk is the end
                return 0;
            }
            chunkLen = announced;
        }
        else {
            int32_t bst = 0, beo = 0;
            chunkLen = z.lz4(srcBase, srcOff + chunkPos, clen, blockLen, bst, beo);
            if (bst != 0) {
                eo = (int64_t)beo;
                return bst;
            }
        }
        total += chunkLen;
    }
}
#undef DS_FAIL

constexpr int KIND_LZ4FRAME = 0, KIND_SNAPPYFRAMED = 1, KIND_LZ4HADOOP = 2, KIND_SNAPPYHADOOP = 3;

template <int KIND, class Z>
__device__ __forceinline__ int32_t container_size_item(const SizeArgs& s, int64_t stream, Z& z, int64_t& total, int64_t& eo)
{
    const int32_t inLen = s.srcLen[stream] > 0 ? s.srcLen[stream] : 0;
    if constexpr (KIND == KIND_LZ4FRAME) {
        return lz4frame_size_item(s.srcBase, s.srcOff[stream], inLen, s.lz4fLinked != 0, z, total, eo);
    }
    else if constexpr (KIND == KIND_SNAPPYFRAMED) {
        return snappyframed_size_item(s.srcBase, s.srcOff[stream], inLen, z, total, eo);
    }
    else {
        return hadoop_size_item<KIND == KIND_SNAPPYHADOOP>(s.srcBase, s.srcOff[stream], inLen, z, total, eo);
    }
}
}  // namespace ds

// a lane per stream: its LZ4 blocks into the list
template <int KIND>
__global__ __launch_bounds__(64) void container_list_kernel(SizeArgs s, ds::SizeList L)
{
    const int64_t stream = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (stream >= s.nBlocks) {
        return;
    }
    int64_t total = 0, eo = 0;
    ds::ListingSizer<false> counting{L, 0, 0};
    ds::container_size_item<KIND>(s, stream, counting, total, eo);
    const int32_t n = counting.n;
    const int32_t first = n > 0 ? atomicAdd(L.counters, n) : 0;
    const bool fits = (int64_t)first + n <= lists::CAPACITY;
    L.sFirst[stream] = first;
    L.sCount[stream] = fits ? n : 0;
    if (fits && n > 0) {
        ds::ListingSizer<true> filling{L, first, 0};
        ds::container_size_item<KIND>(s, stream, filling, total, eo);
    }
    else if (!fits) {  // the part of this stream's range that lies inside the list: empty blocks nobody looks at
        for (int64_t c = first; c < (int64_t)first + n && c < lists::CAPACITY; c++) {
            L.cSrcOff[c] = 0;
            L.cSrcLen[c] = 0;
        }
    }
}

// a lane per stream: the stream's size, the first fault in stream order winning.  LISTED: the LZ4 blocks' sizes are at hand in the list
template <int KIND, bool LISTED>
__global__ __launch_bounds__(64) void container_size_kernel(SizeArgs s, ds::SizeList L)
{
    const int64_t stream = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (stream >= s.nBlocks) {
        return;
    }
    int64_t total = 0, eo = 0;
    int32_t st;
    if constexpr (LISTED) {
        ds::FoldSizer z{L, L.sFirst[stream], L.sCount[stream], 0};
        st = ds::container_size_item<KIND>(s, stream, z, total, eo);
    }
    else {
        ds::NoSizer z;
        st = ds::container_size_item<KIND>(s, stream, z, total, eo);
    }
    ds::put_result(s, stream, total, st, eo);
}

// ---------------------------------------------------------------------------------------------------------------------
// the planner: dstCap[i] = outSize[i], dstOff[i] = the sum of the capacities in front of i, each rounded up to `align`; an item with a status or beyond
// INT32_MAX takes no room.  The scan itself is achip_plan.h's.
namespace ds {
struct PlanRoom {
    const int64_t* __restrict__ outSize;
    const int32_t* __restrict__ status;
    int64_t* dstOff;
    int32_t* dstCap;
    __device__ __forceinline__ int64_t room(int64_t i, int64_t n, int64_t mask, int32_t& cap, int32_t& leftOut) const
    {
        cap = 0;
        leftOut = 0;
        if (i >= n) {
            return 0;
        }
        const int64_t size = outSize[i];
        if (status[i] != 0 || size < 0 || size > 0x7FFFFFFF) {
            leftOut = 1;
            return 0;
        }
        cap = (int32_t)size;
        return (size + mask) & ~mask;
    }
    __device__ __forceinline__ void emit(int64_t i, int64_t at, int32_t cap) const
    {
        dstOff[i] = at;
        dstCap[i] = cap;
    }
    __device__ __forceinline__ void finish(int64_t*) const {}
};
}  // namespace ds

// ---------------------------------------------------------------------------------------------------------------------
// launchers
namespace {
constexpr int64_t ZSTD_TABLES_AT = 1024;  // (the predefined tables in the scratch)

// LZ4 blocks, by the batch size as the two-pass decoder's parser is chosen (lz4_decompress_v7.hip: a wavefront per block up to 16 384 blocks): a lane walks
// one block however many there are, so a batch that leaves lanes of the chip idle is better off with 64 positions per trip.  A count the host does not
// know (a listed batch) takes the shape by its streams.
constexpr int32_t LZ4_SIZE_WAVE_MAX_BLOCKS = 16384;
hipError_t launch_lz4_size(const SizeArgs& s, int32_t shapeCount, hipStream_t stream)
{
    if (shapeCount <= LZ4_SIZE_WAVE_MAX_BLOCKS) {
        const int32_t grid = s.nBlocksDev != nullptr ? LZ4_SIZE_WAVE_MAX_BLOCKS : s.nBlocks;
        hipLaunchKernelGGL(lz4_size_wave_kernel, dim3((unsigned)grid), dim3(64), 0, stream, s);
    }
    else {
        hipLaunchKernelGGL(lz4_size_lane_kernel, dim3((unsigned)((s.nBlocks + 63) / 64)), dim3(64), 0, stream, s);
    }
    return hipGetLastError();
}

template <int KIND>
hipError_t launch_container_size(const SizeArgs& s, hipStream_t stream, void* scratch)
{
    const dim3 grid((unsigned)((s.nBlocks + 63) / 64)), wg(64);
    ds::SizeList L = {};
    if constexpr (KIND == ds::KIND_SNAPPYFRAMED || KIND == ds::KIND_SNAPPYHADOOP) {
        hipLaunchKernelGGL((container_size_kernel<KIND, false>), grid, wg, 0, stream, s, L);
        return hipGetLastError();
    }
    else {
        lists::Carver k(scratch);
        L.carve(k, s.nBlocks);
        hipError_t e = hipMemsetAsync(L.counters, 0, (size_t)lists::COUNTER_WORDS * sizeof(int32_t), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((container_list_kernel<KIND>), grid, wg, 0, stream, s, L);
        hipLaunchKernelGGL(lists::seal_kernel, dim3(1), dim3(1), 0, stream, L.counters, lists::CAPACITY);
        SizeArgs listed = s;
        listed.srcOff = L.cSrcOff;
        listed.srcLen = L.cSrcLen;
        listed.outSize = L.cSize;
        listed.status = L.cStatus;
        listed.errOffset = L.cErrOff;
        listed.nBlocks = lists::CAPACITY;
        listed.nBlocksDev = L.counters + 1;
        e = launch_lz4_size(listed, s.nBlocks, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((container_size_kernel<KIND, true>), grid, wg, 0, stream, s, L);
        return hipGetLastError();
    }
}
}  // namespace

int64_t decoded_size_scratch_bytes(int32_t op, int32_t nBlocks)
{
    if (op == ACHIP_OP_ZSTD_DECOMPRESS) {
        return ZSTD_TABLES_AT + 3 * (int64_t)sizeof(zd::FseTable);
    }
    if (op == ACHIP_OP_LZ4FRAME_DECOMPRESS || op == ACHIP_OP_LZ4HADOOP_DECOMPRESS) {
        lists::Carver k(nullptr);
        ds::SizeList L;
        L.carve(k, nBlocks);
        return k.used();
    }
    return 0;
}

hipError_t launch_decoded_size(int32_t op, const SizeArgs& s, hipStream_t stream, void* scratch)
{
    if (s.nBlocks <= 0) {
        return hipSuccess;
    }
    const dim3 perLane((unsigned)((s.nBlocks + 63) / 64)), wg(64);
    switch (op) {
        case ACHIP_OP_LZ4_DECOMPRESS: return launch_lz4_size(s, s.nBlocks, stream);
        case ACHIP_OP_SNAPPY_DECOMPRESS: hipLaunchKernelGGL(snappy_size_kernel, perLane, wg, 0, stream, s); return hipGetLastError();
        case ACHIP_OP_ZSTD_DECOMPRESS: {
            zd::FseTable* dflt = (zd::FseTable*)((uint8_t*)scratch + ZSTD_TABLES_AT);
            hipLaunchKernelGGL(zstd_default_tables_kernel, dim3(1), wg, 0, stream, dflt);
            // a wavefront and 17 KiB of tables per item: the workgroups a chip holds at once, the items dealt round
            hipLaunchKernelGGL(zstd_size_kernel, dim3((unsigned)(s.nBlocks < 2048 ? s.nBlocks : 2048)), wg, 0, stream, s, (const zd::FseTable*)dflt);
            return hipGetLastError();
        }
        case ACHIP_OP_LZ4FRAME_DECOMPRESS: return launch_container_size<ds::KIND_LZ4FRAME>(s, stream, scratch);
        case ACHIP_OP_SNAPPYFRAMED_DECOMPRESS: return launch_container_size<ds::KIND_SNAPPYFRAMED>(s, stream, scratch);
        case ACHIP_OP_LZ4HADOOP_DECOMPRESS: return launch_container_size<ds::KIND_LZ4HADOOP>(s, stream, scratch);
        case ACHIP_OP_SNAPPYHADOOP_DECOMPRESS: return launch_container_size<ds::KIND_SNAPPYHADOOP>(s, stream, scratch);
        case ACHIP_OP_LZO_DECOMPRESS: hipLaunchKernelGGL(lzo_size_kernel, perLane, wg, 0, stream, s); return hipGetLastError();
        default: return hipErrorUnknown;  // (achip_decoded_size_batch has refused any other op)
    }
}

int64_t plan_outputs_scratch_bytes(int32_t nBlocks) { return plan_scan_scratch_bytes(nBlocks); }

hipError_t launch_plan_outputs(const int64_t* outSize, const int32_t* status, int32_t nBlocks, int32_t align, int64_t* dstOff, int32_t* dstCap, int64_t* total, void* scratch,
                               hipStream_t stream)
{
    return launch_plan_scan(ds::PlanRoom{outSize, status, dstOff, dstCap}, nBlocks, align, total, scratch, stream);
}

}  // namespace achip
