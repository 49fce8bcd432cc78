// lzo_decompress.hip -- batched LZO1X decode for gfx950 (M/lzo/LzoRawDecompressor.java:32-352): an item is any number of concatenated blocks.
//
// The grammar is state-dependent (what a 0b0000_xxxx byte means depends on the literals of the command before it) and serial; lzo_decode_body.h walks it once
// for every kernel here.  Every check of the Java loop depends on lengths, offsets and positions only, so the walk alone decides status, error offset and
// output length -- the copies just move bytes.
//
//   lzo_parse2_kernel            a lane per item (64 items per wavefront) walks the commands and writes records for seq_execute2_kernel (achip_seqexec.h,
//                                lz4_decompress_v7.hip).  An LZO command is a match FOLLOWED by its literals, a record is literals THEN a match: record k pairs
//                                the literals of command k with the match of command k + 1, and the bytes of command k + 1 are the next record's `skip`.  The
//                                first command of a block, a literal run and a block's end have no partner: a record of literals alone.
//   lzo_decompress_wave_kernel   a wavefront per item: every lane walks the same commands (one address per load), the 64 lanes copy -- group_copy /
//                                group_match_copy, the periodic case for offsets below the copy width included.  Self-sufficient: variant 2, batches of a
//                                few items, and what the two passes hand over (`only`: items whose records did not fit the arena or cannot be expressed).
#include "achip_seqexec.h"
#include "lzo_decode_body.h"
#include "achip_launch.h"

namespace achip {

__global__ __launch_bounds__(64) void lzo_parse2_kernel(BatchArgs a, sx::ArenaHeader* hdr, sx::BlockMeta* meta, int32_t* only, uint64_t* arena, int32_t maxChunks, const int32_t* stats)
{
    (void)stats;  // (no probe picks between the LZO decoders on the device: the host does)
    const int lane = threadIdx.x;
    const int64_t block = (int64_t)blockIdx.x * 64 + lane;
    const bool have = block < a.nBlocks;
    const uint8_t* __restrict__ in = have ? a.srcBase + a.srcOff[block] : a.srcBase;
    const int32_t inLimit = have ? a.srcLen[block] : 0;
    const int64_t outLimit = have ? a.dstCap[block] : 0;

    lzod::Walk w;
    w.begin();
    // the sequence whose pieces are being emitted (literals, then a match), and the literals that wait for the next command's match
    int32_t sLit = 0, sLitPos = 0, sMl = 0, sOff = 0, sK = 0, sPieces = 0;
    int32_t cLit = 0, cLitPos = 0;
    int32_t litEndPrev = 0;  // where the literals of the last record ended in the input
    int32_t finished = have ? 0 : 1;
    int32_t fallback = 0;
    uint64_t rec[8];
    int32_t groupAny = 0;
    sx::LaneRecordSink K;
    K.init();

    while (__ballot(finished == 0) != 0) {  // (uniform)
        groupAny = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (finished == 0 && sK == sPieces) {  // the next command
                int32_t ml = 0, off = 0, lit = 0, litPos = 0;
                const int r = lzod::step(in, inLimit, outLimit, w, ml, off, lit, litPos);
                if (r == lzod::STEP_DONE) {
                    finished = 1;
                }
                else {
                    const bool end = r == lzod::STEP_END;
                    sLit = cLit;
                    sLitPos = cLit > 0 ? cLitPos : litEndPrev;
                    sMl = end ? 0 : ml;
                    sOff = end ? 0 : off;
                    sK = 0;
                    sPieces = (sLit | sMl) != 0 ? sx::piece_count(sLit, sMl) : 0;
                    cLit = end ? 0 : lit;
                    cLitPos = litPos;
                }
            }
            uint64_t r8 = 0;
            if (finished == 0 && sK < sPieces) {  // one piece of at most 16 literal + 16 match bytes
                const int32_t skip = sLitPos - litEndPrev;
                if (sK == 0 && skip > sx::MAX_SKIP) {  // (a gap beyond the record field: kilobytes of length bytes) the wavefront decoder takes the item
                    fallback = 1;
                    finished = 1;
                }
                else {
                    r8 = sx::piece_record(sLit, sMl, sOff, sx::lit_full(sLit), sK, skip);  // (piece 0 alone carries the skip)
                    groupAny = 1;
                    sK++;
                    if (sK == sPieces) {
                        litEndPrev = sLitPos + sLit;
                    }
                }
            }
            rec[t] = r8;
        }
        K.flush(hdr, arena, maxChunks, lane, rec, groupAny, fallback, finished);
    }
    if (have) {
        sx::finish_block(a, hdr, meta, only, block, fallback != 0, K.firstChunk, K.count, w.st, w.eo, (int32_t)w.op);
    }
}

// the items a launch has are dealt round over its workgroups (a wavefront each)
__global__ __launch_bounds__(64) void lzo_decompress_wave_kernel(BatchArgs a)
{
    const int lane = threadIdx.x;
    for (int64_t block = blockIdx.x; block < a.nBlocks; block += gridDim.x) {  // (uniform)
        if (a.only != nullptr && uni(a.only[block]) == 0) {
            continue;
        }
        const uint8_t* __restrict__ in = a.srcBase + a.srcOff[block];
        uint8_t* out = a.dstBase + a.dstOff[block];
        const int32_t inLimit = uni(a.srcLen[block]);
        const int64_t outLimit = uni(a.dstCap[block]);
        lzod::Walk w;
        w.begin();
        for (;;) {  // (uniform: every lane reads the same bytes)
            int32_t ml = 0, off = 0, lit = 0, litPos = 0;
            const int r = uni(lzod::step(in, inLimit, outLimit, w, ml, off, lit, litPos));
            if (r == lzod::STEP_DONE) {
                break;
            }
            if (r == lzod::STEP_END) {
                continue;
            }
            ml = uni(ml);
            off = uni(off);
            lit = uni(lit);
            litPos = uni(litPos);
            const int32_t at = uni((int32_t)w.op) - lit - ml;
            if (ml != 0) {  // :256-320 (the bytes in front of `at` were stored by other lanes: group_match_copy begins with the ordering point)
                group_match_copy<64>(out, at, off, ml, lane);
            }
            if (lit != 0) {  // :322-347
                group_copy<64>(out + at + ml, in + litPos, lit, lane);
            }
        }
        wave_sync();
        if (lane == 0) {
            a.outLen[block] = w.st == 0 ? (int32_t)w.op : 0;
            a.status[block] = w.st;
            a.errOffset[block] = (int64_t)w.eo;
        }
    }
}

// a wavefront per item, at most what the chip holds at once
hipError_t launch_lzo_decompress_wave(const BatchArgs& a, hipStream_t stream)
{
    if (a.nBlocks <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(lzo_decompress_wave_kernel, dim3((unsigned)(a.nBlocks < 16384 ? a.nBlocks : 16384)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

namespace {
hipError_t lzo_rings(const BatchArgs& a, hipStream_t stream, int, int, const int32_t*) { return launch_lzo_decompress_wave(a, stream); }
}  // namespace

// parse to records, the record executor, the wavefront decoder for what the parser handed over
hipError_t launch_lzo_decompress_twopass(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int32_t maxChunks)
{
    if (maxChunks > 0) {  // (TwoPassLayout keeps one chunk to spare)
        const int64_t capped = sx::TwoPassLayout::fixed(a.nBlocks) + ((int64_t)maxChunks + 1) * (sx::CHUNK_SLOTS * 8);
        scratchBytes = capped < scratchBytes ? capped : scratchBytes;
    }
    return launch_twopass(a, stream, scratch, scratchBytes, 0, 0, nullptr, 1, 0, 12, lzo_parse2_kernel, lzo_parse2_kernel, lzo_rings);
}

}  // namespace achip
