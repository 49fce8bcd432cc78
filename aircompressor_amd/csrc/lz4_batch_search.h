// lz4_batch_search.h -- the batch-probe search loop of one block by one wavefront (M/lz4/Lz4RawCompressor.java:113-184, M/lzo/LzoRawCompressor.java:120-195: the
// same loop), as TEXT: included inside a function body, with no include guard, by lz4_compress_block (lz4_compress_body.h) and lzo_compress_block (lzo_compress.hip).
// One text, so a fix to the batch schedule is made once -- and the LZ4 expansion is, token for token, what lz4_compress_block held (tools/isa_diff.py says so; a shared
// inlined function is known not to achieve that: lz4_compress_kernels.h).
// In scope at the include: in, out, table, mask, hashBits, matchFindLimit, matchLimit, accel, lane, output, anchor; `using namespace lz4c`.  The includer defines
//   BATCH_SEARCH_PROBE(role, pos, k)   the lz4_probe_step call (table type, acceleration form, farthest candidate)
//   BATCH_SEARCH_EMIT_STATE            declarations in front of a sequence's emit calls
//   BATCH_SEARCH_EMIT_LITERALS         the literal run [anchor, input) in front of a match (behind catch-up)
//   BATCH_SEARCH_EMIT_NO_LITERALS      the re-probe right behind a match hit: a match without a literal run
//   BATCH_SEARCH_EMIT_MATCH            the match of matchLength + MIN_MATCH bytes at input - matchIndex
// and undefines them behind the include.
            // mode 0: block start (lane 0 inserts position 0, search starts at 1); mode 1: after a match; mode 2: search continues
            int mode = 0;
            int32_t input = 0;      // mode 1: position right after the last match
            int32_t scanStart = 1;  // position of probe 0 of the current search
            int32_t k0 = 0;         // first probe index of this batch (mode 2)
            int width = 64;          // lanes used by a batch (a narrow first batch of 8 was measured slower on MI355X: profiles/r01_notes.md)
            for (;;) {
                // ---- roles and positions ----
                int role = 0;  // 0 idle, 1 insert only, 2 probe
                int32_t pos = 0;
                int32_t k = -1;  // search probe index (>= 0 for search probes; -1 for the insert / re-probe lanes)
                if (mode == 0) {
                    if (lane == 0) {
                        role = 1;
                        pos = 0;
                    }
                    else {
                        role = 2;
                        k = lane - 1;
                    }
                }
                else if (mode == 1) {
                    if (lane == 0) {
                        role = 1;
                        pos = input - 2;
                    }
                    else if (lane == 1) {
                        role = 2;
                        pos = input;
                    }
                    else {
                        role = 2;
                        k = lane - 2;
                    }
                }
                else {
                    role = 2;
                    k = k0 + lane;
                }
                if (lane >= width) {
                    role = 0;
                    k = -1;
                }
                const Lz4ProbeStep s = BATCH_SEARCH_PROBE(role, pos, k);
                __syncthreads();

                if (s.winner < 0) {
                    if (s.firstInvalid < 64) {
                        break;  // search ran off the end: last literals from anchor
                    }
                    // no match in this batch: the search goes on
                    const int32_t probes = mode == 0 ? width - 1 : (mode == 1 ? width - 2 : width);
                    k0 = (mode == 2 ? k0 : 0) + probes;
                    mode = 2;
                    width = 64;
                    continue;
                }
                input = __shfl(s.pos, s.winner);
                int32_t matchIndex = __shfl(s.cand, s.winner);
                const bool reprobe = mode == 1 && s.winner == 1;

                BATCH_SEARCH_EMIT_STATE
                if (!reprobe) {
                    lz4_catch_up_mem(in, input, matchIndex, input - anchor < matchIndex ? input - anchor : matchIndex, lane);
                    BATCH_SEARCH_EMIT_LITERALS
                }
                else {
                    BATCH_SEARCH_EMIT_NO_LITERALS
                }
                const int32_t matchLength = wave_count(in, input + MIN_MATCH, matchIndex + MIN_MATCH, matchLimit, lane);
                BATCH_SEARCH_EMIT_MATCH
                input += matchLength + MIN_MATCH;
                anchor = input;
                if (input > matchFindLimit) {
                    break;  // :152-155
                }
                mode = 1;
                scanStart = input + 1;
                k0 = 0;
                width = 64;
            }
