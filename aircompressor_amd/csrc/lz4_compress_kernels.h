// lz4_compress_kernels.h -- the kernels of lz4_compress.hip (which has the design notes and the launchers).  Included TWICE, with no include guard:
//   LZ4K(name) = name,          LZ4K_PARAM empty,            LZ4K_ACCEL false, LZ4K_VALUE 1:      the kernels as they were before the acceleration parameter;
//   LZ4K(name) = name##_accel,  LZ4K_PARAM `, int32_t accel`, LZ4K_ACCEL true,  LZ4K_VALUE accel:  their twins with the search schedule of
//                                                                                                 Lz4Compressor.create(acceleration) (lz4_compress_body.h).
// One text, so the two cannot drift apart -- and the first expansion is, token for token, what this file's kernels were: acceleration 1 runs the instructions it
// ran before the parameter existed (tools/isa_diff.py says so; a shared inlined body did not achieve that: the same source behind one more level of inlining came
// out with another register assignment in all eight kernels).

template <typename TableT>
__global__ __launch_bounds__(64) void LZ4K(lz4_compress_kernel)(BatchArgs a, int32_t bothWidths LZ4K_PARAM)
{
    using namespace lz4c;
    __shared__ TableT table[MAX_TABLE_SIZE];
    const int lane = threadIdx.x;
    const int64_t block = blockIdx.x;
    const int32_t inLen = a.srcLen[block];
    constexpr bool WIDE = sizeof(TableT) == 4;
    // two launches cover a batch: u16 tables for blocks <= 64 KiB, i32 tables for the rest
    if (WIDE ? (inLen <= 65536) : (inLen > 65536)) {
        if (!bothWidths && lane == 0) {  // the caller's max_src_len_hint was wrong: say so instead of leaving the block's results unwritten
            a.outLen[block] = 0;
            a.status[block] = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
            a.errOffset[block] = 0;
        }
        return;
    }
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[block];
    uint8_t* __restrict__ out = a.dstBase + a.dstOff[block];
    const int32_t outCap = a.dstCap[block];

    int32_t output = 0;
    const int32_t st = lz4_block_status(inLen, outCap);
    if (st == 0) {
        const int32_t tableSize = lz4_table_init(inLen, table, lane);
        __syncthreads();
        const int32_t mask = tableSize - 1;

        const int32_t inputLimit = inLen;
        const int32_t matchFindLimit = inputLimit - MATCH_FIND_LIMIT;
        const int32_t matchLimit = inputLimit - LAST_LITERAL_SIZE;
        int32_t input = 0;
        int32_t anchor = 0;

        if (inLen >= MIN_LENGTH) {
            table[lz4_hash(ld8(in + input), mask)] = (TableT)input;  // every lane stores the same value: no cross-lane hazard
            input++;
            int32_t nextHash = lz4_hash(ld8(in + input), mask);

            bool done = false;
            do {
                int32_t nextInputIndex = input;
                int32_t findMatchAttempts = LZ4K_VALUE << SKIP_TRIGGER;  // :115
                int32_t step = 1;
                int32_t matchIndex;
                bool exhausted = false;
                for (;;) {  // :120-138
                    const int32_t hash = nextHash;
                    input = nextInputIndex;
                    nextInputIndex += step;
                    step = (int32_t)((uint32_t)(findMatchAttempts++) >> SKIP_TRIGGER);
                    if (nextInputIndex > matchFindLimit) {
                        exhausted = true;
                        break;
                    }
                    matchIndex = (int32_t)table[hash];
                    nextHash = lz4_hash(ld8(in + nextInputIndex), mask);
                    table[hash] = (TableT)input;
                    if (ld4(in + matchIndex) == ld4(in + input) && matchIndex + MAX_DISTANCE >= input) {
                        break;
                    }
                }
                if (exhausted) {
                    break;  // tail literals from anchor
                }

                // catch up :141-144
                while (input > anchor && matchIndex > 0 && in[input - 1] == in[matchIndex - 1]) {
                    --input;
                    --matchIndex;
                }

                int32_t literalLength = input - anchor;
                int32_t tokenPos = output;
                // emitLiteral :194-207 (token byte is written once the match length is known)
                int32_t litPos = tokenPos + lz4_run_length_size(literalLength);
                group_copy<64>(out + litPos, in + anchor, literalLength, lane);
                output = litPos + literalLength;

                for (;;) {  // :147-184
                    const int32_t matchLength = wave_count(in, input + MIN_MATCH, matchIndex + MIN_MATCH, matchLimit, lane);
                    output = lz4_emit_match(out, tokenPos, literalLength, input - matchIndex, matchLength, output, lane);

                    input += matchLength + MIN_MATCH;
                    anchor = input;
                    if (input > matchFindLimit) {
                        done = true;
                        break;
                    }

                    const int32_t position = input - 2;
                    const int32_t hp = lz4_hash(ld8(in + position), mask);
                    const int32_t hash = lz4_hash(ld8(in + input), mask);
                    table[hp] = (TableT)position;
                    matchIndex = (int32_t)table[hash];
                    table[hash] = (TableT)input;
                    if (matchIndex + MAX_DISTANCE < input || ld4(in + matchIndex) != ld4(in + input)) {
                        input++;
                        nextHash = lz4_hash(ld8(in + input), mask);
                        break;
                    }
                    // go for another match: zero-literal token
                    tokenPos = output++;
                    literalLength = 0;
                }
            } while (!done);
        }
        output = lz4_emit_last_literals(in, out, output, anchor, inputLimit, lane);  // (all three exits of the Java method end here)
    }

    if (lane == 0) {
        a.outLen[block] = st == 0 ? output : 0;
        a.status[block] = st;
        a.errOffset[block] = 0;
    }
}


// Batch-probe variant: the 64 lanes evaluate the next 64 steps of the Java search loop at once.
//   lane roles after a match (:157-184): lane 0 = the `input - 2` insert, lane 1 = the immediate re-probe at `input`,
//   lanes 2.. = the probes of the search that follows if the re-probe fails (:113-138, skip schedule included).
// Same-hash collisions inside the batch are resolved so that every probe sees exactly the table state the serial
// loop would have produced (a probe's candidate is the latest earlier batch position with the same hash, else the
// table entry); only the entries up to the winning probe are written back, latest position last.
template <typename TableT>
__global__ __launch_bounds__(64) void LZ4K(lz4_compress_batch_kernel)(BatchArgs a, int32_t bothWidths LZ4K_PARAM)
{
    using namespace lz4c;
    __shared__ TableT table[MAX_TABLE_SIZE];
    const int lane = threadIdx.x;
    const int64_t block = blockIdx.x;
    const int32_t inLen = a.srcLen[block];
    constexpr bool WIDE = sizeof(TableT) == 4;
    if (WIDE ? (inLen <= 65536) : (inLen > 65536)) {
        if (!bothWidths && lane == 0) {  // the caller's max_src_len_hint was wrong: say so instead of leaving the block's results unwritten
            a.outLen[block] = 0;
            a.status[block] = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
            a.errOffset[block] = 0;
        }
        return;
    }
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[block];
    uint8_t* __restrict__ out = a.dstBase + a.dstOff[block];
    const int32_t outCap = a.dstCap[block];

    int32_t st = 0;
    const int32_t output = lz4_compress_block<TableT, LZ4K_ACCEL>(in, inLen, out, outCap, table, lane, st, LZ4K_VALUE);
    if (lane == 0) {
        a.outLen[block] = st == 0 ? output : 0;
        a.status[block] = st;
        a.errOffset[block] = 0;
    }
}

// "Many matches per window" variant (lz4_compress_mw.h): the same parse, replayed over 64 consecutive positions held in registers.
template <typename TableT>
__global__ __launch_bounds__(64) void LZ4K(lz4_compress_mw_kernel)(BatchArgs a, int32_t bothWidths LZ4K_PARAM)
{
    using namespace lz4c;
    __shared__ TableT table[MAX_TABLE_SIZE];
    const int lane = threadIdx.x;
    const int64_t block = blockIdx.x;
    const int32_t inLen = a.srcLen[block];
    constexpr bool WIDE = sizeof(TableT) == 4;
    if (WIDE ? (inLen <= 65536) : (inLen > 65536)) {
        if (!bothWidths && lane == 0) {
            a.outLen[block] = 0;
            a.status[block] = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
            a.errOffset[block] = 0;
        }
        return;
    }
    const uint8_t* __restrict__ in = a.srcBase + a.srcOff[block];
    uint8_t* __restrict__ out = a.dstBase + a.dstOff[block];
    int32_t st = 0;
    const int32_t output = lz4_compress_block_mw<TableT, LZ4K_ACCEL>(in, inLen, out, a.dstCap[block], table, lane, st, LZ4K_VALUE);
    if (lane == 0) {
        a.outLen[block] = st == 0 ? output : 0;
        a.status[block] = st;
        a.errOffset[block] = 0;
    }
}

// Two tiers (round 6), the arrangement of snappy_compress_tiers_kernel for the 64 KiB blocks of this encoder.  The 8 KiB table allows twenty wavefronts a CU when
// it sits in LDS, the encoder is a serial chain per block whose wavefronts wait 42 % of their cycles (profiles/r06_counters_lz4_compress_corpus_after2.txt), and 72
// vector registers hold 28.  A workgroup here is FIVE wavefronts with their tables in LDS and up to two with theirs in a slab of global memory (8 KiB each: L2-resident)
// -- four workgroups a CU: the twenty LDS chains as before, and eight slower ones beside them.  Persistent; every wavefront draws its next block from a counter, so
// the slower chains simply take fewer.  (First shape tried: a workgroup of one LDS and one memory wavefront -- 14 + 14 chains a CU: corpus 38.9 -> 44.5 GiB/s,
// fragments 103.6 -> 71.6: on data whose searches run through windows the memory tier's table round trips are what a chain is made of.  profiles/r06_notes.md.)
// (Blocks beyond 64 KiB keep lz4_compress_mw_kernel<int32_t>.)
__global__ __launch_bounds__(64 * (lz4t::LDS_WAVES + lz4t::MEM_WAVES_MAX), 7) void LZ4K(lz4_compress_tiers_kernel)(BatchArgs a, int32_t bothWidths, uint16_t* slabs, int32_t* nextItem LZ4K_PARAM)
{
    using namespace lz4c;
    __shared__ uint16_t ldsTable[lz4t::LDS_WAVES][MAX_TABLE_SIZE];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint16_t* const slab = slabs + ((size_t)blockIdx.x * lz4t::MEM_WAVES_MAX + (wave >= lz4t::LDS_WAVES ? wave - lz4t::LDS_WAVES : 0)) * MAX_TABLE_SIZE;
    for (;;) {
        int32_t unit = 0;
        if (lane == 0) {
            unit = atomicAdd(nextItem, 1);
        }
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a.nBlocks) {
            return;
        }
        const int64_t block = unit;
        const int32_t inLen = uni(a.srcLen[block]);
        if (inLen > 65536) {
            if (!bothWidths && lane == 0) {
                a.outLen[block] = 0;
                a.status[block] = mk_status(ACHIP_CLASS_INVALID_ARGUMENT, ACHIP_D_BAD_ARGUMENT);
                a.errOffset[block] = 0;
            }
            continue;
        }
        const uint8_t* __restrict__ in = a.srcBase + a.srcOff[block];
        uint8_t* __restrict__ out = a.dstBase + a.dstOff[block];
        int32_t st = 0;
        int32_t output;
        if (wave < lz4t::LDS_WAVES) {
            output = lz4_compress_block_mw<uint16_t, LZ4K_ACCEL>(in, inLen, out, a.dstCap[block], ldsTable[wave], lane, st, LZ4K_VALUE);
        }
        else {
            output = lz4_compress_block_mw<uint16_t, LZ4K_ACCEL>(in, inLen, out, a.dstCap[block], slab, lane, st, LZ4K_VALUE);
        }
        if (lane == 0) {
            a.outLen[block] = st == 0 ? output : 0;
            a.status[block] = st;
            a.errOffset[block] = 0;
        }
        wave_mem_order();
    }
}

// ---- LZ4 frame container, encoder -------------------------------------------------------------
// Replaces Lz4FrameCompression.compress (M/lz4/Lz4FrameCompression.java:96-140): header (magic, FLG = version 01 +
// independent blocks, BD = 4 MiB, xxHash32 header checksum byte), 4 MiB blocks each through the block encoder above into a
// per-wave scratch slab, stored uncompressed when that is not smaller (:117-131), end mark.  One wavefront per item,
// persistent grid; the capacity checks are made where the Java code makes them (writeInt / ensureCapacity).

__global__ __launch_bounds__(64) void LZ4K(lz4frame_compress_kernel)(BatchArgs a, uint8_t* slabs, int32_t* nextItem LZ4K_PARAM)
{
    using namespace lz4c;
    __shared__ int32_t table[MAX_TABLE_SIZE];
    __shared__ int32_t item;
    const int lane = threadIdx.x;
    uint8_t* slab = slabs + (size_t)blockIdx.x * lz4f::SLAB_BYTES;
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
        const uint8_t* __restrict__ in = a.srcBase + a.srcOff[block];
        uint8_t* out = a.dstBase + a.dstOff[block];
        const int32_t inLen = a.srcLen[block];
        const int64_t outCap = a.dstCap[block];
        int64_t pos = 0;
        bool tooSmall = false;
        // frame header :102-107
        if (outCap < 7) {
            tooSmall = true;
        }
        else {
            if (lane == 0) {
                st4(out, 0x184D2204u);
                out[4] = 0x60;  // FLG_VERSION | FLG_BLOCK_INDEPENDENCE
                out[5] = 0x70;  // BD_4MB
                out[6] = 0x73;  // (xxHash32({0x60, 0x70}) >>> 8) & 0xFF
            }
            pos = 7;
        }
        int32_t ipos = 0;
        while (!tooSmall && ipos < inLen) {
            const int32_t blockLen = inLen - ipos < lz4f::BLOCK_MAX_4MB ? inLen - ipos : lz4f::BLOCK_MAX_4MB;
            int32_t st = 0;
            wave_mem_order();
            const int32_t clen = lz4_compress_block_mw<int32_t, LZ4K_ACCEL>(in + ipos, blockLen, slab, (int32_t)lz4f::SLAB_BYTES, table, lane, st, LZ4K_VALUE);
            wave_mem_order();
            const bool compressed = st == 0 && clen < blockLen;
            const int32_t payload = compressed ? clen : blockLen;
            if (pos + 4 > outCap || pos + 4 + payload > outCap) {
                tooSmall = true;
                break;
            }
            if (lane == 0) {
                st4(out + pos, compressed ? (uint32_t)clen : ((uint32_t)blockLen | 0x80000000u));
            }
            pos += 4;
            group_copy<64>(out + pos, compressed ? (const uint8_t*)slab : in + ipos, payload, lane);
            pos += payload;
            ipos += blockLen;
            __syncthreads();
        }
        if (!tooSmall) {
            if (pos + 4 > outCap) {
                tooSmall = true;
            }
            else {
                if (lane == 0) {
                    st4(out + pos, 0u);
                }
                pos += 4;
            }
        }
        if (lane == 0) {
            a.outLen[block] = tooSmall ? 0 : (int32_t)pos;
            a.status[block] = tooSmall ? mk_status(ACHIP_CLASS_OUTPUT_TOO_SMALL, ACHIP_D_LZ4F_MAX_OUTPUT) : 0;
            a.errOffset[block] = 0;
        }
    }
}
