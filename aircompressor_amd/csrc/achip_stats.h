// achip_stats.h -- what achip_ctx_get_stat reads out of the context's scratch: where each launcher's counters lie (the kernels and their launchers write by
// these names, the reader reads by them), the record of which launch left them there (LastLaunch), and the rule from a statistic's name to its value
// (locate).  A statistic kept in the scratch answers for the LAST launch that took the scratch and is -1 after any other.
// Plain C++17: no HIP, no device code (tests/test_stats_layout.py compiles it alone); achip_device.h includes it for the names.
#pragma once

#include <cstdint>
#include <cstring>

namespace achip {

// The block decoders' choice in auto mode (lz4_pick, achip_device.h; plan::auto_pick on the host): what decompress.choice reports and achip_ctx::autoChoice remembers.
constexpr int LZ4_PICK_RINGS = 0, LZ4_PICK_TWOPASS = 3;

namespace stats {

// ---- the Zstd pipeline's counter block: the first ZSTD_COUNTER_BYTES of its scratch, as 32-bit words (zstd_decompress_pipe.hip) ----
constexpr int ZSTD_FALLBACK_ITEMS = 0;                        // items handed to the one-kernel decoder
constexpr int ZSTD_SEQ_CURSOR = 16, ZSTD_LIT_CURSOR = 17;     // a tile's sequence and literal arena cursors ...
constexpr int ZSTD_LONG_ITEMS = 18;                           // ... and its count of long-sequence items (the three are cleared together per tile)
constexpr int ZSTD_STAGE = 32, ZSTD_STAGES = 6;               // ZSTD_STAGE + s, s = 1 .. ZSTD_STAGES: items handed over by stage s (6: the multi-block stages' walk)
constexpr int ZSTD_MB_ITEMS = 40, ZSTD_MB_BLOCKS = 41, ZSTD_MB_FAST_ITEMS = 42;  // items K1 listed for the multi-block stages, their blocks, items those stages finished
constexpr int ZSTD_COUNTER_BYTES = 256;
constexpr int ZSTD_STEP_CURSORS_AT = 256;                     // the stream steps' layout: a second cursor pair (sequence, literal) at this byte, behind the counter block

// ---- auto mode's probe statistics: the first words of the block decoders' scratch (decode_probes.hip writes, lz4_pick and plan::auto_pick read) ----
constexpr int PROBE_MIXED_GROUPS = 0;    // groups of 16 blocks whose compressed sizes differ by more than 2x
constexpr int PROBE_SEQUENCES = 1;       // sequences parsed from the heads of the sampled blocks ...
constexpr int PROBE_BYTES4 = 2;          // ... and the bytes they produce, in units of 4
constexpr int PROBE_HAS_RECORDS = 3;     // != 0: the caller has record scratch (the two passes are a candidate)
constexpr int PROBE_SHORT_BLOCKS = 4;    // sampled blocks of short sequences ...
constexpr int PROBE_SAMPLED_BLOCKS = 5;  // ... of this many sampled blocks (0: not counted)
constexpr int PROBE_WORDS = 6;
constexpr int PROBE_LEAD_BYTES = 4096;   // the probes' page: in auto mode the two-pass layout starts behind it

// ---- the two-pass decoders' arena header (sx::ArenaHeader, achip_seqexec.h, which asserts the offset) ----
constexpr int ARENA_FALLBACK_BLOCKS = 2;

// What the last launch that took the context's scratch left at its head.  Whoever hands the scratch to a launch clears this first (take_scratch,
// abi_dispatch.cpp); a launcher that leaves statistics then says so.
struct LastLaunch {
    enum Kind { Nothing, BlockDecode, LzoDecode, ZstdDecode };
    Kind kind = Nothing;
    int32_t blocks = 0;       // BlockDecode (what the probes saw), ZstdDecode: the batch's items
    int32_t shortLimit = 0;   // BlockDecode: its codec family's (BlockCodec::shortLimit; 12 LZ4, 6 Snappy)
    bool probes = false;      // BlockDecode: auto mode's probes ran; their statistics lead the scratch
    bool twopass = false;     // BlockDecode, LzoDecode: the two passes ran; their arena header lies ...
    int32_t twopassLead = 0;  // ... this many bytes into the scratch
    int remembered = -1;      // BlockDecode: the one decoder launched on a remembered choice (LZ4_PICK_*), -1: none
    int variant = 0;          // ZstdDecode: 0 the one-kernel decoder (no counters), else the pipeline

    static LastLaunch block_decode(int32_t blocks, int32_t shortLimit, bool probes, bool twopass, int remembered)
    {
        LastLaunch l;
        l.kind = BlockDecode;
        l.blocks = blocks;
        l.shortLimit = shortLimit;
        l.probes = probes;
        l.twopass = twopass;
        l.twopassLead = probes ? PROBE_LEAD_BYTES : 0;
        l.remembered = remembered;
        return l;
    }
    static LastLaunch lzo_decode(bool twopass)
    {
        LastLaunch l;
        l.kind = LzoDecode;
        l.twopass = twopass;
        return l;
    }
    static LastLaunch zstd_decode(int32_t blocks, int variant)
    {
        LastLaunch l;
        l.kind = ZstdDecode;
        l.blocks = blocks;
        l.variant = variant;
        return l;
    }
};

// Where a statistic is.  words == 0: `value` is the answer (-1: unknown name, or the last launch left no such statistic).  Else: read `words` words at byte
// `byteOffset` of the scratch; the answer is word `word` of them -- or, with `pick`, plan::auto_pick(them, pickBlocks, pickShortLimit).
struct Located {
    int64_t value = -1;
    int64_t byteOffset = 0;
    int words = 0, word = 0;
    bool pick = false;
    int32_t pickBlocks = 0, pickShortLimit = 0;
};

inline Located constant(int64_t value)
{
    Located at;
    at.value = value;
    return at;
}
inline Located word_at(int64_t byteOffset, int word)
{
    Located at;
    at.byteOffset = byteOffset;
    at.words = word + 1;
    at.word = word;
    return at;
}

inline Located locate(const LastLaunch& last, const char* name)
{
    const Located none;
    auto is = [&](const char* k) { return strcmp(name, k) == 0; };
    if (is("lz4.decompress.mixed_groups")) {  // auto mode's probe count of the last LZ4 / Snappy decode
        return last.kind == LastLaunch::BlockDecode && last.probes ? word_at(0, PROBE_MIXED_GROUPS) : none;
    }
    if (is("decompress.choice")) {  // which decoder auto mode ran: LZ4_PICK_RINGS, LZ4_PICK_TWOPASS
        if (last.kind != LastLaunch::BlockDecode) return none;
        if (last.remembered >= 0) return constant(last.remembered);  // (decompress.auto_remember)
        if (!last.probes) return none;
        Located at = word_at(0, PROBE_WORDS - 1);
        at.pick = true;
        at.pickBlocks = last.blocks;
        at.pickShortLimit = last.shortLimit;
        return at;
    }
    if (is("decompress.twopass_fallback_blocks")) {  // blocks the last two-pass LZ4 / Snappy decode handed to the ring decoder
        return last.kind == LastLaunch::BlockDecode && last.twopass ? word_at(last.twopassLead, ARENA_FALLBACK_BLOCKS) : none;
    }
    if (is("lzo.decompress.fallback_blocks")) {  // items of the last LZO decode whose records did not fit the arena: the wavefront decoder took them
        if (last.kind != LastLaunch::LzoDecode) return none;
        return last.twopass ? word_at(0, ARENA_FALLBACK_BLOCKS) : constant(0);
    }
    const char* const zstd = "zstd.decompress.";
    if (strncmp(name, zstd, strlen(zstd)) != 0) return none;
    const char* what = name + strlen(zstd);
    // the pipeline's counters lead its scratch.  The one-kernel decoder has none: every item is a "fallback" item, of no stage
    int word = -1;
    bool oneKernelKnows = false;
    if (strcmp(what, "fallback_items") == 0) {
        word = ZSTD_FALLBACK_ITEMS;
        oneKernelKnows = true;
    }
    else if (strncmp(what, "fallback_stage", 14) == 0 && what[14] >= '1' && what[14] <= '0' + ZSTD_STAGES && what[15] == 0) {
        word = ZSTD_STAGE + (what[14] - '0');
        oneKernelKnows = true;
    }
    else if (strcmp(what, "multiblock_items") == 0) word = ZSTD_MB_ITEMS;
    else if (strcmp(what, "multiblock_blocks") == 0) word = ZSTD_MB_BLOCKS;
    else if (strcmp(what, "multiblock_fast_items") == 0) word = ZSTD_MB_FAST_ITEMS;
    else if (strcmp(what, "long_items") == 0) word = ZSTD_LONG_ITEMS;  // (of the last tile)
    if (word < 0 || last.kind != LastLaunch::ZstdDecode) return none;
    if (last.variant == 0) return oneKernelKnows ? constant(word == ZSTD_FALLBACK_ITEMS ? last.blocks : 0) : none;
    return word_at(4 * (int64_t)word, 0);
}

}  // namespace stats
}  // namespace achip
