// achip_settings.h -- what achip_ctx_set_option sets: a context's settings as one copyable value, and the table of options that fills it.
// Plain C++ without HIP: tests/test_options.py compiles it with g++ and checks every option's accepted values.
#pragma once
#include <cstdint>
#include <cstring>

namespace achip {

// The settings the launchers read (achip_launch.h): per context, passed to every launch.
struct KernelSettings {
    int lz4Parse = 0;     // lz4.decompress.parse: the two-pass decoder's parser -- 0 by the batch, 1 a lane per block, 2 a wavefront per block (lz4_decompress_v7.hip)
    int snappyParse = 0;  // snappy.decompress.parse: likewise (snappy_decompress_v5.hip)
    int zstdExec = 2;     // zstd.decompress.exec: the Zstd pipeline's execute stage -- 2 chosen per item, 1 the record executor, 0 the rings
    int zstdSeqWaves = 1;    // zstd.decompress.seq_waves: wavefronts per workgroup of the pipeline's sequence stage
    int zstdLitItems = 13;   // zstd.decompress.lit_items: items per wavefront of the pipeline's literal stage
    int zstdSeqSpread = 256;  // the CUs a small tile of the sequence stage is spread over (no option; tools/hostemu sets 1 to get full workgroups from a handful of items)
    // lz4.compress.mem_waves: 0 = one wavefront per block, table in LDS (until round 6); 1 / 2 = memory-tier wavefronts beside five LDS ones.
    // Measured, 65 536 blocks (profiles/r06_ab_lz4_compress_tiers.txt): corpus 38.8 / **44.1** / 41.3 GiB/s at 0 / 1 / 2, fragments 103.6 / 104.8 / 93.0
    int lz4MemWaves = 1;
    int lz4TierMinBlocks = 256 * 20;  // lz4.compress.tier_min_blocks: batches of at least this many blocks take the two-tier kernel (what the LDS tier holds at once)
    int lz4TierWorkgroups = 0;        // the two-tier LZ4 kernel's grid (no option; 0: lz4t::WORKGROUPS, tools/hostemu makes it small)
    // Lz4Compressor.create(acceleration), 1 .. 65537 (no option: achip_ctx_set_lz4_acceleration -- a property of the compressor object, not a tuning knob): the LZ4
    // block and LZ4 frame encoders' search advances by this many positions per probe from its second probe on.  Above 1 the launchers take the `_accel` kernels.
    int lz4Acceleration = 1;
    // LZ4 frames whose block-independence bit is clear (what liblz4's frame API writes at its defaults), 0 or 1 (no option: achip_ctx_set_lz4frame_linked_blocks --
    // a property of the reader object; nothing in the reference, whose reader refuses them): 1 = every LZ4 frame decode and the LZ4FRAME line of the size query
    // read such frames, a block's matches reaching up to 65 535 bytes into the frame's content in front of it; 0 = ACHIP_D_LZ4F_LINKED_BLOCKS, as the Java reader.
    int lz4fLinkedBlocks = 0;
    // snappy.compress.mem_waves: wavefronts of a workgroup whose table lies in memory (0 .. 3).  Their tables are what the kernel's HBM traffic is made of -- 431 GB
    // a launch on the corpus batch, 100 x the input: 1 280 workgroups x 3 slabs x 32 KiB = 120 MB of tables, 15 MB per XCD against 4 MB of L2.
    int snappyMemWaves = 3;
    int snappyTierWorkgroups = 256 * 5;  // the persistent grid where the unit count is known on the device only (no option; tools/hostemu makes it small)
    // SnappyFramedOutputStream(compressor, out, writeChecksums, blockSize, minCompressionRatio) and SnappyFramedInputStream(decompressor, in, verifyChecksums)
    // (no options: achip_ctx_set_snappyframed_writer / _verify_checksums -- properties of the stream objects, not tuning knobs).  Every x-snappy-framed encode of
    // the context cuts its input at snfBlockSize (1 .. 65536), keeps a chunk compressed at compressed / length <= the double whose bits snfMinRatioBits holds
    // (0.85), and writes the masked CRC-32C or 0; every x-snappy-framed decode compares the CRC field or skips the CRC pass altogether.
    int snfWriteChecksums = 1;
    int snfBlockSize = 65536;
    int64_t snfMinRatioBits = 0x3FEB333333333333LL;
    int snfVerifyChecksums = 1;
    int snfEncodeWorkgroups = 0;  // the block-list writer's persistent encode grid (no option; 0: 768, tools/hostemu makes it small)
    int snfListEntries = 0;  // entries of the x-snappy-framed writer's block list (no option; 0: lists::CAPACITY, tools/hostemu makes it small: streams beyond it take the serial kernel)
    // The LZ4 frame writer's frame descriptor (no options: achip_ctx_set_lz4frame_writer -- properties of the writer object; nothing in the reference, whose writer
    // has one shape, M/lz4/Lz4FrameCompression.java:98-132): the block-maximum size (64 KiB, 256 KiB, 1 MiB, 4 MiB: BD ids 4 .. 7) and whether a frame carries
    // block checksums, a content checksum, its content size.  At (4 MiB, 0, 0, 0) with lz4frame.compress.variant 0 every LZ4 frame encode is the wavefront-per-frame
    // kernel as it was; anything else takes the block-list writer (lz4_frame_writer.hip), which asks bound::lz4frame_list of dstCap.
    int lz4fBlockMaxSize = 4 << 20;
    int lz4fBlockChecksum = 0;
    int lz4fContentChecksum = 0;
    int lz4fContentSize = 0;
    int lz4fCompressVariant = 0;   // lz4frame.compress.variant: 0 = by the settings above, 1 = the block-list writer at the default settings too
    int lz4fEncodeWorkgroups = 0;  // the block-list writer's persistent encode grid (no option; 0: 2560, tools/hostemu makes it small)
    int lz4fListEntries = 0;       // entries of its block list (no option; 0: lists::CAPACITY, tools/hostemu makes it small: a frame beyond it is refused)
};

// achip_ctx_set_lz4frame_writer's checks, in the order of its arguments: the block-maximum size must be one of the format's four, then each flag 0 or 1.  set_ stores
// only what passed all four: a refused call leaves `ks` as it was.
enum class Lz4fRefusal { None, BlockMaxSize, BlockChecksum, ContentChecksum, ContentSize };
inline Lz4fRefusal check_lz4f_writer(int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize)
{
    if (blockMaxSize != 65536 && blockMaxSize != 262144 && blockMaxSize != 1048576 && blockMaxSize != 4194304) return Lz4fRefusal::BlockMaxSize;
    if (blockChecksum != 0 && blockChecksum != 1) return Lz4fRefusal::BlockChecksum;
    if (contentChecksum != 0 && contentChecksum != 1) return Lz4fRefusal::ContentChecksum;
    if (contentSize != 0 && contentSize != 1) return Lz4fRefusal::ContentSize;
    return Lz4fRefusal::None;
}
inline const char* lz4f_refusal_text(Lz4fRefusal r)
{
    switch (r) {
        case Lz4fRefusal::BlockMaxSize: return "blockMaxSize must be 65536, 262144, 1048576 or 4194304";
        case Lz4fRefusal::BlockChecksum: return "blockChecksum must be 0 or 1";
        case Lz4fRefusal::ContentChecksum: return "contentChecksum must be 0 or 1";
        case Lz4fRefusal::ContentSize: return "contentSize must be 0 or 1";
        case Lz4fRefusal::None: break;
    }
    return "";
}
inline Lz4fRefusal set_lz4f_writer(KernelSettings& ks, int32_t blockMaxSize, int32_t blockChecksum, int32_t contentChecksum, int32_t contentSize)
{
    const Lz4fRefusal r = check_lz4f_writer(blockMaxSize, blockChecksum, contentChecksum, contentSize);
    if (r == Lz4fRefusal::None) {
        ks.lz4fBlockMaxSize = blockMaxSize;
        ks.lz4fBlockChecksum = blockChecksum;
        ks.lz4fContentChecksum = contentChecksum;
        ks.lz4fContentSize = contentSize;
    }
    return r;
}
// which LZ4 frame writer a launch takes: the block list unless everything is at its default
inline bool lz4f_list_writer(const KernelSettings& ks)
{
    return ks.lz4fCompressVariant != 0 || ks.lz4fBlockMaxSize != (4 << 20) || ks.lz4fBlockChecksum != 0 || ks.lz4fContentChecksum != 0 || ks.lz4fContentSize != 0;
}

// achip_ctx_set_snappyframed_writer's checks, in the order of SnappyFramedOutputStream's constructor (M/snappy/SnappyFramedOutputStream.java:83, :90): the ratio
// (its IEEE-754 bits) must be > 0 and <= 1.0 -- NaN fails --, then the block size must be in (0, 65536], then the flag 0 or 1.  set_ stores only what passed all
// three: a refused call leaves `ks` as it was.
enum class SnfRefusal { None, Ratio, BlockSize, Flag };
inline double snf_ratio(int64_t bits)
{
    double ratio;
    static_assert(sizeof(ratio) == sizeof(bits), "a double is 64 bits");
    memcpy(&ratio, &bits, sizeof(ratio));
    return ratio;
}
inline SnfRefusal check_snf_writer(int32_t writeChecksums, int32_t blockSize, int64_t minRatioBits)
{
    const double ratio = snf_ratio(minRatioBits);
    if (!(ratio > 0 && ratio <= 1.0)) return SnfRefusal::Ratio;
    if (blockSize <= 0 || blockSize > 65536) return SnfRefusal::BlockSize;
    if (writeChecksums != 0 && writeChecksums != 1) return SnfRefusal::Flag;
    return SnfRefusal::None;
}
inline SnfRefusal set_snf_writer(KernelSettings& ks, int32_t writeChecksums, int32_t blockSize, int64_t minRatioBits)
{
    const SnfRefusal r = check_snf_writer(writeChecksums, blockSize, minRatioBits);
    if (r == SnfRefusal::None) {
        ks.snfWriteChecksums = writeChecksums;
        ks.snfBlockSize = blockSize;
        ks.snfMinRatioBits = minRatioBits;
    }
    return r;
}
// achip_ctx_set_lz4frame_linked_blocks: 0 or 1; a refused value leaves `ks` as it was
inline bool set_lz4f_linked_blocks(KernelSettings& ks, int32_t accept)
{
    if (accept != 0 && accept != 1) return false;
    ks.lz4fLinkedBlocks = accept;
    return true;
}
inline SnfRefusal set_snf_verify(KernelSettings& ks, int32_t verify)
{
    if (verify != 0 && verify != 1) return SnfRefusal::Flag;
    ks.snfVerifyChecksums = verify;
    return SnfRefusal::None;
}

// Everything achip_ctx_set_option writes.  A mixed batch's helper contexts take a copy of their caller's (abi_dispatch.cpp: mix_lane).
struct Settings {
    int lz4dGroup = 0;       // ring decoder, lanes per block: 0 = by the batch size (4 from 32 768 blocks on -- the headline's form --, 16 below, 64 up to 4 096: lz4_ring_group_for), else 1 .. 64
    int snappydGroup = 0;    // likewise (64 up to 2 048 blocks, 16 below 16 384, 4 above: snappy_ring_group_for)
    int lzodVariant = 0;           // LZO decode: 0 auto (by the batch size: lzodAutoMinBlocks), 1 two passes (lzo_parse2_kernel + the record executor), 2 a wavefront per item (lzo_decompress.hip)
    int lzodAutoMinBlocks = 8192;  // ... auto runs the two passes from this many items on (provisional -- one run, profiles/lzo_rate.txt: on text the two decoders cross between 4 096 and 16 384 blocks)
    int lzodMaxChunks = 0;         // ... the two passes use at most this many 4 KiB chunks of the record arena (0: all the scratch has; a test aid, not a tuning knob)
    int lz4dAutoMinBlocks = 4096;  // auto mode probes batches from this size on (smaller ones always take the rings)
    int lz4dVariant = 5;     // 5 = chosen on the device per batch (default: DESIGN 4c), 1 = LDS rings, a lane group per block (lz4_decompress_v2.hip), 7 = two passes: parse to records + a wavefront per block (lz4_decompress_v7.hip).  (4 / 6, a lane per block, lost to 7 on every batch they were built for -- 300 .. 330 GiB/s against 515 on corpus -- and were removed in round 4.)
    int snappydVariant = 5;  // 5 auto, 1 rings (snappy_decompress_v2.hip), 7 two passes (snappy_decompress_v5.hip), as for LZ4
    int latencyMaxBlocks = 256;  // batches of at most this many blocks (a single block!) take the ring decoders' latency class: a wavefront and 128 KiB of LDS history per block
    int ringClass = 0;       // 0 = compact rings, 1 = large rings
    int lz4cVariant = 4;     // 4 = many matches per window of 64 positions (lz4_compress_mw.h; default since round 3: 25.8 against 18.2 GiB/s on corpus, 100 against 111 on fragments), 0 = serial probes, 1 = 64 probes per step (batch).  (3, the batch over an LDS input window, measured 17.2 against 18.2 GiB/s on corpus in round 3: removed)
    int snappycVariant = 4;  // THE DEFAULT IS 4 = two tiers, many matches per window (snappy_compress_mw.h; since round 3: 22.0 against 8.3 GiB/s on corpus, 65 against 74 on fragments); tested non-default variants: 0 = serial probes, 1 = 64 probes per step (batch), 2 = batch in two tiers: tables in LDS and in global memory.  (3, variant 2 over an LDS input window, measured 8.3 against 7.6 GiB/s for 2 and a third of variant 4: removed in round 4.)
    int zstddVariant = 1;  // 1 = five-stage pipeline (+ one-kernel decoder for its fallback list), 0 = one-kernel decoder only
    int zstdcVariant = 3;  // match kernel in window form (zstd_dfast_mw.h) + entropy kernel
    int hadoopBufferSize = 262144;        // Hadoop block streams: the streams' buffer size (Lz4HadoopStreams.java:30; io.compression.codec.*.buffersize)
    int lz4FrameDecompressVariant = 2;    // 2 = chosen per call by a probe of the sequence lengths (default: 75 / 13.4 GiB/s on fragments / corpus frames); 0 = a wavefront per item (75 / 7.8); 1 = the frames' blocks as one batch through the two-pass block decoder (22 / 13.4)
    int hadoopDecompressVariant = 3;      // 3 = chunk list, the block decoder chosen per call by a probe of the sequence lengths (default); 1 = always the rings; 2 = always the two-pass decoders; 0 = one wavefront per stream (profiles/r03_notes.md)
    int snappyFramedCompressVariant = 1;  // framed writer: 1 = block list + two-tier block encoder + compaction (default), 0 = one wavefront per stream
    int snappyFramedVariant = 3;  // framed reader: 3 = chunk list, the block decoder chosen per call by a probe of the element lengths (default); 1 = always the rings; 2 = always the two-pass decoder; 0 = one wavefront per stream
    int zstdTile = 65536;    // items per pass of the Zstd decode pipeline (halved automatically when its scratch cannot be allocated)
    int zstdStreamChunked = 1;     // 1: the stream writer takes streams from 4 MiB on as well (chunks flushed before close(), window slides: zstd_stream.hip; byte-identical with
                                   // the test suite's CPU restatement under tools/hostemu, not yet run on a GPU); 0: it refuses them (INVALID_ARGUMENT / ACHIP_D_UNSUPPORTED)
    int zstdStreamBlocks = 65536;  // 128 KiB blocks a pass of the pipeline's multi-block stages has room for (0: multi-block frames take the one-kernel decoder); ~20 GB of scratch, allocated when a batch first holds such frames (halved as often as it takes when the device cannot give that)
    int ringPad = 80;        // 64 bytes of far-match staging + 16: consecutive blocks start on different LDS banks
    int scratchPoison = -1;
    int autoRemember = 1;    // decompress.auto_remember (abi_dispatch.cpp: auto_remembered)
    int maxSrcLenHint = 0;
    int snappyFan = 1;     // snappy.compress.fan: 1 = the sub-blocks of buffers beyond 64 KiB are work units of their own (default), 0 = a buffer is one wavefront's work
    int mixConcurrent = 1;   // mixed batches: 1 = the three codec families side by side, each on a stream (and scratch) of its own -- a bucket's tail is a few long
                             // serial chains on a few CUs (a 10 MB file as ONE block: 0.4 s of one wavefront) --, 0 = every bucket in turn on the context's stream
    // host-pointer batches (achip_batch_host / achip_mixed_batch_host)
    int hostLookMaxBlocks = 0;  // host.look_max_blocks: chunks of up to this many blocks have their first tokens looked at on the host (long sequences: the rings at 64 lanes)
    int hostCopyLowPriority = 1;  // host.copy_priority: 1 = the pipeline's copy streams at the lowest stream priority (to be set before the first host-pointer batch)
    int hostRamp = 1;  // host.ramp: 1 = smaller chunks at a batch's start and end (default), 0 = chunks of host.chunk_bytes throughout
    int hostSlots = 8;  // host.slots: staging slots the host-pointer pipeline uses (2 .. achip_ctx::kHostSlots; round 6: 8 -- with 4 the gather thread waited for a slot 20 of a call's 34 ms)
    int hostBlit = 0;          // host.blit: bit 0 = the pipeline's uploads by a copy kernel instead of hipMemcpyAsync, bit 1 = its downloads
    int hostBlitGroups = 128;  // host.blit_groups: workgroups of that kernel
    int64_t hostChunkBytes = 192 << 20;   // staging bytes (inputs + output capacities) per pipeline chunk: ~2000 blocks of 64 KiB -- a chunk's kernels
                                         // take a block's serial chain (~1-2 ms) however few blocks it holds, so a chunk must be worth that long on the
                                         // link.  Round 6 (profiles/r06_hostsweep.txt, r06_host_timeline.txt): with eight slots, the copy streams at the lowest
                                         // priority and smaller chunks at both ends 192 MiB gives 40-42 GiB/s where round 5's 96 MiB over four slots gave 26-30
                                         // on the same box (the 48 MiB of rounds 1-4 over two slots: 8.7)
    int hostCopyThreads = 0;             // per copy pool; 0 = hardware threads / 16, 2 .. 8 (4 and 8 measured best; 32 no better: the scatter is
                                         // bound by the host's memory system, not by the thread count)
    KernelSettings kernel;
};

// The values an option accepts.
struct Accepted {
    enum Kind { Any, Flag, Range, Pow2, OneOf } kind;  // Flag: any value, stored as 0 or 1
    int64_t lo = 0, hi = 0, step = 1;  // Range: lo .. hi in steps of `step`; Pow2: the powers of two in lo .. hi
    bool zero = false;                 // 0 as well
    int64_t list[5] = {};              // OneOf
    int count = 0;

    bool operator()(int64_t v) const
    {
        if (zero && v == 0) return true;
        switch (kind) {
            case Any:
            case Flag: return true;
            case Range: return v >= lo && v <= hi && (v - lo) % step == 0;
            case Pow2: return v >= lo && v <= hi && (v & (v - 1)) == 0;
            case OneOf:
                for (int i = 0; i < count; i++) {
                    if (list[i] == v) return true;
                }
                return false;
        }
        return false;
    }
};
constexpr Accepted any_value() { return {Accepted::Any}; }
constexpr Accepted flag() { return {Accepted::Flag}; }
constexpr Accepted range(int64_t lo, int64_t hi, int64_t step = 1) { return {Accepted::Range, lo, hi, step}; }
constexpr Accepted pow2(int64_t lo, int64_t hi) { return {Accepted::Pow2, lo, hi}; }
template <class... V>
constexpr Accepted one_of(V... v)
{
    Accepted a{Accepted::OneOf};
    ((a.list[a.count++] = v), ...);
    return a;
}
constexpr Accepted or_zero(Accepted a)
{
    a.zero = true;
    return a;
}

// Where an option's value goes: a field of Settings or of its KernelSettings (none: the option only validates).
struct Field {
    int Settings::*ctx = nullptr;
    int64_t Settings::*wide = nullptr;
    int KernelSettings::*kernel = nullptr;
    constexpr Field() = default;
    constexpr Field(int Settings::*f) : ctx(f) {}
    constexpr Field(int64_t Settings::*f) : wide(f) {}
    constexpr Field(int KernelSettings::*f) : kernel(f) {}
};

struct Option {
    const char* name;
    Field field;
    Accepted accepted;
    const char* refusal;  // the error text of a value it does not accept
};

// Every option achip_ctx_set_option knows (DESIGN.md 8b documents them: tests/test_docs.py).  Special cases of achip_ctx_set_option itself:
// host.copy_threads once the host-pointer pipeline exists, decompress.auto_remember (clears the remembered choices).
inline const Option kOptions[] = {
    {"lz4.decompress.group", &Settings::lz4dGroup, pow2(1, 64), "group size must be a power of two in 1..64"},
    {"snappy.decompress.group", &Settings::snappydGroup, or_zero(pow2(1, 64)), "snappy.decompress.group: 0 (by the batch size) or a power of two in 1..64"},
    {"lz4.decompress.variant", &Settings::lz4dVariant, one_of(1, 5, 7), "lz4.decompress.variant: 1 rings, 7 two passes, 5 auto"},
    {"lz4.decompress.auto_min_blocks", &Settings::lz4dAutoMinBlocks, range(16, 0x7FFFFFFF), "lz4.decompress.auto_min_blocks must be at least 16"},
    {"snappy.decompress.variant", &Settings::snappydVariant, one_of(1, 5, 7), "snappy.decompress.variant: 1 rings, 7 two passes, 5 auto"},
    {"decompress.ring_class", &Settings::ringClass, range(0, 2), "decompress.ring_class: 0 compact (4 lanes per block: phased), 1 large, 2 round-2 compact rings (4 lanes per block)"},
    {"lz4.compress.variant", &Settings::lz4cVariant, one_of(0, 1, 4), "lz4.compress.variant: 0 serial probes, 1 batch probes, 4 many matches per window"},
    {"snappy.compress.variant", &Settings::snappycVariant, one_of(0, 1, 2, 4), "snappy.compress.variant: 0 serial probes, 1 batch probes, 2 two tiers, 4 two tiers, many matches per window"},
    {"snappyframed.decompress.variant", &Settings::snappyFramedVariant, range(0, 3), "snappyframed.decompress.variant: 0 a wavefront per stream, 1 chunk list through the ring decoders, 2 through the two-pass decoder, 3 chosen by a probe"},
    {"snappyframed.compress.variant", &Settings::snappyFramedCompressVariant, range(0, 1), "snappyframed.compress.variant: 0 a wavefront per stream, 1 block list"},
    {"hadoop.buffer_size", &Settings::hadoopBufferSize, range(64, 0x40000000), "hadoop.buffer_size out of range"},
    {"hadoop.decompress.variant", &Settings::hadoopDecompressVariant, range(0, 3), "hadoop.decompress.variant: 0 a wavefront per stream, 1 chunk list through the ring decoders, 2 through the two-pass decoders, 3 chosen by a probe"},
    {"lz4frame.decompress.variant", &Settings::lz4FrameDecompressVariant, range(0, 2), "lz4frame.decompress.variant: 0 a wavefront per item, 1 block list through the two-pass decoder, 2 chosen by a probe"},
    {"lz4.decompress.parse", &KernelSettings::lz4Parse, range(0, 2), "lz4.decompress.parse: 0 by the batch (a wavefront per block below 32768 blocks), 1 a lane per block, 2 a wavefront per block"},
    {"mixed.concurrent", &Settings::mixConcurrent, range(0, 1), "mixed.concurrent: 1 a mixed batch's codec families side by side (a stream and scratch each), 0 every bucket in turn"},
    {"snappy.decompress.parse", &KernelSettings::snappyParse, range(0, 2), "snappy.decompress.parse: 0 by the batch (a wavefront per block up to 4096 blocks), 1 a lane per block, 2 a wavefront per block"},
    {"zstd.decompress.exec", &KernelSettings::zstdExec, range(0, 2), "zstd.decompress.exec: 0 rings, 1 record executor, 2 chosen per item"},
    {"zstd.decompress.seq_waves", &KernelSettings::zstdSeqWaves, one_of(1, 2, 4), "zstd.decompress.seq_waves: wavefronts per workgroup of the pipeline's sequence stage: 1, 2 or 4 (64 items a workgroup either way)"},
    {"zstd.decompress.lit_items", &KernelSettings::zstdLitItems, one_of(8, 10, 13, 16, 20), "zstd.decompress.lit_items: items per wavefront of the pipeline's literal stage: 8, 10 or 16 (4 KiB of LDS an item), 13 (3 KiB: symbols and length nibbles apart), 20 (16 items of 2 304 bytes: symbols, and lengths by symbol)"},
    {"decompress.latency_max_blocks", &Settings::latencyMaxBlocks, range(0, 65536), "decompress.latency_max_blocks: 0 (never) .. 65536: LZ4 / Snappy batches of at most this many blocks take a wavefront and 128 KiB of LDS history per block"},
    {"decompress.ring_pad", &Settings::ringPad, range(0, 256, 16), "ring pad must be a multiple of 16 in 0..256"},
    {"zstd.decompress.tile", &Settings::zstdTile, range(64, 65536), "tile must be in 64..65536"},
    {"debug.scratch_poison", &Settings::scratchPoison, any_value(), ""},
    {"zstd.decompress.variant", &Settings::zstddVariant, range(0, 1), "zstd.decompress.variant: 1 pipeline, 0 one-kernel decoder"},
    {"zstd.stream.chunked", &Settings::zstdStreamChunked, flag(), ""},
    {"zstd.decompress.stream_blocks", &Settings::zstdStreamBlocks, or_zero(range(16, 131072)), "zstd.decompress.stream_blocks must be 0 or 16..131072"},
    {"zstd.compress.variant", &Settings::zstdcVariant, range(0, 3), "zstd.compress.variant: 3 match-finder kernel (many matches per window) + entropy kernel, 0 the same with batch probes, 1 with serial probes, 2 one kernel"},
    {"host.look_max_blocks", &Settings::hostLookMaxBlocks, range(0, 65536), "host.look_max_blocks: 0 .. 65536"},
    {"host.copy_priority", &Settings::hostCopyLowPriority, range(0, 1), "host.copy_priority: 1 the host-pointer pipeline's copy streams at the lowest priority (default), 0 at the default priority"},
    {"decompress.auto_remember", &Settings::autoRemember, range(0, 1), "decompress.auto_remember: 1 auto mode launches only the decoder the last arrived probe statistics chose for batches of that shape (default), 0 both decoders in every call"},
    {"host.ramp", &Settings::hostRamp, range(0, 1), "host.ramp: 1 smaller chunks at the start and the end of a host-pointer batch (default), 0 equal chunks"},
    {"host.slots", &Settings::hostSlots, range(2, 8), "host.slots: 2 .. 8 staging slots of the host-pointer pipeline"},
    {"host.blit", &Settings::hostBlit, range(0, 3), "host.blit: bit 0 = the host-pointer pipeline's uploads by a copy kernel, bit 1 = its downloads (0 = both by hipMemcpyAsync)"},
    {"host.blit_groups", &Settings::hostBlitGroups, range(1, 4096), "host.blit_groups: 1 .. 4096 workgroups of the copy kernel"},
    {"max_src_len_hint", &Settings::maxSrcLenHint, any_value(), ""},
    {"lz4.compress.mem_waves", &KernelSettings::lz4MemWaves, range(0, 2), "lz4.compress.mem_waves: wavefronts per workgroup of the window encoder whose table lies in memory: 0 (one wavefront per block, table in LDS), 1 or 2"},
    {"lz4.compress.tier_min_blocks", &KernelSettings::lz4TierMinBlocks, range(1, 1 << 30), "lz4.compress.tier_min_blocks: batches of at least this many blocks take the two-tier kernel (default 5120)"},
    {"snappy.compress.mem_waves", &KernelSettings::snappyMemWaves, range(0, 3), "snappy.compress.mem_waves: wavefronts per workgroup of the two-tier encoder whose table lies in memory, 0 .. 3"},
    {"snappy.compress.fan", &Settings::snappyFan, range(0, 1), "snappy.compress.fan: 1 the independent 64 KiB sub-blocks of a buffer side by side (default), 0 in turn on one wavefront"},
    // 2: the two-pass decoders' one executor.  (Round 2's experiments and timing aids -- 121 .. 125, 201, 302 .. 308 -- were measured, then removed: rounds 3 and 4.)
    {"decompress.exec_variant", {}, one_of(2), "decompress.exec_variant: 2"},
    {"host.chunk_bytes", &Settings::hostChunkBytes, range(1 << 16, 1LL << 32), "host.chunk_bytes must be in 64 KiB .. 4 GiB"},
    {"host.copy_threads", &Settings::hostCopyThreads, range(0, 64), "host.copy_threads must be in 0..64"},
};

// Options that came after that table was frozen against the parser it replaced (tests/test_options.py holds kOptions to that parser's names and values); DESIGN.md 8b
// documents them below its table.
inline const Option kLaterOptions[] = {
    {"lzo.decompress.variant", &Settings::lzodVariant, range(0, 2), "lzo.decompress.variant: 0 auto, 1 two passes, 2 a wavefront per item"},
    {"lzo.decompress.auto_min_blocks", &Settings::lzodAutoMinBlocks, range(1, 0x7FFFFFFF), "lzo.decompress.auto_min_blocks must be at least 1"},
    {"lzo.decompress.max_chunks", &Settings::lzodMaxChunks, range(0, 0x7FFFFFFF), "lzo.decompress.max_chunks must not be negative"},
    {"lz4frame.compress.variant", &KernelSettings::lz4fCompressVariant, range(0, 1), "lz4frame.compress.variant: 0 the writer the context's frame settings ask for (a wavefront per frame at the defaults), 1 the block-list writer at the default settings too"},
};

enum class Applied { Ok, Unknown, BadValue };

// One option applied to `s`.
inline Applied apply_option(Settings& s, const Option& o, int64_t value, const char** refusal)
{
    if (!o.accepted(value)) {
        if (refusal) *refusal = o.refusal;
        return Applied::BadValue;
    }
    const int64_t v = o.accepted.kind == Accepted::Flag ? (value != 0 ? 1 : 0) : value;
    if (o.field.ctx) s.*o.field.ctx = (int)v;
    if (o.field.wide) s.*o.field.wide = v;
    if (o.field.kernel) s.kernel.*o.field.kernel = (int)v;
    return Applied::Ok;
}

// Sets option `name` of `s` to `value`.  BadValue leaves `s` as it was and points `*refusal` (if given) at the option's error text.
inline Applied apply(Settings& s, const char* name, int64_t value, const char** refusal = nullptr)
{
    for (const Option& o : kOptions) {
        if (strcmp(o.name, name) == 0) return apply_option(s, o, value, refusal);
    }
    for (const Option& o : kLaterOptions) {
        if (strcmp(o.name, name) == 0) return apply_option(s, o, value, refusal);
    }
    return Applied::Unknown;
}

}  // namespace achip
