// abi_dispatch.cpp -- from an entry point of the device-resident API to kernel launches: the context's scratch and who may grow it how, the choice of the
// LZ4 / Snappy block decoder (launch_block_decode) with auto mode's memory, one switch over the codec ops (launch_op), and the entry points over them: the
// per-codec batches, the mixed batch, decoded sizes / output planner / compress bounds / pack.
#include "achip_host.h"

using namespace achip::host;
using achip::BlockCodec;
using achip::kBlockCodecs;

namespace achip {
namespace host ACHIP_HIDDEN {

// frees what is there FIRST (the device may have room for one of the two, not both), then allocates
int32_t ensure_scratch(achip_ctx* ctx, int64_t bytes)
{
    if (bytes <= ctx->scratchBytes) {
        return 0;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->scratch) {
        HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
        ctx->scratchBytes = 0;
        HIP_TRY(ctx->scratch.reset());
    }
    const hipError_t e = ctx->scratch.alloc((size_t)bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // not sticky: the caller may retry with a smaller request
        return device_failure("hipMalloc(scratch)", e);
    }
    ctx->scratchBytes = bytes;
    return 0;
}

// bytes > what is there: allocates the larger buffer, then -- only then -- frees the old one.  Non-zero (and nothing changed) when the device
// cannot hold both.
int32_t grow_scratch_keeping_old(achip_ctx* ctx, int64_t bytes)
{
    if (bytes <= ctx->scratchBytes) {
        return 0;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceBuffer<> fresh;
    if (fresh.alloc((size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    if (ctx->scratch) {
        const hipError_t s = hipStreamSynchronize(ctx->stream.get());
        if (s != hipSuccess) {
            return device_failure("hipStreamSynchronize", s);
        }
    }
    ctx->scratch = std::move(fresh);  // (frees the old one)
    ctx->scratchBytes = bytes;
    return 0;
}

// The one way to the context's scratch for a launch.  The launch will write over what the last one left at the scratch's head, so the record of that
// (ctx->last: what achip_ctx_get_stat goes by) ends here and nowhere else; a launcher that leaves statistics of its own sets it afterwards.  Grows by
// ensure_scratch (bytes 0: as it is -- launch_op, whose cases grow it by their own policies).
int32_t take_scratch(achip_ctx* ctx, int64_t bytes)
{
    ctx->last = {};
    return ensure_scratch(ctx, bytes);
}

// scratch of the Zstd pipeline's multi-block stages (achip::ZstdMbProvider::get; the stream is idle when the stages ask)
void* zstd_mb_scratch(void* user, int64_t bytes)
{
    achip_ctx* ctx = (achip_ctx*)user;
    if (bytes <= ctx->zstdMbScratchBytes) {
        return ctx->zstdMbScratch.get();
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        return nullptr;
    }
    ctx->zstdMbScratchBytes = 0;
    if (ctx->zstdMbScratch.alloc((size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    ctx->zstdMbScratchBytes = bytes;
    return ctx->zstdMbScratch.get();
}

}  // namespace host
}  // namespace achip

namespace {

// LZ4 and Snappy block decoding: one policy (launch_block_decode) over the row of its codec family in achip::kBlockCodecs (achip_launch.h) -- 0 LZ4, 1 Snappy.

// Auto mode's memory (achip_ctx::autoPinned ...).  auto_remembered: the decoder to launch alone for this batch (LZ4_PICK_RINGS or LZ4_PICK_TWOPASS), or -1: launch both.  First takes
// in what an earlier call sent home, if it has arrived (an event query, never a wait).
int auto_remembered(achip_ctx* ctx, int fam, const achip::BatchArgs& a)
{
    if (ctx->autoInFlight && hipEventQuery(ctx->autoEv.get()) == hipSuccess) {
        const int pf = ctx->autoPendingFam;
        ctx->autoChoice[pf] = achip::plan::auto_pick(ctx->autoPinned.get(), ctx->autoPendingBlocks, kBlockCodecs[pf].shortLimit);
        ctx->autoBlocks[pf] = ctx->autoPendingBlocks;
        ctx->autoSrc[pf] = ctx->autoPendingSrc;
        ctx->autoDst[pf] = ctx->autoPendingDst;
        ctx->autoInFlight = false;
    }
    else if (ctx->autoInFlight) {
        (void)hipGetLastError();  // (hipErrorNotReady is not an error)
    }
    if (ctx->autoRemember == 0 || ctx->autoChoice[fam] < 0 || a.nBlocksDev != nullptr || a.only != nullptr) return -1;
    if (ctx->autoBlocks[fam] != a.nBlocks || ctx->autoSrc[fam] != (const void*)a.srcBase || ctx->autoDst[fam] != (const void*)a.dstBase) return -1;
    return ctx->autoChoice[fam];
}
// behind a call's kernels: its probe statistics on their way to pinned memory (nothing waits for them; one set in flight at a time)
void auto_send_home(achip_ctx* ctx, int fam, const achip::BatchArgs& a, const int32_t* stats)
{
    if (ctx->autoRemember == 0 || ctx->autoInFlight || a.nBlocksDev != nullptr || a.only != nullptr) return;
    if (!ctx->autoPinned) {
        if (ctx->autoPinned.alloc(64) != hipSuccess || ctx->autoEv.create() != hipSuccess) {
            (void)hipGetLastError();
            (void)ctx->autoPinned.reset();
            ctx->autoRemember = 0;  // (no memory for it: both decoders in every call)
            return;
        }
    }
    if (hipMemcpyAsync(ctx->autoPinned.get(), stats, 32, hipMemcpyDeviceToHost, ctx->stream.get()) != hipSuccess || hipEventRecord(ctx->autoEv.get(), ctx->stream.get()) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    ctx->autoInFlight = true;
    ctx->autoPendingFam = fam;
    ctx->autoPendingBlocks = a.nBlocks;
    ctx->autoPendingSrc = a.srcBase;
    ctx->autoPendingDst = a.dstBase;
}

// The two-pass decoders' scratch (lead bytes of probe statistics + header, meta and record arena): the full arena (`perBlock` bytes of
// records per block) if the device has it to spare -- never more than half of what is free right now beyond what the context already
// holds, so that one large batch does not take the device from its other users --, else what is there down to `perBlockMin` (blocks whose
// records do not fit are decoded by the ring decoder: the parse kernels hand them over per block).  Returns 1 with the scratch in
// place, 0 when not even the minimum could be had -- the caller then runs the ring decoder alone, which needs no scratch: a batch that
// decoded before the two-pass decoders existed still decodes on a busy device -- and < 0 for an error that is not about memory.
int32_t ensure_twopass_scratch(achip_ctx* ctx, int64_t lead, int32_t nBlocks, int64_t perBlock, int64_t perBlockMin)
{
    const int64_t want = lead + achip::twopass_scratch_bytes(nBlocks, perBlock);
    if (want <= ctx->scratchBytes) {
        return 1;
    }
    const int64_t atLeast = lead + achip::twopass_scratch_bytes(nBlocks, perBlockMin);
    HIP_TRY(hipSetDevice(ctx->device));
    size_t freeB = 0, totalB = 0;
    int64_t ask = want;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
        const int64_t room = ctx->scratchBytes + (int64_t)(freeB / 2);
        ask = std::min(want, std::max(room, atLeast));
    }
    else {
        (void)hipGetLastError();
    }
    if (ask <= ctx->scratchBytes) {
        return ctx->scratchBytes >= atLeast ? 1 : 0;
    }
    // Grow WITHOUT giving up what is there: the new buffer is allocated first and the old one freed only when that worked, so a
    // context never loses a working scratch to a failed request.  Only a context whose scratch is below the minimum anyway lets it go and
    // asks again (the device may have room for one of the two, not both).
    if (grow_scratch_keeping_old(ctx, ask) == 0) {
        return 1;
    }
    if (ask > atLeast && ctx->scratchBytes < atLeast && grow_scratch_keeping_old(ctx, atLeast) == 0) {
        return 1;
    }
    if (ctx->scratchBytes >= atLeast) {
        g_lastError.clear();
        return 1;  // what is there serves (fewer records per block: more blocks go to the ring decoder -- decompress.twopass_fallback_blocks)
    }
    if (ensure_scratch(ctx, atLeast) == 0) {  // (frees the old scratch first)
        return 1;
    }
    g_lastError.clear();
    return 0;
}

int32_t launch_block_decode(achip_ctx* ctx, const achip::BatchArgs& a, int fam, int variant, int group)
{
    const BlockCodec& c = kBlockCodecs[fam];
    const int groupSize = group > 0 ? group : (a.nBlocksDev != nullptr ? 4 : c.groupFor(a.nBlocks));
    auto launched = [](hipError_t e) { return e != hipSuccess ? device_failure("kernel launch", e) : 0; };
    if (variant == 5 && a.nBlocks >= ctx->lz4dAutoMinBlocks) {
        // auto: the choice is made on the device (no host round trip): probes count the mixed 16-block groups and sample the
        // sequence lengths, every candidate decoder is launched and the ones not chosen return at once.  Mixed or short-sequence
        // batches go to the two-pass decoder (parse to records + a wavefront per block), the rest to the rings.
        // scratch: [probe statistics: the first PROBE_LEAD_BYTES][two-pass header, meta, arena]
        constexpr int64_t lead = achip::stats::PROBE_LEAD_BYTES;
        const int32_t r = ensure_twopass_scratch(ctx, lead, a.nBlocks, c.recordBytes, c.recordBytesMin);
        if (r < 0) return r;
        if (r == 0) {  // no room for records on this device right now: the rings alone
            return launched(c.rings(a, ctx->stream.get(), groupSize, ctx->ringClass, nullptr));
        }
        int32_t* stats = (int32_t*)ctx->scratch.get();
        const int remembered = auto_remembered(ctx, fam, a);
        const bool rings = remembered != achip::LZ4_PICK_TWOPASS, twopass = remembered != achip::LZ4_PICK_RINGS;
        ctx->last = achip::stats::LastLaunch::block_decode(a.nBlocks, c.shortLimit, true, twopass, remembered);
        hipError_t e = achip::launch_lz4_mixed_groups(a, ctx->stream.get(), stats, 0);
        if (e == hipSuccess) e = hipMemsetAsync(stats + achip::stats::PROBE_HAS_RECORDS, 1, 1, ctx->stream.get());  // = 1: the two-pass scheme (achip_device.h lz4_pick)
        if (e == hipSuccess) e = c.sample(a, ctx->stream.get(), stats, 0, c.shortLimit);
        // (remembered: that decoder alone and whatever this call's probes say -- they are for the calls to come)
        if (e == hipSuccess && rings) e = c.rings(a, ctx->stream.get(), groupSize, ctx->ringClass, twopass ? stats : nullptr);
        if (e == hipSuccess && twopass) {
            e = c.twopass(a, ctx->stream.get(), (uint8_t*)ctx->scratch.get() + lead, ctx->scratchBytes - lead, groupSize, ctx->ringClass, rings ? stats : nullptr, ctx->kernel);
        }
        if (e == hipSuccess) auto_send_home(ctx, fam, a, stats);
        return launched(e);
    }
    // FEW blocks (at most decompress.latency_max_blocks; a single block is the literal Lz4HipDecompressor.decompress): nothing hides a lone block's chain,
    // so the choice is by what one 64 KiB block costs (profiles/r05_single_block_latency.txt): long sequences -- the ring decoders' latency class
    // (0.64 ms; the two passes 1.0); short ones or unknown -- the two passes with the wavefront-per-block parser (text 1.3 ms; the latency class 5.1;
    // Snappy: one 64 KiB text block 7.2 ms with a lane parsing it)
    // ... and so does every batch below the size auto mode probes from (4 096): such a batch of LARGE blocks -- files as single blocks, a frame's 4 MiB blocks --
    // is the compact rings' worst case (four lanes per block, 83 % of a text block's matches a memory round trip each: the 263-item LZ4 bucket of the mixed corpus batch
    // took 526 ms, its two largest files alone through the two passes 80), and on long sequences the two passes cost about what the rings do at these sizes
    const bool fewBlocks = variant == 5 && a.nBlocks < ctx->lz4dAutoMinBlocks && a.nBlocksDev == nullptr && a.only == nullptr;
    const int hint = ctx->smallBatchHint;
    ctx->smallBatchHint = 0;
    if (variant == 7 || (fewBlocks && hint != 2)) {  // two passes: parse to records, a wavefront per block executes them (lz4_decompress_v7.hip, snappy_decompress_v5.hip)
        const int32_t r = ensure_twopass_scratch(ctx, 0, a.nBlocks, achip::plan::few_blocks_record_bytes(a.nBlocks, c.recordBytes), c.recordBytesMin);
        if (r < 0) return r;
        if (r == 0) {
            return launched(c.rings(a, ctx->stream.get(), groupSize, ctx->ringClass, nullptr));
        }
        ctx->last = achip::stats::LastLaunch::block_decode(a.nBlocks, c.shortLimit, false, true, -1);
        return launched(c.twopass(a, ctx->stream.get(), ctx->scratch.get(), ctx->scratchBytes, groupSize, ctx->ringClass, nullptr, ctx->kernel));
    }
    return launched(c.rings(a, ctx->stream.get(), groupSize, ctx->ringClass == 0 && a.nBlocks <= ctx->latencyMaxBlocks ? 3 : ctx->ringClass, nullptr));
}

}  // namespace

namespace achip {
namespace host ACHIP_HIDDEN {

int32_t launch_op(int32_t op, achip_ctx* ctx, const achip::BatchArgs& args)
{
    if (!ctx) {
        return bad_argument("ctx is null");
    }
    achip::BatchArgs a = args;
    a.ringPad = ctx->ringPad;
    if (op == ACHIP_OP_ZSTD_COMPRESS) a.ringPad = ctx->zstdcVariant == 1 ? 1 : (ctx->zstdcVariant == 3 ? 3 : 0);  // the encoder variant rides in the spare field
    if (a.nBlocks < 0) {
        return bad_argument("nBlocks < 0");
    }
    if (a.nBlocks == 0) {
        return 0;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipSuccess;
    // Whatever the op: this launch is the context's last one now, and the scratch is its to write (the cases grow it by their own policies -- ensure_scratch,
    // grow_scratch_keeping_old, ensure_twopass_scratch over the two).  The four launchers that leave statistics say so once they have it.
    if (const int32_t r = take_scratch(ctx, 0); r < 0) return r;
    switch (op) {
        case ACHIP_OP_LZ4_DECOMPRESS: return launch_block_decode(ctx, a, 0, ctx->lz4dVariant, ctx->lz4dGroup);
        case ACHIP_OP_SNAPPY_DECOMPRESS: return launch_block_decode(ctx, a, 1, ctx->snappydVariant, ctx->snappydGroup);
        case ACHIP_OP_LZ4_COMPRESS: {
            // the two-tier kernel's table slabs, for a batch that takes it (the launcher takes it only with this scratch in hand)
            const achip::KernelSettings& ks = ctx->kernel;
            if (ctx->lz4cVariant == 4 && ks.lz4MemWaves > 0 && a.nBlocks >= ks.lz4TierMinBlocks) {
                if (const int32_t r = ensure_scratch(ctx, achip::lz4_compress_scratch_bytes()); r < 0) return r;
            }
            e = achip::launch_lz4_compress(a, ctx->stream.get(), ctx->lz4cVariant, ctx->maxSrcLenHint, ctx->scratch.get(), ctx->scratchBytes, ks);
            break;
        }
        case ACHIP_OP_SNAPPY_COMPRESS: {
            if (ctx->snappycVariant >= 2) {
                if (const int32_t r = ensure_scratch(ctx, achip::snappy_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            }
            // (buffers beyond 64 KiB: their independent sub-blocks side by side -- unless the caller, or the host-pointer path that has seen the lengths, says there are none)
            e = achip::launch_snappy_compress(a, ctx->stream.get(), ctx->snappycVariant, ctx->scratch.get(), ctx->snappyFan != 0 && !(ctx->maxSrcLenHint > 0 && ctx->maxSrcLenHint <= 65536), ctx->kernel);
            break;
        }
        case ACHIP_OP_ZSTD_DECOMPRESS: {
            // pipeline scratch scales with the tile (items per pass, <= 65536: ~17 GB); when the device cannot give that much,
            // smaller tiles are tried before giving up (the one-kernel decoder's 270 MB are always part of it)
            int32_t r = ensure_scratch(ctx, achip::zstd_decompress_scratch_bytes(a.nBlocks, ctx->zstdTile));
            while (r < 0 && ctx->zstdTile > 1024 && ctx->zstdTile >= a.nBlocks / 64) {
                ctx->zstdTile /= 2;
                r = ensure_scratch(ctx, achip::zstd_decompress_scratch_bytes(a.nBlocks, ctx->zstdTile));
            }
            if (r < 0) return r;
            const achip::ZstdMbProvider mbp{zstd_mb_scratch, ctx, ctx->zstdStreamBlocks};
            ctx->last = achip::stats::LastLaunch::zstd_decode(a.nBlocks, ctx->zstddVariant);
            e = achip::launch_zstd_decompress(a, ctx->stream.get(), ctx->scratch.get(), ctx->scratchBytes, ctx->zstddVariant, ctx->zstdTile, ctx->zstdStreamBlocks >= 16 ? &mbp : nullptr, ctx->kernel);
            break;
        }
        case ACHIP_OP_LZ4FRAME_DECOMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::lz4frame_decompress_scratch_bytes(a.nBlocks, ctx->lz4FrameDecompressVariant)); r < 0) return r;
            const achip::AuxScratch aux{zstd_mb_scratch, ctx};
            e = achip::launch_lz4frame_decompress(a, ctx->stream.get(), ctx->scratch.get(), ctx->lz4FrameDecompressVariant, &aux, ctx->kernel);
            break;
        }
        case ACHIP_OP_SNAPPYFRAMED_DECOMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::snappyframed_decompress_scratch_bytes(a.nBlocks)); r < 0) return r;
            const achip::AuxScratch aux{zstd_mb_scratch, ctx};
            e = achip::launch_snappyframed_decompress(a, ctx->stream.get(), ctx->scratch.get(), ctx->snappyFramedVariant, &aux, ctx->kernel);
            break;
        }
        case ACHIP_OP_SNAPPYFRAMED_COMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::snappyframed_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            e = achip::launch_snappyframed_compress(a, ctx->stream.get(), ctx->scratch.get(), ctx->snappyFramedCompressVariant, ctx->kernel);
            break;
        }
        case ACHIP_OP_LZ4HADOOP_DECOMPRESS:
        case ACHIP_OP_SNAPPYHADOOP_DECOMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::hadoop_decompress_scratch_bytes(a.nBlocks, ctx->hadoopBufferSize)); r < 0) return r;
            const achip::AuxScratch aux{zstd_mb_scratch, ctx};  // (the context's second, lazily grown buffer: shared with the Zstd multi-block stages)
            e = achip::launch_hadoop_decompress(a, ctx->stream.get(), ctx->scratch.get(), op == ACHIP_OP_SNAPPYHADOOP_DECOMPRESS, ctx->hadoopBufferSize, ctx->hadoopDecompressVariant, &aux, ctx->kernel);
            break;
        }
        case ACHIP_OP_LZ4HADOOP_COMPRESS:
        case ACHIP_OP_SNAPPYHADOOP_COMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::hadoop_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            e = achip::launch_hadoop_compress(a, ctx->stream.get(), ctx->scratch.get(), op == ACHIP_OP_SNAPPYHADOOP_COMPRESS, ctx->hadoopBufferSize);
            break;
        }
        case ACHIP_OP_LZ4FRAME_COMPRESS: {
            if (achip::lz4f_list_writer(ctx->kernel)) {  // any frame setting but the Java writer's, or lz4frame.compress.variant 1: the block list
                if (const int32_t r = ensure_scratch(ctx, achip::lz4frame_list_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
                e = achip::launch_lz4frame_list_compress(a, ctx->stream.get(), ctx->scratch.get(), ctx->kernel);
                break;
            }
            // a slab per resident wavefront; when the device cannot give the full set the launch runs with fewer wavefronts
            if (grow_scratch_keeping_old(ctx, achip::lz4frame_compress_scratch_bytes(a.nBlocks, false)) != 0) {
                g_lastError.clear();
                if (const int32_t r = ensure_scratch(ctx, achip::lz4frame_compress_scratch_bytes(a.nBlocks, true)); r < 0) return r;
            }
            e = achip::launch_lz4frame_compress(a, ctx->stream.get(), ctx->scratch.get(), ctx->scratchBytes, ctx->kernel.lz4Acceleration);
            break;
        }
        case ACHIP_OP_ZSTDSTREAM_COMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::zstd_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            e = achip::launch_zstd_stream_compress(a, ctx->stream.get(), ctx->scratch.get(), ctx->zstdStreamChunked);
            break;
        }
        case ACHIP_OP_ZSTD_COMPRESS: {
            if (const int32_t r = ensure_scratch(ctx, achip::zstd_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            if (ctx->scratchPoison >= 0) {  // debugging aid: expose reads of uninitialised scratch
                HIP_TRY(hipMemsetAsync(ctx->scratch.get(), ctx->scratchPoison, (size_t)ctx->scratchBytes, ctx->stream.get()));
            }
            e = achip::launch_zstd_compress(a, ctx->stream.get(), ctx->scratch.get(), ctx->scratchBytes, ctx->zstdcVariant);
            break;
        }
        case ACHIP_OP_LZO_DECOMPRESS: {
            // auto: batches below lzo.decompress.auto_min_blocks (and the `only` lists and device-counted batches no caller has for this op) run a wavefront per
            // item -- nothing hides a lane's serial walk when there are not items for every lane of the chip --, larger ones the two passes.  The line (8 192) is
            // from profiles/lzo_rate.txt: the two passes cost the same 16 .. 19 ms of a text batch whatever its count, the wavefront decoder 12.5 ms at 4 096 blocks and 34.5 at 16 384
            const bool twopass = ctx->lzodVariant == 1 || (ctx->lzodVariant == 0 && a.nBlocks >= ctx->lzodAutoMinBlocks);
            if (twopass) {
                const int32_t r = ensure_twopass_scratch(ctx, 0, a.nBlocks, achip::LZ4_RECORD_BYTES_PER_BLOCK, achip::LZ4_RECORD_BYTES_PER_BLOCK_MIN);
                if (r < 0) return r;
                if (r > 0) {
                    ctx->last = achip::stats::LastLaunch::lzo_decode(true);
                    e = achip::launch_lzo_decompress_twopass(a, ctx->stream.get(), ctx->scratch.get(), ctx->scratchBytes, ctx->lzodMaxChunks);
                    break;
                }
            }
            ctx->last = achip::stats::LastLaunch::lzo_decode(false);
            e = achip::launch_lzo_decompress_wave(a, ctx->stream.get());
            break;
        }
        case ACHIP_OP_LZO_COMPRESS: e = achip::launch_lzo_compress(a, ctx->stream.get()); break;
        default: return bad_argument("unknown codecOp");
    }
    if (e != hipSuccess) {
        return device_failure("kernel launch", e);
    }
    return 0;
}

}  // namespace host
}  // namespace achip

extern "C" {

// ---- batched device-resident API ----------------------------------------
#define ACHIP_DEFINE_BATCH(fn, op)                                                                                      \
    int32_t fn(ACHIP_BATCH_ARGS)                                                                                        \
    {                                                                                                                   \
        return launch_op(op, ctx, make_args(srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks)); \
    }
ACHIP_DEFINE_BATCH(achip_lz4_decompress_batch, ACHIP_OP_LZ4_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_lz4_compress_batch, ACHIP_OP_LZ4_COMPRESS)
ACHIP_DEFINE_BATCH(achip_snappy_decompress_batch, ACHIP_OP_SNAPPY_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_snappy_compress_batch, ACHIP_OP_SNAPPY_COMPRESS)
ACHIP_DEFINE_BATCH(achip_zstd_decompress_batch, ACHIP_OP_ZSTD_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_zstd_compress_batch, ACHIP_OP_ZSTD_COMPRESS)
ACHIP_DEFINE_BATCH(achip_lz4frame_decompress_batch, ACHIP_OP_LZ4FRAME_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_lz4frame_compress_batch, ACHIP_OP_LZ4FRAME_COMPRESS)
ACHIP_DEFINE_BATCH(achip_snappyframed_decompress_batch, ACHIP_OP_SNAPPYFRAMED_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_snappyframed_compress_batch, ACHIP_OP_SNAPPYFRAMED_COMPRESS)
ACHIP_DEFINE_BATCH(achip_lz4hadoop_decompress_batch, ACHIP_OP_LZ4HADOOP_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_lz4hadoop_compress_batch, ACHIP_OP_LZ4HADOOP_COMPRESS)
ACHIP_DEFINE_BATCH(achip_snappyhadoop_decompress_batch, ACHIP_OP_SNAPPYHADOOP_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_snappyhadoop_compress_batch, ACHIP_OP_SNAPPYHADOOP_COMPRESS)
ACHIP_DEFINE_BATCH(achip_zstdstream_compress_batch, ACHIP_OP_ZSTDSTREAM_COMPRESS)
ACHIP_DEFINE_BATCH(achip_lzo_decompress_batch, ACHIP_OP_LZO_DECOMPRESS)
ACHIP_DEFINE_BATCH(achip_lzo_compress_batch, ACHIP_OP_LZO_COMPRESS)

// ---- mixed batch: bucket by codec op, run every op over its slice, un-bucket (BASELINE configs[4]) ----
namespace {
int32_t ensure_mix(achip_ctx* ctx, int64_t n)
{
    if (n <= ctx->mixItems) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    ctx->mixItems = 0;
    const int64_t want = std::max<int64_t>(n, 4096);
    HIP_TRY(ctx->mixHost.reset());
    HIP_TRY(ctx->mixDev.reset());
    HIP_TRY(ctx->mixHost.alloc((size_t)(want * 4)));
    HIP_TRY(ctx->mixDev.alloc((size_t)(want * 48 + 256)));
    if (!ctx->mixUploaded) HIP_TRY(ctx->mixUploaded.create());
    ctx->mixItems = want;
    return 0;
}
constexpr int kMixFamilies = 3;  // LZ4 (block, frame, Hadoop; LZO), Snappy (block, framed, Hadoop), Zstd (frame, stream): op_family, achip_host.h
// the helper context codec family `op` (1, 2) of a mixed batch runs on: made at first use, this context's options at every use
int32_t mix_lane(achip_ctx* ctx, int op, achip_ctx** out)
{
    if (!ctx->mixLane[op]) {
        ctx->mixLane[op].reset(achip_ctx_create(ctx->device));
        if (!ctx->mixLane[op]) return ACHIP_STATUS(ACHIP_CLASS_DEVICE, ACHIP_D_HIP_ERROR);
    }
    if (!ctx->mixLaneDone[op]) {  // (on its own: a context whose event could not be made at the first attempt tries again, it does not record on a null event)
        HIP_TRY(ctx->mixLaneDone[op].create());
    }
    static_cast<achip::Settings&>(*ctx->mixLane[op]) = *ctx;  // (the settings only: a lane's state -- auto mode's memory among it -- is its own)
    *out = ctx->mixLane[op].get();
    return 0;
}
}  // namespace

int32_t achip_mixed_batch(achip_ctx* ctx, const int32_t* codecOp, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                          const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks)
{
    if (!ctx) return bad_argument("ctx is null");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!codecOp || !srcOff || !srcLen || !dstOff || !dstCap || !outLen || !status) return bad_argument("null metadata array");
    const int64_t n = nBlocks;
    int64_t count[kNumOps + 1] = {0};
    for (int64_t i = 0; i < n; i++) {
        if (!op_known(codecOp[i])) return bad_argument("codecOp out of range");
        count[codecOp[i] + 1]++;
    }
    int32_t r = ensure_mix(ctx, n);
    if (r < 0) return r;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(ctx->mixUploaded.get()));  // the previous call's upload has left the pinned buffer (no-op on the first call)
    int64_t start[kNumOps + 1];
    start[0] = 0;
    for (int k = 0; k < kNumOps; k++) start[k + 1] = start[k] + count[k + 1];
    {
        int64_t fill[kNumOps];
        for (int k = 0; k < kNumOps; k++) fill[k] = start[k];
        for (int64_t i = 0; i < n; i++) ctx->mixHost.get()[fill[codecOp[i]]++] = (int32_t)i;  // stable: items of one codec keep their order
    }
    const int64_t cap = ctx->mixItems;
    uint8_t* d = ctx->mixDev.get();
    int64_t* gSrcOff = (int64_t*)d;
    int64_t* gDstOff = gSrcOff + cap;
    int64_t* gErr = gDstOff + cap;
    int32_t* gSrcLen = (int32_t*)(gErr + cap);
    int32_t* gDstCap = gSrcLen + cap;
    int32_t* gOutLen = gDstCap + cap;
    int32_t* gStatus = gOutLen + cap;
    int32_t* perm = gStatus + cap;
    HIP_TRY(hipMemcpyAsync(perm, ctx->mixHost.get(), (size_t)(n * 4), hipMemcpyHostToDevice, ctx->stream.get()));
    HIP_TRY(hipEventRecord(ctx->mixUploaded.get(), ctx->stream.get()));
    const achip::BatchArgs all = make_args(srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks);
    HIP_TRY(achip::launch_mix_gather(perm, nBlocks, all, gSrcOff, gSrcLen, gDstOff, gDstCap, ctx->stream.get()));
    // The buckets of one codec family in turn (its encoders first: theirs are the long chains -- a file as ONE block is a single wavefront's work for 0.4 s --, and they are
    // launched without a host round trip), the families side by side: LZ4's on this context's stream, Snappy's and Zstd's on a helper context each.
    bool familyUsed[kMixFamilies] = {};
    for (int k = 0; k < kNumOps; k++) familyUsed[op_family(k)] |= count[k + 1] != 0;
    const bool sideBySide = ctx->mixConcurrent != 0 && (int)familyUsed[0] + (int)familyUsed[1] + (int)familyUsed[2] > 1;
    achip_ctx* lanes[kMixFamilies] = {ctx, ctx, ctx};
    bool laneJoined[kMixFamilies] = {};  // helper lanes that were made to wait for the gather (and may have been given work): they must be joined back, also on failure
    // joins the helper lanes used so far back into the context's stream -- on every way out, so that achip_ctx_synchronize covers them and the next
    // call cannot reuse the mixed-batch scratch (gOutLen, gStatus, perm) under kernels of this one
    auto join_lanes = [&]() -> int32_t {
        int32_t jr = 0;
        for (int f = 1; f < kMixFamilies; f++) {
            if (!laneJoined[f]) continue;
            laneJoined[f] = false;
            hipError_t e = hipEventRecord(ctx->mixLaneDone[f].get(), lanes[f]->stream.get());
            if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream.get(), ctx->mixLaneDone[f].get(), 0);
            if (e != hipSuccess) {
                (void)hipStreamSynchronize(lanes[f]->stream.get());  // (the event path failed: wait here instead)
                jr = device_failure("joining the mixed batch's helper lanes", e);
            }
        }
        return jr;
    };
    r = 0;
    if (sideBySide) {
        if (!ctx->mixGathered) HIP_TRY(ctx->mixGathered.create());
        HIP_TRY(hipEventRecord(ctx->mixGathered.get(), ctx->stream.get()));
        for (int f = 1; f < kMixFamilies && r >= 0; f++) {
            if (!familyUsed[f]) continue;
            r = mix_lane(ctx, f, &lanes[f]);
            if (r < 0) break;
            const hipError_t e = hipStreamWaitEvent(lanes[f]->stream.get(), ctx->mixGathered.get(), 0);
            if (e != hipSuccess) {
                r = device_failure("hipStreamWaitEvent(lane, gathered)", e);
                break;
            }
            laneJoined[f] = true;
        }
    }
    for (int pass = 0; pass < 2 && r >= 0; pass++) {
        for (int k = 0; k < kNumOps && r >= 0; k++) {
            if (count[k + 1] == 0 || (pass == 0) != op_is_encoder(k)) continue;
            const int64_t s = start[k];
            r = launch_op(k, lanes[op_family(k)], make_args(srcBase, gSrcOff + s, gSrcLen + s, dstBase, gDstOff + s, gDstCap + s, gOutLen + s, gStatus + s, gErr + s, (int32_t)count[k + 1]));
        }
    }
    const int32_t joined = join_lanes();
    if (r < 0) return r;
    if (joined < 0) return joined;
    HIP_TRY(achip::launch_mix_scatter(perm, nBlocks, gOutLen, gStatus, gErr, all, ctx->stream.get()));
    return 0;
}

// ---- decoded sizes and the output planner (decoded_size.hip) ----
// (the value arguments are checked before the context is looked at: a caller's mistake is reported the same with and without a device)
int32_t achip_decoded_size_batch(achip_ctx* ctx, int32_t codecOp, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t* outSize, int32_t* status,
                                 int64_t* errOffset, int32_t nBlocks)
{
    if (!op_known(codecOp) || op_is_encoder(codecOp)) return bad_argument("codecOp is not a decode op");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!ctx) return bad_argument("ctx is null");
    if (!srcOff || !srcLen || !outSize || !status || !errOffset) return bad_argument("null array");
    HIP_TRY(hipSetDevice(ctx->device));
    // (the block codecs' size kernels use no scratch -- 0 bytes --: such a call does not take it, and the last decode's statistics stay readable)
    if (const int64_t bytes = achip::decoded_size_scratch_bytes(codecOp, nBlocks); bytes > 0) {
        if (const int32_t r = take_scratch(ctx, bytes); r < 0) return r;
    }
    achip::SizeArgs s{(const uint8_t*)srcBase, srcOff, srcLen, outSize, status, errOffset, nBlocks};
    s.lz4fLinked = ctx->kernel.lz4fLinkedBlocks;
    HIP_TRY(achip::launch_decoded_size(codecOp, s, ctx->stream.get(), ctx->scratch.get()));
    return 0;
}

int32_t achip_plan_outputs(achip_ctx* ctx, const int64_t* outSize, const int32_t* status, int32_t nBlocks, int32_t align, int64_t* dstOff, int32_t* dstCap, int64_t* total)
{
    if (align < 1 || align > 4096 || (align & (align - 1)) != 0) return bad_argument("align must be a power of two in 1..4096");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!ctx) return bad_argument("ctx is null");
    if (!outSize || !status || !dstOff || !dstCap || !total) return bad_argument("null array");
    HIP_TRY(hipSetDevice(ctx->device));
    if (const int32_t r = take_scratch(ctx, achip::plan_outputs_scratch_bytes(nBlocks)); r < 0) return r;
    HIP_TRY(achip::launch_plan_outputs(outSize, status, nBlocks, align, dstOff, dstCap, total, ctx->scratch.get(), ctx->stream.get()));
    return 0;
}

// ---- compress bounds and the dense copy of a compressed batch (pack_outputs.hip) ----
int32_t achip_compress_bound_batch(achip_ctx* ctx, int32_t codecOp, const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t nBlocks)
{
    if (!op_known(codecOp) || !op_is_encoder(codecOp)) return bad_argument("codecOp is not a compress op");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!ctx) return bad_argument("ctx is null");
    if (!srcLen || !outSize || !status) return bad_argument("null array");
    HIP_TRY(hipSetDevice(ctx->device));
    if (codecOp == ACHIP_OP_LZ4FRAME_COMPRESS && achip::lz4f_list_writer(ctx->kernel)) {  // the bound of the writer that will run
        HIP_TRY(achip::launch_lz4frame_list_bound(srcLen, outSize, status, nBlocks, ctx->stream.get(), ctx->kernel));
        return 0;
    }
    HIP_TRY(achip::launch_compress_bound(codecOp, srcLen, outSize, status, nBlocks, ctx->hadoopBufferSize, ctx->stream.get(), ctx->kernel.snfBlockSize));
    return 0;
}

int32_t achip_pack_outputs(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* outLen, const int32_t* status, const void* rawBase, const int64_t* rawOff,
                           const int32_t* rawLen, int32_t nBlocks, int32_t align, void* packedBase, int64_t packedCap, int64_t* packedOff, int32_t* packedLen, int32_t* stored,
                           int64_t* total)
{
    if (align < 1 || align > 4096 || (align & (align - 1)) != 0) return bad_argument("align must be a power of two in 1..4096");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    const int rawGiven = (rawBase != nullptr ? 1 : 0) + (rawOff != nullptr ? 1 : 0) + (rawLen != nullptr ? 1 : 0);
    if (rawGiven != 0 && rawGiven != 3) return bad_argument("rawBase, rawOff and rawLen must all be given or all be null");
    if ((stored != nullptr) != (rawGiven == 3)) return bad_argument("stored must be given exactly when the raw arrays are");
    if (packedBase != nullptr && packedCap < 0) return bad_argument("packedCap < 0");
    if (nBlocks == 0) return 0;
    if (!ctx) return bad_argument("ctx is null");
    if (!srcOff || !outLen || !status || !packedOff || !packedLen || !total) return bad_argument("null array");
    HIP_TRY(hipSetDevice(ctx->device));
    if (const int32_t r = take_scratch(ctx, achip::pack_outputs_scratch_bytes(nBlocks)); r < 0) return r;
    const achip::PackArgs p{(const uint8_t*)srcBase, srcOff, outLen, status, (const uint8_t*)rawBase, rawOff, rawLen, nBlocks, align, (uint8_t*)packedBase, packedCap,
                            packedOff, packedLen, stored, total};
    HIP_TRY(achip::launch_pack_outputs(p, ctx->scratch.get(), ctx->stream.get()));
    return 0;
}

}  // extern "C"
