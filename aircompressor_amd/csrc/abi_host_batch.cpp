// abi_host_batch.cpp -- the host-pointer API: chunked, multi-buffered staging (H2D || kernels || D2H || host copies); the single-block calls and the
// call over several contexts on top of it.  How a batch is cut and laid out in a slot is achip_host_plan.h's.
// What a Compressor.compress(byte[]...) / decompress(MemorySegment...) caller gets.  The items are cut into chunks of about
// host.chunk_bytes of staging; chunk c uses slot c & 1.  Per chunk: the host gathers the inputs into the slot's pinned buffer (a few
// copy threads), `copyIn` uploads, the context stream runs the codec kernels, `copyOut` downloads, and the host scatters the outputs
// to the caller's buffers -- while the next chunk is already being gathered / uploaded / run.  Kernels stay on ONE stream (they share
// the context's scratch); events order the slots.  A mixed batch is first ordered by codec op so that every chunk is homogeneous.
#include "achip_host.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

using namespace achip::host;
using achip::plan::HostChunk;

struct achip::host::CopyPool {
    std::vector<std::thread> threads;
    std::mutex m;
    std::condition_variable cvWork, cvDone;
    std::function<void(int64_t)> fn;
    int64_t nTasks = 0;
    std::atomic<int64_t> next{0};
    int64_t generation = 0;
    int active = 0;
    bool stop = false;

    explicit CopyPool(int n)
    {
        for (int t = 0; t < n; t++) {
            threads.emplace_back([this] { worker(); });
        }
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(m);
            stop = true;
        }
        cvWork.notify_all();
        for (auto& t : threads) t.join();
    }
    void worker()
    {
        int64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(m);
                cvWork.wait(g, [&] { return stop || generation != seen; });
                if (stop) return;
                seen = generation;
            }
            drain();
            {
                std::lock_guard<std::mutex> g(m);
                if (--active == 0) cvDone.notify_all();
            }
        }
    }
    void drain()
    {
        for (;;) {
            const int64_t i = next.fetch_add(1);
            if (i >= nTasks) return;
            fn(i);
        }
    }
    // runs f(0..n-1) on the pool's threads and the calling thread; returns when all are done
    void run(int64_t n, std::function<void(int64_t)> f)
    {
        if (n <= 0) return;
        if (threads.empty() || n == 1) {
            for (int64_t i = 0; i < n; i++) f(i);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m);
            fn = std::move(f);
            nTasks = n;
            next.store(0);
            active = (int)threads.size();
            generation++;
        }
        cvWork.notify_all();
        drain();
        std::unique_lock<std::mutex> g(m);
        cvDone.wait(g, [&] { return active == 0; });
    }
};
void achip::host::CopyPoolDelete::operator()(CopyPool* p) const { delete p; }

namespace {

// `slots` staging slots of at least `slotBytes` each (pinned host + device); the copy streams, events and copy threads on first use
int32_t ensure_host_path(achip_ctx* ctx, int64_t slotBytes, int slots)
{
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->copyIn) {
        // The download of a chunk is a copy KERNEL of the runtime's (`__amd_rocclr_copyBuffer`: the timeline in profiles/r06_host_timeline.txt), launched wide;
        // at the decode stream's priority the next chunk's decode kernels only got the CUs when it had drained -- a chunk's kernels took 1.7 ms beside it
        // against 0.5 alone, and the pipeline ran at the sum of its stages.  The copy streams therefore have the LOWEST priority (host.copy_priority = 0: the default one).
        int least = 0, greatest = 0;
        if (ctx->hostCopyLowPriority != 0 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest) {
            HIP_TRY(ctx->copyIn.create(least));
            HIP_TRY(ctx->copyOut.create(least));
        }
        else {
            (void)hipGetLastError();
            HIP_TRY(ctx->copyIn.create());
            HIP_TRY(ctx->copyOut.create());
        }
        for (int s = 0; s < achip_ctx::kHostSlots; s++) {
            HIP_TRY(ctx->evH2D[s].create());
            HIP_TRY(ctx->evK[s].create());
            HIP_TRY(ctx->evD2H[s].create());
        }
    }
    if (!ctx->pool) {
        // gather and scatter have a pool each (they run side by side): host.copy_threads threads each, by default a sixteenth of the host's
        // hardware threads, 2 .. 16 (the calling thread / the finalizer thread is one of each pool's copiers).  (Round 6: 16 where it was 8 -- on boxes whose
        // host copies are slow, two NUMA nodes and the process on the far one, the scatter IS the call: 8 threads 31-34 GiB/s, 16 threads 33-40; on the
        // others 8 and 16 are alike: profiles/r06_notes.md)
        int t = ctx->hostCopyThreads;
        if (t == 0) t = (int)std::min<unsigned>(16u, std::max(2u, std::thread::hardware_concurrency() / 16));
        ctx->pool.reset(new CopyPool(t - 1));
        ctx->poolOut.reset(new CopyPool(t - 1));
    }
    int64_t bytes = ctx->slotBytes;
    if (slotBytes > ctx->slotBytes) {
        HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
        HIP_TRY(hipStreamSynchronize(ctx->copyIn.get()));
        HIP_TRY(hipStreamSynchronize(ctx->copyOut.get()));
        ctx->slotBytes = 0;
        ctx->slotCount = 0;
        for (int s = 0; s < achip_ctx::kHostSlots; s++) {
            HIP_TRY(ctx->slotHost[s].reset());
            HIP_TRY(ctx->slotDev[s].reset());
        }
        bytes = std::max<int64_t>(slotBytes, 1 << 20);
    }
    // A slot whose allocation fails fails the call; the size counts only once a slot of it is held, so a context that could not have one oversized slot is
    // back at none and serves the next, smaller batch.  (A pinned half without its device half stays with the context for the next attempt or its end.)
    while (ctx->slotCount < slots) {
        const int s = ctx->slotCount;
        HIP_TRY(ctx->slotHost[s].alloc((size_t)bytes));
        HIP_TRY(ctx->slotDev[s].alloc((size_t)bytes));
        ctx->slotBytes = bytes;
        ctx->slotCount = s + 1;
    }
    return 0;
}

// order[j] = caller's item index of the j-th processed item (nullptr: identity); ops: per item (mixed) or nullptr (all `op`)
int32_t host_batch(achip_ctx* ctx, int32_t op, const int32_t* ops, const int32_t* order, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen,
                   void* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int64_t n)
{
    auto item = [&](int64_t j) -> int64_t { return order ? order[j] : j; };
    achip::plan::ChunkPlan plan = achip::plan::cut_chunks(n, order, ops, op, srcLen, dstCap, ctx->hostChunkBytes, ctx->hostRamp != 0);
    if (plan.negativeLength) return bad_argument("negative length");
    const std::vector<HostChunk>& chunks = plan.chunks;
    const std::vector<int64_t>& sOff = plan.sOff;  // per processed item: offsets inside its chunk's input / output regions
    const std::vector<int64_t>& dOff = plan.dOff;
    const int nSlots = (int)std::min<size_t>(chunks.size(), (size_t)ctx->hostSlots);
    int32_t r = ensure_host_path(ctx, plan.maxSlot, nSlots);
    if (r < 0) return r;

    // copy tasks over a chunk's items: consecutive items are grouped up to kCopyGrain bytes, one task per group
    auto for_items = [&](CopyPool& pool, const HostChunk& c, bool outputs, const std::function<void(int64_t)>& body) {
        if (c.count == 1) {
            body(c.first);
            return;
        }
        const std::vector<int64_t> cut = achip::plan::copy_cuts(c.first, c.count, [&](int64_t j) -> int64_t {
            const int64_t i = item(j);
            return outputs ? std::max(outLen[i], 0) : srcLen[i];
        });
        pool.run((int64_t)cut.size() - 1, [&](int64_t t) {
            for (int64_t j = cut[t]; j < cut[t + 1]; j++) body(j);
        });
    };

    auto gather = [&](const HostChunk& c, uint8_t* h) {
        for_items(*ctx->pool, c, false, [&](int64_t j) {
            const int64_t i = item(j);
            if (srcLen[i] > 0) memcpy(h + sOff[j], (const uint8_t*)srcBase + srcOff[i], (size_t)srcLen[i]);
        });
        for (int64_t j = c.first; j < c.first + c.count; j++) {
            const int64_t i = item(j), k = j - c.first;
            ((int64_t*)(h + c.oSrcOff))[k] = sOff[j];
            ((int64_t*)(h + c.oDstOff))[k] = c.oDst + dOff[j];
            ((int32_t*)(h + c.oSrcLen))[k] = srcLen[i];
            ((int32_t*)(h + c.oDstCap))[k] = dstCap[i];
        }
    };
    auto scatter = [&](const HostChunk& c, const uint8_t* h) {
        for (int64_t j = c.first; j < c.first + c.count; j++) {
            const int64_t i = item(j), k = j - c.first;
            outLen[i] = ((const int32_t*)(h + c.oOutLen))[k];
            status[i] = ((const int32_t*)(h + c.oStatus))[k];
            if (errOffset) errOffset[i] = ((const int64_t*)(h + c.oErr))[k];
        }
        for_items(*ctx->poolOut, c, true, [&](int64_t j) {
            const int64_t i = item(j);
            if (status[i] == 0 && outLen[i] > 0) memcpy((uint8_t*)dstBase + dstOff[i], h + c.oDst + dOff[j], (size_t)outLen[i]);
        });
    };
    auto batch_args = [&](const HostChunk& c, uint8_t* d) {
        return make_args(d, (const int64_t*)(d + c.oSrcOff), (const int32_t*)(d + c.oSrcLen), d, (const int64_t*)(d + c.oDstOff), (const int32_t*)(d + c.oDstCap),
                         (int32_t*)(d + c.oOutLen), (int32_t*)(d + c.oStatus), (int64_t*)(d + c.oErr), (int32_t)c.count);
    };
    const int savedHint = ctx->maxSrcLenHint;
    // A chunk of few blocks (at most decompress.latency_max_blocks: a single block, a small batch) in host memory: a look at its first block's first tokens tells
    // the decoders apart -- short sequences: the two passes; long ones: the ring decoders' latency class.  Only the choice of the decoder depends on it, never a
    // result: whatever these bytes are, every decoder reports what the Java decoder would.  (Larger chunks -- a pipeline chunk is ~1 000 blocks -- take the two
    // passes unseen.  Looking at them too was tried: a chunk's kernels take 0.76 ms with the rings at 64 lanes against 0.92 with the two passes, but the pipeline
    // is bound by the host's copies and the link, and its rate varies 28-40 GiB/s from run to run on one box with either: nothing to gain, one more rule to explain.)
    auto look_at_tokens = [&](const HostChunk& c, const uint8_t* h) {
        const bool few = (c.op == ACHIP_OP_LZ4_DECOMPRESS || c.op == ACHIP_OP_SNAPPY_DECOMPRESS) && c.count <= std::max(ctx->latencyMaxBlocks, ctx->hostLookMaxBlocks);
        if (few) {
            ctx->smallBatchHint = achip::plan::probe_sequences(c.op == ACHIP_OP_SNAPPY_DECOMPRESS, h + sOff[c.first], srcLen[item(c.first)]);
        }
    };

    if (chunks.size() == 1) {
        // one chunk (a single block -- what Compressor.compress(MemorySegment, MemorySegment) hands over -- or a small batch): nothing to overlap,
        // everything in order on the context stream: upload, kernels, download, one wait
        const HostChunk& c = chunks[0];
        uint8_t* h = ctx->slotHost[0].get();
        uint8_t* d = ctx->slotDev[0].get();
        gather(c, h);
        look_at_tokens(c, h);
        HIP_TRY(hipMemcpyAsync(d, h, (size_t)c.inEnd, hipMemcpyHostToDevice, ctx->stream.get()));
        ctx->maxSrcLenHint = std::max(c.maxLen, 1);
        r = launch_op(c.op, ctx, batch_args(c, d));
        ctx->maxSrcLenHint = savedHint;
        if (r < 0) {
            (void)hipStreamSynchronize(ctx->stream.get());
            return r;
        }
        HIP_TRY(hipMemcpyAsync(h + c.oErr, d + c.oErr, (size_t)(c.end - c.oErr), hipMemcpyDeviceToHost, ctx->stream.get()));
        HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
        scatter(c, h);
        return 0;
    }

    // ---- several chunks: chunk c uses slot c % nSlots.  This thread gathers chunk after chunk into pinned memory and enqueues upload (copyIn),
    // kernels (the context stream: they share the context's scratch) and download (copyOut), events ordering the three; a finalizer thread waits
    // for each download and scatters the outputs to the caller's buffers with a copy pool of its own -- so that gather, upload, kernels, download
    // and scatter of up to nSlots chunks are in flight side by side. ----
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clk::now() - t0).count(); };
    const clk::time_point tStart = clk::now();
    int64_t gatherUs = 0, scatterUs = 0, waitSlotUs = 0, waitDownloadUs = 0;
    std::mutex m;
    std::condition_variable cv;
    int64_t enqueued = 0, finalized = 0;  // chunk counts
    bool aborted = false;
    int32_t finalizerStatus = 0;
    std::string finalizerMessage;
    std::thread finalizer([&] {
        if (hipSetDevice(ctx->device) != hipSuccess) {
            std::lock_guard<std::mutex> g(m);
            finalizerStatus = ACHIP_STATUS(ACHIP_CLASS_DEVICE, ACHIP_D_HIP_ERROR);
            finalizerMessage = "hipSetDevice failed in the finalizer thread";
            finalized = (int64_t)chunks.size();
            cv.notify_all();
            return;
        }
        for (int64_t ci = 0; ci < (int64_t)chunks.size(); ci++) {
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return enqueued > ci || aborted; });
                if (enqueued <= ci) return;
            }
            const int slot = (int)(ci % nSlots);
            clk::time_point t0 = clk::now();
            const hipError_t e = hipEventSynchronize(ctx->evD2H[slot].get());
            waitDownloadUs += us_since(t0);
            if (e != hipSuccess) {
                std::lock_guard<std::mutex> g(m);
                finalizerStatus = ACHIP_STATUS(ACHIP_CLASS_DEVICE, ACHIP_D_HIP_ERROR);
                finalizerMessage = std::string("hipEventSynchronize: ") + hipGetErrorString(e);
            }
            else {
                t0 = clk::now();
                scatter(chunks[(size_t)ci], ctx->slotHost[slot].get());
                scatterUs += us_since(t0);
            }
            {
                std::lock_guard<std::mutex> g(m);
                finalized = ci + 1;
            }
            cv.notify_all();
        }
    });
    auto enqueue = [&](const HostChunk& c, int slot) -> int32_t {
        uint8_t* h = ctx->slotHost[slot].get();
        uint8_t* d = ctx->slotDev[slot].get();
        if ((ctx->hostBlit & 1) != 0) HIP_TRY(achip::launch_blit(d, h, c.inEnd, ctx->hostBlitGroups, ctx->copyIn.get()));
        else HIP_TRY(hipMemcpyAsync(d, h, (size_t)c.inEnd, hipMemcpyHostToDevice, ctx->copyIn.get()));
        HIP_TRY(hipEventRecord(ctx->evH2D[slot].get(), ctx->copyIn.get()));
        HIP_TRY(hipStreamWaitEvent(ctx->stream.get(), ctx->evH2D[slot].get(), 0));
        ctx->maxSrcLenHint = std::max(c.maxLen, 1);
        look_at_tokens(c, h);
        const int32_t rr = launch_op(c.op, ctx, batch_args(c, d));
        ctx->maxSrcLenHint = savedHint;
        if (rr < 0) return rr;
        HIP_TRY(hipEventRecord(ctx->evK[slot].get(), ctx->stream.get()));
        HIP_TRY(hipStreamWaitEvent(ctx->copyOut.get(), ctx->evK[slot].get(), 0));
        if ((ctx->hostBlit & 2) != 0) HIP_TRY(achip::launch_blit(h + c.oErr, d + c.oErr, c.end - c.oErr, ctx->hostBlitGroups, ctx->copyOut.get()));
        else HIP_TRY(hipMemcpyAsync(h + c.oErr, d + c.oErr, (size_t)(c.end - c.oErr), hipMemcpyDeviceToHost, ctx->copyOut.get()));
        HIP_TRY(hipEventRecord(ctx->evD2H[slot].get(), ctx->copyOut.get()));
        return 0;
    };
    std::string message;
    for (int64_t ci = 0; ci < (int64_t)chunks.size() && r >= 0; ci++) {
        const int slot = (int)(ci % nSlots);
        clk::time_point t0 = clk::now();
        {
            std::unique_lock<std::mutex> g(m);
            cv.wait(g, [&] { return finalized >= ci - nSlots + 1; });  // the slot's previous chunk has left it
            if (finalizerStatus < 0) break;
        }
        waitSlotUs += us_since(t0);
        t0 = clk::now();
        gather(chunks[(size_t)ci], ctx->slotHost[slot].get());
        gatherUs += us_since(t0);
        r = enqueue(chunks[(size_t)ci], slot);
        if (r < 0) message = g_lastError;
        {
            std::lock_guard<std::mutex> g(m);
            if (r < 0) aborted = true;
            else enqueued = ci + 1;
        }
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> g(m);
        aborted = true;  // (nothing more will be enqueued: the finalizer leaves after the last enqueued chunk)
    }
    cv.notify_all();
    finalizer.join();
    ctx->hostGatherUs = gatherUs;
    ctx->hostScatterUs = scatterUs;
    ctx->hostWaitSlotUs = waitSlotUs;
    ctx->hostWaitDownloadUs = waitDownloadUs;
    ctx->hostChunks = (int64_t)chunks.size();
    ctx->hostTotalUs = us_since(tStart);
    if (r < 0 || finalizerStatus < 0) {
        (void)hipStreamSynchronize(ctx->copyIn.get());
        (void)hipStreamSynchronize(ctx->stream.get());
        (void)hipStreamSynchronize(ctx->copyOut.get());
        if (r < 0) {
            g_lastError = message;
            return r;
        }
        g_lastError = finalizerMessage;
        return finalizerStatus;
    }
    // the context stream is idle again for the caller (everything it launched was awaited through evK -> evD2H)
    return 0;
}

}  // namespace

extern "C" {

int32_t achip_batch_host(int32_t codecOp, ACHIP_BATCH_ARGS)
{
    if (!ctx) return bad_argument("ctx is null");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!op_known(codecOp)) return bad_argument("unknown codecOp");
    if (!srcOff || !srcLen || !dstOff || !dstCap || !outLen || !status) return bad_argument("null metadata array");
    return host_batch(ctx, codecOp, nullptr, nullptr, srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks);
}

int32_t achip_mixed_batch_host(achip_ctx* ctx, const int32_t* codecOp, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                               const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks)
{
    if (!ctx) return bad_argument("ctx is null");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!codecOp || !srcOff || !srcLen || !dstOff || !dstCap || !outLen || !status) return bad_argument("null metadata array");
    // bucket by codec op (stable): every chunk of the pipeline is then homogeneous
    std::vector<int32_t> order((size_t)nBlocks);
    int64_t start[kNumOps + 1] = {0};
    for (int32_t i = 0; i < nBlocks; i++) {
        if (!op_known(codecOp[i])) return bad_argument("codecOp out of range");
        start[codecOp[i] + 1]++;
    }
    for (int k = 0; k < kNumOps; k++) start[k + 1] += start[k];
    for (int32_t i = 0; i < nBlocks; i++) order[(size_t)start[codecOp[i]]++] = i;
    return host_batch(ctx, 0, codecOp, order.data(), srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks);
}

// ---- single block, host pointers -----------------------------------------
static int32_t single_block(int32_t op, achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset)
{
    if (!ctx) return bad_argument("ctx is null");
    if (srcLen < 0 || dstCap < 0) return bad_argument("negative length");
    int64_t so = 0, dofs = 0, eo = 0;
    int32_t outLen = 0, status = 0;
    int32_t r = achip_batch_host(op, ctx, src, &so, &srcLen, dst, &dofs, &dstCap, &outLen, &status, &eo, 1);
    if (r < 0) return r;
    if (errOffset) *errOffset = eo;
    return status < 0 ? status : outLen;
}

#define ACHIP_DEFINE_SINGLE(fn, op)                                                                                   \
    int32_t fn(achip_ctx* ctx, const void* src, void* dst, int32_t srcLen, int32_t dstCap, int64_t* errOffset)        \
    {                                                                                                                 \
        return single_block(op, ctx, src, dst, srcLen, dstCap, errOffset);                                            \
    }
ACHIP_DEFINE_SINGLE(achip_lz4_decompress, ACHIP_OP_LZ4_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_lz4_compress, ACHIP_OP_LZ4_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_snappy_decompress, ACHIP_OP_SNAPPY_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_snappy_compress, ACHIP_OP_SNAPPY_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_zstd_decompress, ACHIP_OP_ZSTD_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_zstd_compress, ACHIP_OP_ZSTD_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_lz4frame_decompress, ACHIP_OP_LZ4FRAME_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_lz4frame_compress, ACHIP_OP_LZ4FRAME_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_snappyframed_decompress, ACHIP_OP_SNAPPYFRAMED_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_snappyframed_compress, ACHIP_OP_SNAPPYFRAMED_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_lz4hadoop_decompress, ACHIP_OP_LZ4HADOOP_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_lz4hadoop_compress, ACHIP_OP_LZ4HADOOP_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_snappyhadoop_decompress, ACHIP_OP_SNAPPYHADOOP_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_snappyhadoop_compress, ACHIP_OP_SNAPPYHADOOP_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_zstdstream_compress, ACHIP_OP_ZSTDSTREAM_COMPRESS)
ACHIP_DEFINE_SINGLE(achip_lzo_decompress, ACHIP_OP_LZO_DECOMPRESS)
ACHIP_DEFINE_SINGLE(achip_lzo_compress, ACHIP_OP_LZO_COMPRESS)

// ---- one process, several contexts (normally one per device), one host thread each -------------------------------------------
// The native twin of java/.../HipBatchCodec.run: the batch is cut into nCtx contiguous slices balanced by srcLen + dstCap (the rule of
// achip_partition_blocks), slice d goes through achip_batch_host / achip_mixed_batch_host on ctxs[d] in a thread of its own.  Units are
// independent (M/zstd/ZstdFrameDecompressor.java:151, M/zstd/ZstdFrameCompressor.java:162): no exchange between the slices.
int32_t achip_multi_batch_host(achip_ctx* const* ctxs, int32_t nCtx, int32_t codecOp, const int32_t* codecOps, const void* srcBase, const int64_t* srcOff,
                               const int32_t* srcLen, void* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status,
                               int64_t* errOffset, int32_t nBlocks, int32_t* sliceStarts)
{
    if (!ctxs || nCtx <= 0) return bad_argument("no contexts");
    if (nCtx > 64) return bad_argument("more than 64 contexts");
    for (int32_t d = 0; d < nCtx; d++) {
        if (!ctxs[d]) return bad_argument("ctx is null");
        for (int32_t e = 0; e < d; e++) {
            if (ctxs[e] == ctxs[d]) return bad_argument("a context listed twice (a context serves one thread at a time)");
        }
    }
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (!codecOps && !op_known(codecOp)) return bad_argument("unknown codecOp");
    std::vector<int32_t> starts((size_t)nCtx + 1, 0);
    if (nBlocks > 0) {
        if (!srcOff || !srcLen || !dstOff || !dstCap || !outLen || !status) return bad_argument("null metadata array");
        std::vector<int64_t> weight((size_t)nBlocks);
        for (int32_t i = 0; i < nBlocks; i++) weight[(size_t)i] = (int64_t)std::max(srcLen[i], 0) + std::max(dstCap[i], 0);
        const int32_t r = achip_partition_blocks(weight.data(), nBlocks, nCtx, starts.data());
        if (r < 0) return r;
    }
    if (sliceStarts) {
        for (int32_t d = 0; d <= nCtx; d++) sliceStarts[d] = starts[(size_t)d];
    }
    std::vector<int32_t> rc((size_t)nCtx, 0);
    std::vector<std::string> messages((size_t)nCtx);
    auto slice = [&](int32_t d) {
        const int32_t first = starts[(size_t)d], count = starts[(size_t)d + 1] - first;
        if (count == 0) return;
        int64_t* eo = errOffset ? errOffset + first : nullptr;
        rc[(size_t)d] = codecOps ? achip_mixed_batch_host(ctxs[d], codecOps + first, srcBase, srcOff + first, srcLen + first, dstBase, dstOff + first, dstCap + first,
                                                          outLen + first, status + first, eo, count)
                                 : achip_batch_host(codecOp, ctxs[d], srcBase, srcOff + first, srcLen + first, dstBase, dstOff + first, dstCap + first, outLen + first,
                                                    status + first, eo, count);
        if (rc[(size_t)d] < 0) messages[(size_t)d] = g_lastError;  // (thread-local: carried to the caller's thread below)
    };
    std::vector<std::thread> workers;
    for (int32_t d = 1; d < nCtx; d++) workers.emplace_back(slice, d);
    slice(0);
    for (auto& w : workers) w.join();
    for (int32_t d = 0; d < nCtx; d++) {
        if (rc[(size_t)d] < 0) {
            g_lastError = "context " + std::to_string(d) + ": " + messages[(size_t)d];
            return rc[(size_t)d];
        }
    }
    return 0;
}

// ---- multi-GPU partition (host arithmetic) --------------------------------
int32_t achip_partition_blocks(const int64_t* weight, int32_t nBlocks, int32_t nParts, int32_t* starts)
{
    if (nBlocks < 0 || nParts <= 0 || !starts) return bad_argument("bad partition arguments");
    achip::plan::partition_blocks(weight, nBlocks, nParts, starts);
    return 0;
}

}  // extern "C"
