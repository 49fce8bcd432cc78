// achip_host.h -- what the host units of libaircompressor_hip.so share (private to csrc/, not installed): the context, the owners of device resources, the
// error helpers, and the few functions one unit calls in another.  The units: abi_context.cpp (context, statuses, sizes), abi_dispatch.cpp (scratch policy, the
// device-resident batch entry points), abi_hash.cpp, abi_host_batch.cpp (the host-pointer pipeline), abi_window.cpp (windows over the chunked containers), abi_zstd_stream.cpp (the incremental Zstd reader and writer).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "achip_host_plan.h"
#include "achip_launch.h"
#include "achip_stats.h"

#define ACHIP_HIDDEN __attribute__((visibility("hidden")))  // what crosses the host units and is no part of the C ABI stays out of the dynamic symbol table

namespace achip {
namespace host ACHIP_HIDDEN {

// ---- owners: move-only, freed by the destructor; reset() frees now and says how that went.  Making one frees what was held first; a failed attempt leaves
// the holder empty (clearing the runtime's last error is the caller's business). ----
template <class H, hipError_t (*Release)(H)>
class Holder {
public:
    Holder() = default;
    Holder(Holder&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Holder& operator=(Holder&& o) noexcept
    {
        if (this != &o) {
            (void)reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~Holder() { (void)reset(); }
    explicit operator bool() const { return h_ != nullptr; }
    hipError_t reset()
    {
        const hipError_t e = h_ ? Release(h_) : hipSuccess;
        h_ = nullptr;
        return e;
    }

protected:
    template <class Make>
    hipError_t make(Make m)
    {
        (void)reset();
        const hipError_t e = m(&h_);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    H h_ = nullptr;
};
template <class T = void>
struct DeviceBuffer : Holder<void*, hipFree> {
    T* get() const { return (T*)h_; }
    hipError_t alloc(size_t bytes) { return make([&](void** p) { return hipMalloc(p, bytes); }); }
};
template <class T = void>
struct PinnedBuffer : Holder<void*, hipHostFree> {
    T* get() const { return (T*)h_; }
    hipError_t alloc(size_t bytes) { return make([&](void** p) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }); }
};
struct Event : Holder<hipEvent_t, hipEventDestroy> {
    hipEvent_t get() const { return h_; }
    hipError_t create() { return make([](hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }); }
};
struct Stream : Holder<hipStream_t, hipStreamDestroy> {
    hipStream_t get() const { return h_; }
    hipError_t create() { return make([](hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }); }
    hipError_t create(int priority) { return make([&](hipStream_t* s) { return hipStreamCreateWithPriority(s, hipStreamNonBlocking, priority); }); }
};

struct CopyPool;  // abi_host_batch.cpp
struct CopyPoolDelete {
    void operator()(CopyPool* p) const;
};

}  // namespace host
}  // namespace achip

// A context: its settings (achip_settings.h: what achip_ctx_set_option writes) and the state it owns.
struct achip_ctx : achip::Settings {
    ACHIP_HIDDEN ~achip_ctx();  // sets the device and waits for the stream; the members then free what they hold, the stream last
    int device = 0;
    achip::host::Stream stream;  // (declared in front of everything that is freed: destroyed last)
    int smallBatchHint = 0;      // set by the host-pointer path for ONE launch: what a look at the first block's tokens says -- 1 short sequences, 2 long ones (0: nobody looked)
    achip::stats::LastLaunch last;  // what the last launch that took the scratch left at its head (achip_ctx_get_stat; cleared by take_scratch alone)
    // Auto mode remembers (round 6): a call's probe statistics come back to pinned memory behind its kernels, without a wait; while the batches that follow have its
    // shape (codec, block count, the same source and destination buffers) the decoder the LAST ARRIVED statistics chose is the only one launched -- the other
    // decoder's kernels, launched to return at once, were ~65 us of a 8.2 ms headline call.  The probes still run in every call and go home, so a context whose
    // data changes character under one shape runs the wrong (slower, never incorrect: either decoder decodes any batch to the reference's bytes) decoder for as
    // many calls as it takes the first new statistics to arrive: one, for a caller that waits for its results.  (A first version probed one call in sixteen
    // and ran the rest blind: bench.py's own extras -- fragments, then text, same shape, same buffers -- decoded text on the rings for a whole measurement, 148
    // against 377 GiB/s.)  decompress.auto_remember = 0: both decoders are launched in every call, as until round 5.
    achip::host::PinnedBuffer<int32_t> autoPinned;  // 8 words: the probe statistics of the call in flight
    achip::host::Event autoEv;
    bool autoInFlight = false;
    int autoPendingFam = 0;
    int32_t autoPendingBlocks = 0;
    const void* autoPendingSrc = nullptr;
    const void* autoPendingDst = nullptr;
    int autoChoice[2] = {-1, -1};      // per codec family (0 LZ4, 1 Snappy): -1 unknown, else LZ4_PICK_RINGS or LZ4_PICK_TWOPASS
    int32_t autoBlocks[2] = {0, 0};
    const void* autoSrc[2] = {nullptr, nullptr};
    const void* autoDst[2] = {nullptr, nullptr};
    // The one device buffer every launch works in that needs working memory: the Zstd pipeline's stages, the two-pass decoders' records, the encoders' tables,
    // the containers' lists, the sizing / planning / packing calls' scans.  Grown on demand and never shrunk; a launch owns it until the next one on this
    // context takes it (take_scratch), which is also when the statistics at its head (`last`) end.
    achip::host::DeviceBuffer<> scratch;
    int64_t scratchBytes = 0;
    achip::host::DeviceBuffer<> zstdMbScratch;
    int64_t zstdMbScratchBytes = 0;
    // mixed batches, codec families side by side: a helper context for Snappy's and for Zstd's buckets (made when a batch first needs it: a stream and scratch of
    // its own, this context's options; LZ4's run on this context), and the events that order them behind the gather and in front of the scatter.  (Three streams, not
    // one per bucket: ROCm maps a process's streams onto GPU_MAX_HW_QUEUES = 4 hardware queues, and two long chains on one queue run one after the other --
    // profiles/r05_notes.md: six helper streams 1.22 s, with 8 queues 0.75.)
    std::unique_ptr<achip_ctx> mixLane[3];
    achip::host::Event mixGathered, mixLaneDone[3];
    // mixed batches (achip_mixed_batch): item permutation (pinned host + device) and the bucketed descriptor / result arrays
    achip::host::PinnedBuffer<int32_t> mixHost;
    achip::host::DeviceBuffer<uint8_t> mixDev;
    int64_t mixItems = 0;
    achip::host::Event mixUploaded;  // the last permutation upload: the pinned buffer may be rewritten once it has completed
    // host-pointer batches (achip_batch_host / achip_mixed_batch_host): up to four staging slots, chunks pipelined over three streams, gather and
    // scatter on copy pools of their own
    static constexpr int kHostSlots = 8;  // (the most host.slots accepts)
    std::unique_ptr<achip::host::CopyPool, achip::host::CopyPoolDelete> pool;     // gather: the caller's inputs -> pinned slot
    std::unique_ptr<achip::host::CopyPool, achip::host::CopyPoolDelete> poolOut;  // scatter: pinned slot -> the caller's outputs
    achip::host::PinnedBuffer<uint8_t> slotHost[kHostSlots];
    achip::host::DeviceBuffer<uint8_t> slotDev[kHostSlots];
    int64_t slotBytes = 0;
    int slotCount = 0;
    achip::host::Stream copyIn, copyOut;
    achip::host::Event evH2D[kHostSlots], evK[kHostSlots], evD2H[kHostSlots];
    // achip_ctx_get_stat("host.*"): where the last host-pointer batch of several chunks spent its wall time (microseconds)
    int64_t hostGatherUs = 0, hostScatterUs = 0, hostWaitSlotUs = 0, hostWaitDownloadUs = 0, hostChunks = 0, hostTotalUs = 0;
    // staging for the one-shot hashers (grown on demand)
    achip::host::PinnedBuffer<uint8_t> hostStage;
    achip::host::DeviceBuffer<uint8_t> devStage;
    int64_t stageBytes = 0;
};

namespace achip {
namespace host ACHIP_HIDDEN {

extern thread_local std::string g_lastError;  // achip_last_error (abi_context.cpp)

int32_t device_failure(const char* what, hipError_t e);
int32_t bad_argument(const char* what);
BatchArgs make_args(const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen,
                    int32_t* status, int64_t* errOffset, int32_t nBlocks);

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) {                                \
            return achip::host::device_failure(#expr, e_);     \
        }                                                      \
    } while (0)

// aircompressor_hip.h's ACHIP_OP_*, a row per value: is it an op, does it encode, and which codec family's lane of a mixed batch runs it (0 LZ4's, 1 Snappy's, 2 Zstd's)
struct OpRow {
    bool known, encoder;
    int family;
};
constexpr OpRow kOps[] = {
    {true, false, 0}, {true, true, 0},  // LZ4 block
    {true, false, 1}, {true, true, 1},  // Snappy block
    {true, false, 2}, {true, true, 2},  // Zstd frame
    {true, false, 0}, {true, true, 0},  // LZ4 frame
    {true, false, 1}, {true, true, 1},  // x-snappy-framed
    {true, false, 0}, {true, true, 0},  // Hadoop LZ4
    {true, false, 1}, {true, true, 1},  // Hadoop Snappy
    {true, true, 2}, {false, false, 2},  // Zstd stream: a writer only (its reader is achip_zstdstream_decompress_*), so 15 is no op
    {true, false, 0}, {true, true, 0},  // LZO (rides with LZ4's)
};
constexpr int kNumOps = (int)(sizeof(kOps) / sizeof(kOps[0]));
static_assert(ACHIP_OP_LZ4_DECOMPRESS == 0 && ACHIP_OP_LZ4_COMPRESS == 1 && ACHIP_OP_SNAPPY_DECOMPRESS == 2 && ACHIP_OP_SNAPPY_COMPRESS == 3 && ACHIP_OP_ZSTD_DECOMPRESS == 4 &&
                  ACHIP_OP_ZSTD_COMPRESS == 5 && ACHIP_OP_LZ4FRAME_DECOMPRESS == 6 && ACHIP_OP_LZ4FRAME_COMPRESS == 7 && ACHIP_OP_SNAPPYFRAMED_DECOMPRESS == 8 &&
                  ACHIP_OP_SNAPPYFRAMED_COMPRESS == 9 && ACHIP_OP_LZ4HADOOP_DECOMPRESS == 10 && ACHIP_OP_LZ4HADOOP_COMPRESS == 11 && ACHIP_OP_SNAPPYHADOOP_DECOMPRESS == 12 &&
                  ACHIP_OP_SNAPPYHADOOP_COMPRESS == 13 && ACHIP_OP_ZSTDSTREAM_COMPRESS == 14 && ACHIP_OP_LZO_DECOMPRESS == 16 && ACHIP_OP_LZO_COMPRESS == 17 && kNumOps == 18,
              "kOps has its rows in the order of ACHIP_OP_*");
static_assert(kOps[ACHIP_OP_ZSTDSTREAM_COMPRESS].encoder && kOps[ACHIP_OP_ZSTDSTREAM_COMPRESS].family == kOps[ACHIP_OP_ZSTD_COMPRESS].family && !kOps[15].known &&
                  !kOps[ACHIP_OP_LZO_DECOMPRESS].encoder && kOps[ACHIP_OP_LZO_COMPRESS].encoder && kOps[ACHIP_OP_LZO_COMPRESS].family == kOps[ACHIP_OP_LZ4_COMPRESS].family,
              "the rows that break the even-decodes, odd-encodes pattern");
inline bool op_known(int32_t op) { return op >= 0 && op < kNumOps && kOps[op].known; }
inline bool op_is_encoder(int32_t op) { return kOps[op].encoder; }  // (of a known op)
inline int op_family(int32_t op) { return kOps[op].family; }

// abi_dispatch.cpp
int32_t take_scratch(achip_ctx* ctx, int64_t bytes);  // the one way to the scratch for a launch: forgets what the last launch left in it (ctx->last), then ensure_scratch
// ... the two growth policies underneath it
int32_t ensure_scratch(achip_ctx* ctx, int64_t bytes);            // frees what is there first
int32_t grow_scratch_keeping_old(achip_ctx* ctx, int64_t bytes);  // allocates first, frees the old scratch only when that worked
void* zstd_mb_scratch(void* user, int64_t bytes);                 // the context's second, lazily grown buffer (ZstdMbProvider::get, AuxScratch)
int32_t launch_op(int32_t op, achip_ctx* ctx, const BatchArgs& args);
// abi_hash.cpp
int32_t ensure_stage(achip_ctx* ctx, int64_t bytes);  // the context's hostStage / devStage pair holds at least this much (the stream is idle when it had to grow)

}  // namespace host
}  // namespace achip
