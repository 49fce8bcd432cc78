// abi_hash.cpp -- the xxHash entry points: batches over device memory, one buffer from host memory, states in device memory that are reset / updated /
// digested (xxhash_stream.hip), and achip_hasher_*: one such state fed from host memory.
#include "achip_host.h"

#include "achip_xxh_stream.h"

using namespace achip::host;

namespace achip {
namespace host ACHIP_HIDDEN {

// pinned + device staging for bytes that arrive in host memory (grown on demand, at least 1 MiB)
int32_t ensure_stage(achip_ctx* ctx, int64_t bytes)
{
    if (bytes <= ctx->stageBytes) {
        return 0;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    ctx->stageBytes = 0;
    HIP_TRY(ctx->hostStage.reset());
    HIP_TRY(ctx->devStage.reset());
    int64_t want = std::max<int64_t>(bytes, 1 << 20);
    HIP_TRY(ctx->hostStage.alloc((size_t)want));
    HIP_TRY(ctx->devStage.alloc((size_t)want));
    ctx->stageBytes = want;
    return 0;
}

}  // namespace host
}  // namespace achip

// The body of every hash batch: its checks (countName: what the count is called in its error text), then its launch -- a macro, so that a failed launch is
// reported by the call's own text.
#define ACHIP_HASH_BATCH(arrays, n, countName, call)               \
    do {                                                           \
        if (!ctx) return bad_argument("ctx is null");              \
        if ((n) < 0) return bad_argument(countName);               \
        if ((n) == 0) return 0;                                    \
        if (!(arrays)) return bad_argument("null array");          \
        HIP_TRY(hipSetDevice(ctx->device));                        \
        HIP_TRY(call);                                             \
        return 0;                                                  \
    } while (0)

extern "C" {

// ---- xxhash -------------------------------------------
int32_t achip_xxhash64_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t seed, int64_t* outHash, int32_t nBuffers)
{
    ACHIP_HASH_BATCH(srcOff && srcLen && outHash, nBuffers, "nBuffers < 0", achip::launch_xxh64_batch(srcBase, srcOff, srcLen, nBuffers, (uint64_t)seed, outHash, ctx->stream.get()));
}

int32_t achip_xxhash32_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t seed, int32_t* outHash, int32_t nBuffers)
{
    ACHIP_HASH_BATCH(srcOff && srcLen && outHash, nBuffers, "nBuffers < 0", achip::launch_xxh32_batch(srcBase, srcOff, srcLen, nBuffers, (uint32_t)seed, outHash, ctx->stream.get()));
}

int32_t achip_xxhash3_64_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t seed, int64_t* outHash, int32_t nBuffers)
{
    ACHIP_HASH_BATCH(srcOff && srcLen && outHash, nBuffers, "nBuffers < 0", achip::launch_xxh3_batch(srcBase, srcOff, srcLen, nBuffers, (uint64_t)seed, false, outHash, ctx->stream.get()));
}

int32_t achip_xxhash3_128_batch(achip_ctx* ctx, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int64_t seed, int64_t* outHash, int32_t nBuffers)
{
    ACHIP_HASH_BATCH(srcOff && srcLen && outHash, nBuffers, "nBuffers < 0", achip::launch_xxh3_batch(srcBase, srcOff, srcLen, nBuffers, (uint64_t)seed, true, outHash, ctx->stream.get()));
}

namespace {
enum class HostHash { XXH32, XXH64, XXH3_64, XXH3_128 };
// one host buffer: staged to the device, hashed there, 8 bytes back (16 for XXH3_128: out[0] = low, out[1] = high)
int32_t hash_host(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, HostHash kind, int64_t* out)
{
    if (!ctx) return bad_argument("ctx is null");
    if (srcLen < 0 || srcLen > 0x7FFFFFFF) return bad_argument("length out of range");
    if (srcLen > 0 && !src) return bad_argument("src is null");
    const int64_t metaOff = (srcLen + 63) & ~63LL;
    int32_t r = ensure_stage(ctx, metaOff + 64);
    if (r < 0) return r;
    uint8_t* h = ctx->hostStage.get();
    uint8_t* d = ctx->devStage.get();
    if (srcLen > 0) memcpy(h, src, (size_t)srcLen);
    *(int64_t*)(h + metaOff) = 0;                      // srcOff
    *(int32_t*)(h + metaOff + 8) = (int32_t)srcLen;    // srcLen
    *(int64_t*)(h + metaOff + 16) = 0;                 // result (16 bytes)
    *(int64_t*)(h + metaOff + 24) = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(d, h, (size_t)(metaOff + 64), hipMemcpyHostToDevice, ctx->stream.get()));
    const int64_t* dOff = (const int64_t*)(d + metaOff);
    const int32_t* dLen = (const int32_t*)(d + metaOff + 8);
    int64_t* dOut = (int64_t*)(d + metaOff + 16);
    switch (kind) {
    case HostHash::XXH32: HIP_TRY(achip::launch_xxh32_batch(d, dOff, dLen, 1, (uint32_t)seed, (int32_t*)dOut, ctx->stream.get())); break;
    case HostHash::XXH64: HIP_TRY(achip::launch_xxh64_batch(d, dOff, dLen, 1, (uint64_t)seed, dOut, ctx->stream.get())); break;
    case HostHash::XXH3_64: HIP_TRY(achip::launch_xxh3_batch(d, dOff, dLen, 1, (uint64_t)seed, false, dOut, ctx->stream.get())); break;
    case HostHash::XXH3_128: HIP_TRY(achip::launch_xxh3_batch(d, dOff, dLen, 1, (uint64_t)seed, true, dOut, ctx->stream.get())); break;
    }
    const int words = kind == HostHash::XXH3_128 ? 2 : 1;
    HIP_TRY(hipMemcpyAsync(h + metaOff + 16, d + metaOff + 16, (size_t)(8 * words), hipMemcpyDeviceToHost, ctx->stream.get()));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    for (int k = 0; k < words; k++) out[k] = *(int64_t*)(h + metaOff + 16 + 8 * k);
    return 0;
}
}  // namespace

int32_t achip_xxhash64(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, int64_t* outHash)
{
    if (!outHash) return bad_argument("outHash is null");
    return hash_host(ctx, src, srcLen, seed, HostHash::XXH64, outHash);
}

int32_t achip_xxhash32(achip_ctx* ctx, const void* src, int64_t srcLen, int32_t seed, int32_t* outHash)
{
    if (!outHash) return bad_argument("outHash is null");
    int64_t v = 0;
    const int32_t r = hash_host(ctx, src, srcLen, seed, HostHash::XXH32, &v);
    *outHash = (int32_t)v;
    return r;
}

int32_t achip_xxhash3_64(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, int64_t* outHash)
{
    if (!outHash) return bad_argument("outHash is null");
    return hash_host(ctx, src, srcLen, seed, HostHash::XXH3_64, outHash);
}

int32_t achip_xxhash3_128(achip_ctx* ctx, const void* src, int64_t srcLen, int64_t seed, int64_t* outHash)
{
    if (!outHash) return bad_argument("outHash is null");
    return hash_host(ctx, src, srcLen, seed, HostHash::XXH3_128, outHash);
}

// ---- streaming hashers (xxhash_stream.hip): states in device memory, reset / update / digest ----
int64_t achip_hash_state_size(int32_t algo)
{
    const int64_t n = achip::hash_state_size(algo);
    return n > 0 ? n : bad_argument("unknown hash algorithm");
}

int32_t achip_hash_states_reset(achip_ctx* ctx, int32_t algo, void* states, int32_t nStates, int64_t seed)
{
    if (achip::hash_state_size(algo) < 0) return bad_argument("unknown hash algorithm");
    ACHIP_HASH_BATCH(states, nStates, "nStates < 0", achip::launch_hash_states_reset(algo, states, nStates, (uint64_t)seed, ctx->stream.get()));
}

int32_t achip_hash_states_update(achip_ctx* ctx, int32_t algo, void* states, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t nStates)
{
    if (achip::hash_state_size(algo) < 0) return bad_argument("unknown hash algorithm");
    ACHIP_HASH_BATCH(states && srcOff && srcLen, nStates, "nStates < 0", achip::launch_hash_states_update(algo, states, srcBase, srcOff, srcLen, nStates, ctx->stream.get()));
}

int32_t achip_hash_states_digest(achip_ctx* ctx, int32_t algo, const void* states, int64_t* outHash, int32_t nStates)
{
    if (achip::hash_state_size(algo) < 0) return bad_argument("unknown hash algorithm");
    ACHIP_HASH_BATCH(states && outHash, nStates, "nStates < 0", achip::launch_hash_states_digest(algo, states, outHash, nStates, ctx->stream.get()));
}

// One stream fed from HOST memory: a single state in device memory of its own, and the context's pinned staging for the bytes (a chunk at a
// time: the staging is the context's, so a chunk is absorbed before the next one overwrites it).
namespace {
constexpr int64_t kHasherChunk = 1 << 20;
struct HostHasher {
    achip_ctx* ctx;
    int32_t algo;
    int64_t stateBytes;
    DeviceBuffer<uint8_t> dev;  // the state, then srcOff (8), srcLen (4 + 4), the result (16)
    ~HostHasher() { (void)hipSetDevice(ctx->device); }
};
}  // namespace

void* achip_hasher_create(achip_ctx* ctx, int32_t algo, int64_t seed)
{
    const int64_t stateBytes = achip::hash_state_size(algo);
    if (stateBytes < 0) {
        bad_argument("unknown hash algorithm");
        return nullptr;
    }
    if (!ctx) {
        bad_argument("ctx is null");
        return nullptr;
    }
    HostHasher* h = new HostHasher{ctx, algo, stateBytes};
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = h->dev.alloc((size_t)(stateBytes + 32));
    if (e == hipSuccess) e = achip::launch_hash_states_reset(algo, h->dev.get(), 1, (uint64_t)seed, ctx->stream.get());
    if (e != hipSuccess) {
        device_failure("achip_hasher_create", e);
        delete h;
        return nullptr;
    }
    return h;
}

int32_t achip_hasher_update(void* hasher, const void* src, int64_t srcLen)
{
    HostHasher* h = (HostHasher*)hasher;
    if (!h) return bad_argument("hasher is null");
    if (srcLen < 0) return bad_argument("srcLen < 0");
    if (srcLen > 0 && !src) return bad_argument("src is null");
    achip_ctx* ctx = h->ctx;
    for (int64_t at = 0; at < srcLen; at += kHasherChunk) {
        const int64_t n = std::min(kHasherChunk, srcLen - at);
        const int32_t r = ensure_stage(ctx, kHasherChunk + 64);
        if (r < 0) return r;
        uint8_t* hs = ctx->hostStage.get();
        uint8_t* ds = ctx->devStage.get();
        memcpy(hs, (const uint8_t*)src + at, (size_t)n);
        *(int64_t*)(hs + kHasherChunk) = 0;               // srcOff
        *(int32_t*)(hs + kHasherChunk + 8) = (int32_t)n;  // srcLen
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipMemcpyAsync(ds, hs, (size_t)n, hipMemcpyHostToDevice, ctx->stream.get()));
        HIP_TRY(hipMemcpyAsync(ds + kHasherChunk, hs + kHasherChunk, 16, hipMemcpyHostToDevice, ctx->stream.get()));
        HIP_TRY(achip::launch_hash_states_update(h->algo, h->dev.get(), ds, (const int64_t*)(ds + kHasherChunk), (const int32_t*)(ds + kHasherChunk + 8), 1, ctx->stream.get()));
        HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    }
    return 0;
}

int32_t achip_hasher_digest(void* hasher, int64_t* out)
{
    HostHasher* h = (HostHasher*)hasher;
    if (!h) return bad_argument("hasher is null");
    if (!out) return bad_argument("out is null");
    achip_ctx* ctx = h->ctx;
    int64_t* dOut = (int64_t*)(h->dev.get() + h->stateBytes + 16);
    int64_t got[2] = {0, 0};
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(achip::launch_hash_states_digest(h->algo, h->dev.get(), dOut, 1, ctx->stream.get()));
    HIP_TRY(hipMemcpyAsync(got, dOut, h->algo == achip::HASH_XXH3_128 ? 16 : 8, hipMemcpyDeviceToHost, ctx->stream.get()));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    out[0] = got[0];
    out[1] = got[1];
    return 0;
}

int32_t achip_hasher_reset(void* hasher, int64_t seed)
{
    HostHasher* h = (HostHasher*)hasher;
    if (!h) return bad_argument("hasher is null");
    HIP_TRY(hipSetDevice(h->ctx->device));
    HIP_TRY(achip::launch_hash_states_reset(h->algo, h->dev.get(), 1, (uint64_t)seed, h->ctx->stream.get()));
    return 0;
}

int32_t achip_hasher_destroy(void* hasher)
{
    HostHasher* h = (HostHasher*)hasher;
    if (!h) return bad_argument("hasher is null");
    achip_ctx* ctx = h->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream.get()));
    HIP_TRY(h->dev.reset());
    delete h;
    return 0;
}

}  // extern "C"
