// abi_window.cpp -- windows over the chunked containers (x-snappy-framed, Hadoop LZ4 / Snappy streams): the stateless incremental form of their readers and
// writers.  The device-resident batch calls (many streams' windows side by side) and the single host window staged through the context's pinned buffer; the
// kernels are hadoop_streams.hip's and snappy_frame.hip's window forms.
#include "achip_host.h"

using namespace achip::host;

namespace {

bool is_window_op(int32_t op, bool compress)
{
    if (compress) return op == ACHIP_OP_SNAPPYFRAMED_COMPRESS || op == ACHIP_OP_LZ4HADOOP_COMPRESS || op == ACHIP_OP_SNAPPYHADOOP_COMPRESS;
    return op == ACHIP_OP_SNAPPYFRAMED_DECOMPRESS || op == ACHIP_OP_LZ4HADOOP_DECOMPRESS || op == ACHIP_OP_SNAPPYHADOOP_DECOMPRESS;
}

int32_t launch_window(achip_ctx* ctx, int32_t op, const achip::BatchArgs& args, const achip::WindowArgs& w)
{
    achip::BatchArgs a = args;
    a.ringPad = ctx->ringPad;
    HIP_TRY(hipSetDevice(ctx->device));
    const achip::AuxScratch aux{zstd_mb_scratch, ctx};  // (the context's second, lazily grown buffer: the two-pass decoders' record arena)
    hipError_t e = hipSuccess;
    switch (op) {
        case ACHIP_OP_SNAPPYFRAMED_DECOMPRESS:
            if (const int32_t r = take_scratch(ctx, achip::snappyframed_window_decompress_scratch_bytes(a.nBlocks)); r < 0) return r;
            e = achip::launch_snappyframed_window_decompress(a, w, ctx->stream.get(), ctx->scratch.get(), ctx->snappyFramedVariant == 0 ? 3 : ctx->snappyFramedVariant, &aux, ctx->kernel);
            break;
        case ACHIP_OP_LZ4HADOOP_DECOMPRESS:
        case ACHIP_OP_SNAPPYHADOOP_DECOMPRESS:
            if (const int32_t r = take_scratch(ctx, achip::hadoop_window_decompress_scratch_bytes(a.nBlocks, ctx->hadoopBufferSize)); r < 0) return r;
            e = achip::launch_hadoop_window_decompress(a, w, ctx->stream.get(), ctx->scratch.get(), op == ACHIP_OP_SNAPPYHADOOP_DECOMPRESS, ctx->hadoopBufferSize,
                                                       ctx->hadoopDecompressVariant == 0 ? 3 : ctx->hadoopDecompressVariant, &aux, ctx->kernel);
            break;
        case ACHIP_OP_SNAPPYFRAMED_COMPRESS:
            if (const int32_t r = take_scratch(ctx, achip::snappyframed_window_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            e = achip::launch_snappyframed_window_compress(a, w, ctx->stream.get(), ctx->scratch.get(), ctx->kernel);
            break;
        default:
            if (const int32_t r = take_scratch(ctx, achip::hadoop_window_compress_scratch_bytes(a.nBlocks)); r < 0) return r;
            e = achip::launch_hadoop_window_compress(a, w, ctx->stream.get(), ctx->scratch.get(), op == ACHIP_OP_SNAPPYHADOOP_COMPRESS, ctx->hadoopBufferSize);
            break;
    }
    return e != hipSuccess ? device_failure("kernel launch", e) : 0;
}

// (the value arguments are checked before the context is looked at: a caller's mistake is reported the same with and without a device)
int32_t window_batch(bool compress, achip_ctx* ctx, int32_t codecOp, const int32_t* flags, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                     const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks, int64_t* consumed, int32_t* stop,
                     int64_t* need)
{
    if (!is_window_op(codecOp, compress)) return bad_argument(compress ? "codecOp is not a container compress op" : "codecOp is not a container decompress op");
    if (nBlocks < 0) return bad_argument("nBlocks < 0");
    if (nBlocks == 0) return 0;
    if (!flags || !srcOff || !srcLen || !dstOff || !dstCap || !outLen || !status || !errOffset || !consumed || !stop || !need) return bad_argument("null array");
    if (!ctx) return bad_argument("ctx is null");
    return launch_window(ctx, codecOp, make_args(srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks), achip::WindowArgs{flags, consumed, stop, need});
}

// one host window: [input | room for the output | the call's arrays] in the context's staging pair, one upload, the batch call over one item, one download
struct WindowMeta {
    int64_t srcOff, dstOff, errOffset, consumed, need;
    int32_t srcLen, dstCap, outLen, status, stop, flags;
};

int32_t window_host(bool compress, achip_ctx* ctx, int32_t codecOp, int32_t flags, const void* src, int32_t srcLen, void* dst, int32_t dstCap, int64_t* consumed,
                    int64_t* produced, int32_t* stop, int64_t* need, int64_t* errOffset)
{
    if (!is_window_op(codecOp, compress)) return bad_argument(compress ? "codecOp is not a container compress op" : "codecOp is not a container decompress op");
    if (srcLen < 0 || dstCap < 0) return bad_argument("negative length");
    if ((flags & ~(ACHIP_WINDOW_FIRST | ACHIP_WINDOW_LAST)) != 0) return bad_argument("unknown window flag");
    if (!consumed || !produced || !stop || !need || !errOffset) return bad_argument("null result pointer");
    if ((srcLen > 0 && !src) || (dstCap > 0 && !dst)) return bad_argument("null buffer");
    if (!ctx) return bad_argument("ctx is null");
    const int64_t dstAt = ((int64_t)srcLen + 63) & ~63LL;
    const int64_t metaAt = (dstAt + dstCap + 63) & ~63LL;
    if (const int32_t r = ensure_stage(ctx, metaAt + (int64_t)sizeof(WindowMeta)); r < 0) return r;
    uint8_t* h = ctx->hostStage.get();
    uint8_t* d = ctx->devStage.get();
    if (srcLen > 0) memcpy(h, src, (size_t)srcLen);
    WindowMeta* m = (WindowMeta*)(h + metaAt);
    *m = WindowMeta{0, dstAt, 0, 0, 0, srcLen, dstCap, 0, 0, 0, flags};
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream.get();
    if (srcLen > 0) HIP_TRY(hipMemcpyAsync(d, h, (size_t)srcLen, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + metaAt, h + metaAt, sizeof(WindowMeta), hipMemcpyHostToDevice, s));
    WindowMeta* dm = (WindowMeta*)(d + metaAt);
    const int32_t r = window_batch(compress, ctx, codecOp, &dm->flags, d, &dm->srcOff, &dm->srcLen, d, &dm->dstOff, &dm->dstCap, &dm->outLen, &dm->status, &dm->errOffset, 1,
                                   &dm->consumed, &dm->stop, &dm->need);
    if (r < 0) {
        (void)hipStreamSynchronize(s);
        return r;
    }
    HIP_TRY(hipMemcpyAsync(h + metaAt, d + metaAt, sizeof(WindowMeta), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (m->outLen > 0) {  // (the length is known only now: a second, exact download instead of dstCap bytes every time)
        HIP_TRY(hipMemcpyAsync(h + dstAt, d + dstAt, (size_t)m->outLen, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(dst, h + dstAt, (size_t)m->outLen);
    }
    *consumed = m->consumed;
    *produced = m->outLen;
    *stop = m->stop;
    *need = m->need;
    *errOffset = m->errOffset;
    return m->status;
}

}  // namespace

extern "C" {

int32_t achip_window_decompress_batch(achip_ctx* ctx, int32_t codecOp, const int32_t* flags, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                                      const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks, int64_t* consumed,
                                      int32_t* stop, int64_t* need)
{
    return window_batch(false, ctx, codecOp, flags, srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks, consumed, stop, need);
}

int32_t achip_window_compress_batch(achip_ctx* ctx, int32_t codecOp, const int32_t* flags, const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, void* dstBase,
                                    const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t nBlocks, int64_t* consumed,
                                    int32_t* stop, int64_t* need)
{
    return window_batch(true, ctx, codecOp, flags, srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, nBlocks, consumed, stop, need);
}

int32_t achip_window_decompress(achip_ctx* ctx, int32_t codecOp, int32_t flags, const void* src, int32_t srcLen, void* dst, int32_t dstCap, int64_t* consumed, int64_t* produced,
                                int32_t* stop, int64_t* need, int64_t* errOffset)
{
    return window_host(false, ctx, codecOp, flags, src, srcLen, dst, dstCap, consumed, produced, stop, need, errOffset);
}

int32_t achip_window_compress(achip_ctx* ctx, int32_t codecOp, int32_t flags, const void* src, int32_t srcLen, void* dst, int32_t dstCap, int64_t* consumed, int64_t* produced,
                              int32_t* stop, int64_t* need, int64_t* errOffset)
{
    return window_host(true, ctx, codecOp, flags, src, srcLen, dst, dstCap, consumed, produced, stop, need, errOffset);
}

}  // extern "C"
