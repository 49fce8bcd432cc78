// tools/hostemu/emu_snf_params.cpp -- the x-snappy-framed writers and readers of snappy_frame.hip with the parameters of achip_ctx_set_snappyframed_writer and
// achip_ctx_set_snappyframed_verify_checksums, on the CPU.  Built twice (tools/hostemu/build.sh snf_params):
//   libemu_snf_params_w.so  -DSNF_PARAMS_WRITERS: every memory access an order point and wave_mem_order() a rendezvous, like emu_enc.cpp -- the block encoder
//                           changes its hash table in place and is exact only under the device's lockstep.  The writers: a wavefront per stream, the block
//                           list, the serial kernel over the streams a list marks, the window writer.
//   libemu_snf_params_r.so  soft order points, like emu_all.cpp and emu_window.cpp: the list path and the wavefront-per-stream kernel in one library.  The readers:
//                           variants 0 .. 3 and the window reader.
// Driven by check_snf_params.py.
#ifdef SNF_PARAMS_WRITERS
#define HOSTEMU_ACCESS_LOCKSTEP 1
#define HOSTEMU_ORDER_IS_RENDEZVOUS 1
#else
#define HOSTEMU_ORDER_IS_SOFT 1
#endif
#include "emu.cpp"

namespace {
achip::KernelSettings snf_settings(int32_t checksums, int32_t blockSize, int64_t ratioBits, int32_t verify)
{
    achip::KernelSettings ks;
    if (achip::set_snf_writer(ks, checksums, blockSize, ratioBits) != achip::SnfRefusal::None || achip::set_snf_verify(ks, verify) != achip::SnfRefusal::None) {
        fprintf(stderr, "hostemu: x-snappy-framed parameters refused\n");
        abort();
    }
    ks.snfEncodeWorkgroups = 2;  // (the persistent grid: the emulator runs its wavefronts one after the other)
    return ks;
}
}  // namespace

// variant 0: a wavefront per stream; 1: the block list (encode + compact, and the serial kernel over the streams that do not fit into a list of `listEntries`
// entries; 0: the product's 2^20)
extern "C" int emu_snf_write(int variant, int32_t listEntries, int32_t checksums, int32_t blockSize, int64_t ratioBits, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen,
                             uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 0};
    static GuardedScratch scratch;
    if (scratch.size() != achip::snappyframed_compress_scratch_bytes(n)) scratch.assign(achip::snappyframed_compress_scratch_bytes(n));
    achip::KernelSettings ks = snf_settings(checksums, blockSize, ratioBits, 1);
    ks.snfListEntries = listEntries;
    return scratch.check("the x-snappy-framed writer", achip::launch_snappyframed_compress(a, nullptr, scratch.v.data(), variant, ks));
}

extern "C" int emu_snf_read(int variant, int32_t verify, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff,
                            const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 16};
    static GuardedScratch scratch, auxBuffer;
    scratch.assign(achip::snappyframed_decompress_scratch_bytes(n));
    auxBuffer.assign(0);
    const achip::AuxScratch aux{[](void*, int64_t bytes) -> void* { return auxBuffer.assign(bytes); }, nullptr};
    const int r = achip::launch_snappyframed_decompress(a, nullptr, scratch.v.data(), variant, &aux, snf_settings(1, 65536, ACHIP_SNF_DEFAULT_MIN_RATIO_BITS, verify));
    return auxBuffer.check("the x-snappy-framed reader's record arena", scratch.check("the x-snappy-framed reader", r));
}

// the entries of the window writer's block list (0: the product's 2^20): a small list makes windows stop at their share of it
static int32_t g_windowListEntries = 0;
extern "C" void emu_snf_window_list_entries(int32_t entries) { g_windowListEntries = entries; }

// compress != 0: the window writer with the writer's parameters; else the window reader (variant 1 .. 3) with `verify`
extern "C" int emu_snf_window(int compress, int variant, int32_t checksums, int32_t blockSize, int64_t ratioBits, int32_t verify, const int32_t* flags, const uint8_t* srcBase,
                              const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status,
                              int64_t* errOffset, int32_t n, int64_t* consumed, int32_t* stop, int64_t* need)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 16};
    const achip::WindowArgs w{flags, consumed, stop, need};
    achip::KernelSettings ks = snf_settings(checksums, blockSize, ratioBits, verify);
    ks.snfListEntries = g_windowListEntries;
    static GuardedScratch scratch, auxBuffer;
    auxBuffer.assign(0);
    const achip::AuxScratch aux{[](void*, int64_t bytes) -> void* { return auxBuffer.assign(bytes); }, nullptr};
    int r;
    if (compress) {
        if (scratch.size() != achip::snappyframed_window_compress_scratch_bytes(n)) scratch.assign(achip::snappyframed_window_compress_scratch_bytes(n));
        r = achip::launch_snappyframed_window_compress(a, w, nullptr, scratch.v.data(), ks);
    }
    else {
        scratch.assign(achip::snappyframed_window_decompress_scratch_bytes(n));
        r = achip::launch_snappyframed_window_decompress(a, w, nullptr, scratch.v.data(), variant, &aux, ks);
    }
    return auxBuffer.check("a window reader's record arena", scratch.check("a window call", r));
}
