// tools/hostemu/emu_window.cpp -- the windowed readers and writers of the chunked containers (achip_window_*: hadoop_streams.hip, snappy_frame.hip) under the fiber
// emulator: walk, the listed chunks through the block decoders, verify, fold, the wavefront-per-window kernel behind the fold; the window plans in front of the
// one-shot writers' encode and compact kernels.  Soft order points as in emu_all.cpp: the list path and the wavefront-per-window kernel run in one library.
// Driven by check_window.py.
#define HOSTEMU_ORDER_IS_SOFT 1
#include "emu.cpp"

// op: the container's ACHIP_OP_* (8 / 10 / 12 decompress, 9 / 11 / 13 compress)
extern "C" int emu_window(int op, int bufferSize, int variant, const int32_t* flags, const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase,
                          const int64_t* dstOff, const int32_t* dstCap, int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n, int64_t* consumed, int32_t* stop,
                          int64_t* need)
{
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, 16};
    const achip::WindowArgs w{flags, consumed, stop, need};
    static GuardedScratch scratch, auxBuffer;
    auxBuffer.assign(0);
    const achip::AuxScratch aux{[](void*, int64_t bytes) -> void* { return auxBuffer.assign(bytes); }, nullptr};
    int r = -1;
    switch (op) {
        case ACHIP_OP_SNAPPYFRAMED_DECOMPRESS:
            scratch.assign(achip::snappyframed_window_decompress_scratch_bytes(n));
            r = achip::launch_snappyframed_window_decompress(a, w, nullptr, scratch.v.data(), variant, &aux, achip::KernelSettings());
            break;
        case ACHIP_OP_LZ4HADOOP_DECOMPRESS:
        case ACHIP_OP_SNAPPYHADOOP_DECOMPRESS:
            scratch.assign(achip::hadoop_window_decompress_scratch_bytes(n, bufferSize));
            r = achip::launch_hadoop_window_decompress(a, w, nullptr, scratch.v.data(), op == ACHIP_OP_SNAPPYHADOOP_DECOMPRESS, bufferSize, variant, &aux, achip::KernelSettings());
            break;
        case ACHIP_OP_SNAPPYFRAMED_COMPRESS:
            scratch.assign(achip::snappyframed_window_compress_scratch_bytes(n));
            r = achip::launch_snappyframed_window_compress(a, w, nullptr, scratch.v.data(), achip::KernelSettings());
            break;
        case ACHIP_OP_LZ4HADOOP_COMPRESS:
        case ACHIP_OP_SNAPPYHADOOP_COMPRESS:
            scratch.assign(achip::hadoop_window_compress_scratch_bytes(n));
            r = achip::launch_hadoop_window_compress(a, w, nullptr, scratch.v.data(), op == ACHIP_OP_SNAPPYHADOOP_COMPRESS, bufferSize);
            break;
        default: return -1;
    }
    return auxBuffer.check("a window reader's record arena", scratch.check("a window call", r));
}
