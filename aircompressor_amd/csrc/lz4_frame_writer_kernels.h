// lz4_frame_writer_kernels.h -- the encode kernel of lz4_frame_writer.hip (which has the design notes and the launcher).  Included TWICE, with no include guard, by the
// scheme of lz4_compress_kernels.h: LZ4K(name) = name with LZ4K_PARAM empty, LZ4K_ACCEL false, LZ4K_VALUE 1, and LZ4K(name) = name##_accel with the acceleration
// of Lz4Compressor.create(acceleration) as one more argument.

// A persistent grid of wavefronts draws the list's entries: block k of its frame goes through the block encoder into its worst-case place inside the frame's own
// destination -- 4 bytes behind the slot's start, where the compaction will put the size field if the block stays where it is.  WIDE: the table holds int32_t
// entries for blocks beyond 64 KiB (16 KiB of LDS: ten wavefronts a CU); a launch whose block-maximum size is 64 KiB takes the other form (8 KiB: twenty).
template <bool WIDE>
__global__ __launch_bounds__(64) void LZ4K(lz4f_list_encode_kernel)(BatchArgs a, lz4fw::BlockList L, lz4fw::Frame f LZ4K_PARAM)
{
    __shared__ __attribute__((aligned(16))) uint8_t tableBytes[lz4c::MAX_TABLE_SIZE * (WIDE ? 4 : 2)];
    const int lane = threadIdx.x;
    const int32_t total = L.counters[1];
    const int64_t worst = lz4fw::slot_bytes(f);
    for (;;) {
        int32_t b = 0;
        if (lane == 0) {
            b = atomicAdd(L.counters + 2, 1);
        }
        b = __builtin_amdgcn_readfirstlane(b);
        if (b >= total) {
            return;
        }
        const int32_t stream = L.bStream[b];
        if (stream < 0) {
            continue;
        }
        const int32_t k = L.bIndex[b];
        const int64_t pos = (int64_t)k * f.blockMax;
        const int32_t inLen = a.srcLen[stream];
        const int32_t length = (int32_t)(inLen - pos < f.blockMax ? inLen - pos : f.blockMax);
        const uint8_t* block = a.srcBase + a.srcOff[stream] + pos;
        uint8_t* out = a.dstBase + a.dstOff[stream] + lz4fw::header_bytes(f) + (int64_t)k * worst + 4;
        const int32_t cap = (int32_t)bound::lz4(length);
        int32_t cst = 0, compressed = 0;
        if (!WIDE || length <= 65536) {
            compressed = lz4_compress_block_mw<uint16_t, LZ4K_ACCEL>(block, length, out, cap, (uint16_t*)tableBytes, lane, cst, LZ4K_VALUE);
        }
        else {
            compressed = lz4_compress_block_mw<int32_t, LZ4K_ACCEL>(block, length, out, cap, (int32_t*)tableBytes, lane, cst, LZ4K_VALUE);
        }
        wave_mem_order();
        const bool kept = cst == 0 && compressed < length;  // Lz4FrameCompression.java:114-126: a block that did not shrink is stored
        uint32_t sum = 0;
        if (f.blockChecksum) {  // of the block's data as the frame will hold it, by the wavefront that has it hot
            sum = quad_xxh32(kept ? (const uint8_t*)out : block, kept ? compressed : length, 0u, lane & 3, lane - (lane & 3));
        }
        if (lane == 0) {
            L.bSize[b] = kept ? compressed : -1;
            L.bSum[b] = sum;
        }
        wave_mem_order();
    }
}
