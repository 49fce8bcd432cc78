// achip_launch.h -- the host launchers one translation unit calls in another: the host units (abi_*.cpp, over achip_host.h) call them all, the container readers hand their
// listed blocks to launch_listed_decode (block_decode.cpp), which calls the block decoders, the Zstd decoder's two halves call each other, and
// tools/hostemu calls them on the CPU.  Every file that defines or calls one includes this header.
#pragma once
#include "achip_device.h"
#include "achip_settings.h"

namespace achip {

namespace sx {
struct BlockMeta;
}
namespace zd {
struct FseTable;
}

// ---- LZ4 / Snappy block decoders ----
// ring decoders (lz4_decompress_v2.hip, snappy_decompress_v2.hip) and their lanes per block by the batch size
hipError_t launch_lz4_decompress_rings(const BatchArgs& a, hipStream_t stream, int groupSize, int ringClass, const int32_t* mixedGroups);
hipError_t launch_snappy_decompress_rings(const BatchArgs& a, hipStream_t stream, int groupSize, int ringClass, const int32_t* mixedGroups);
int lz4_ring_group_for(int32_t nBlocks);
int snappy_ring_group_for(int32_t nBlocks);
// two-pass decoders (lz4_decompress_v7.hip, snappy_decompress_v5.hip): parse to records, a wavefront per block executes them
hipError_t launch_lz4_decompress_twopass(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int groupSize, int ringClass, const int32_t* stats, const KernelSettings& ks);
hipError_t launch_snappy_decompress_twopass(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int groupSize, int ringClass, const int32_t* stats, const KernelSettings& ks);
// what the two wrappers above share (lz4_decompress_v7.hip): memset, the parser by `parse` and the batch, the executor, the ring decoder for what is left
namespace sx {
struct ArenaHeader;
}
using TwoPassParseKernel = void (*)(BatchArgs a, sx::ArenaHeader* hdr, sx::BlockMeta* meta, int32_t* only, uint64_t* arena, int32_t maxChunks, const int32_t* stats);
hipError_t launch_twopass(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int groupSize, int ringClass, const int32_t* stats, int parse,
                          int32_t waveMaxBlocks, int32_t shortLimit, TwoPassParseKernel laneParser, TwoPassParseKernel waveParser,
                          hipError_t (*rings)(const BatchArgs&, hipStream_t, int, int, const int32_t*));
hipError_t launch_seq_execute2(const BatchArgs& a, hipStream_t stream, const sx::BlockMeta* meta, const uint64_t* arena, const int32_t* stats, int32_t shortLimit);
int64_t twopass_scratch_bytes(int32_t nBlocks, int64_t perBlock);
// record arena per block of the two-pass decoders (8 bytes per record; lz4_decompress_v7.hip: text-like 64 KiB blocks make 6 000 .. 8 500 LZ4
// records, 8 500 .. 11 500 Snappy records), and the least it is worth running them with (blocks that do not fit go to the ring decoder)
constexpr int64_t LZ4_RECORD_BYTES_PER_BLOCK = 98304, LZ4_RECORD_BYTES_PER_BLOCK_MIN = 32768;
constexpr int64_t SNAPPY_RECORD_BYTES_PER_BLOCK = 131072, SNAPPY_RECORD_BYTES_PER_BLOCK_MIN = 49152;
// auto mode's probes (decode_probes.hip)
hipError_t launch_lz4_mixed_groups(const BatchArgs& a, hipStream_t stream, int32_t* mixedGroups, int32_t minBlocks);
hipError_t launch_lz4_sequence_sample(const BatchArgs& a, hipStream_t stream, int32_t* stats, int32_t minBlocks, int32_t shortLimit);
hipError_t launch_snappy_element_sample(const BatchArgs& a, hipStream_t stream, int32_t* stats, int32_t minBlocks, int32_t shortLimit);
// the two families as one table (block_decode.cpp), a row per family -- 0 LZ4, 1 Snappy: the block API's policy (abi_dispatch.cpp launch_block_decode) and
// the containers' (launch_listed_decode) read the same row
struct BlockCodec {
    hipError_t (*rings)(const BatchArgs& a, hipStream_t stream, int groupSize, int ringClass, const int32_t* mixedGroups);
    hipError_t (*twopass)(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int groupSize, int ringClass, const int32_t* stats, const KernelSettings& ks);
    hipError_t (*sample)(const BatchArgs& a, hipStream_t stream, int32_t* stats, int32_t minBlocks, int32_t shortLimit);  // auto mode's probe of the lengths
    int (*groupFor)(int32_t nBlocks);     // ring decoder lanes per block by the batch size
    int64_t recordBytes, recordBytesMin;  // the two-pass decoder's record arena per block
    int32_t shortLimit;                   // sequences (LZ4) / elements (Snappy) shorter than this are short ones (lz4_pick)
};
extern const BlockCodec kBlockCodecs[2];
// What a container reader wants for the batch it listed on the device (lists::ChunkBatch::as_batch).
struct ListedWant {
    bool sync;            // false: the host never learns the count -- no synchronisation, the launches are sized for the list's capacity
    bool probe;           // (sync) true: the family's length probe decides between the two passes and the rings; false: always the two passes
    bool ringsWithoutArena;  // (sync) the two passes wanted but no arena to be had: true = the rings instead, false = nothing is decoded
    int64_t recordScale;  // arena per listed block: the family's recordBytes x this ...
    int roomWord;         // ... or, if >= 0 and larger, 3/2 of the blocks' mean room, rounded up to 4 KiB, from the 64-bit sum at counters[roomWord]
};
// The one decode path of a listed batch.  `counters`: the list's ([1] = its sealed count); `stats`: four probe words at most 60 words behind
// `counters`, zero on entry (the readers clear their counter page once).  *decoded: a decoder was launched over the list.
hipError_t launch_listed_decode(const BatchArgs& listed, int fam, hipStream_t stream, const int32_t* counters, int32_t* stats, const AuxScratch* aux, const KernelSettings& ks,
                                const ListedWant& want, bool* decoded);

// ---- LZO (lzo_decompress.hip, lzo_compress.hip) ----
// a wavefront per item (honours a.only); and the two passes: the lane parser, the record executor, the wavefront decoder for what the parser handed over
hipError_t launch_lzo_decompress_wave(const BatchArgs& a, hipStream_t stream);
// (maxChunks > 0: no more than that many 4 KiB chunks of the arena are used -- option "lzo.decompress.max_chunks", a test's way to an exhausted arena)
hipError_t launch_lzo_decompress_twopass(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int32_t maxChunks);
hipError_t launch_lzo_compress(const BatchArgs& a, hipStream_t stream);

// ---- LZ4 / Snappy block encoders ----
// the two-tier LZ4 kernel runs only with at least lz4_compress_scratch_bytes() of scratch (scratchBytes); with less, the one-wavefront kernel writes the same bytes
hipError_t launch_lz4_compress(const BatchArgs& a, hipStream_t stream, int variant, int maxSrcLenHint, void* scratch, int64_t scratchBytes, const KernelSettings& ks);
int64_t lz4_compress_scratch_bytes();
hipError_t launch_snappy_compress(const BatchArgs& a, hipStream_t stream, int variant, void* scratch, bool fan, const KernelSettings& ks);
int64_t snappy_compress_scratch_bytes(int32_t nBlocks);

// ---- Zstd ----
hipError_t launch_zstd_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int variant, int32_t tileMax, const ZstdMbProvider* mbp, const KernelSettings& ks);
int64_t zstd_decompress_scratch_bytes(int32_t nBlocks, int32_t tileMax);
// the pipeline (zstd_decompress_pipe.hip) and the one-kernel decoder it hands items to (zstd_decompress.hip)
hipError_t launch_zstd_decompress_pipe(const BatchArgs& a, hipStream_t stream, void* scratch, void* generalScratch, int32_t tileMax, const ZstdMbProvider* mbp, const KernelSettings& ks);
int64_t zstd_decompress_pipe_scratch_bytes(int32_t nBlocks, int32_t tileMax);
void* zstd_decompress_pipe_general_scratch(void* scratch, int32_t nBlocks, int32_t tileMax);
hipError_t launch_zstd_decompress_prepare(hipStream_t stream, void* generalScratch, const zd::FseTable** dflt);
hipError_t launch_zstd_decompress_list(const BatchArgs& a, hipStream_t stream, void* generalScratch, const int32_t* list, const int32_t* listCount);
int64_t zstd_decompress_general_scratch_bytes();
hipError_t launch_zstd_compress(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int variant);
hipError_t launch_zstd_stream_compress(const BatchArgs& a, hipStream_t stream, void* scratch, int chunked);
int64_t zstd_compress_scratch_bytes(int32_t nBlocks);
// ZstdOutputStream, a step at a time (zstd_stream.hip)
int64_t zstd_ostream_state_bytes();
int64_t zstd_ostream_slab_bytes();
hipError_t launch_zstd_ostream_step(hipStream_t stream, void* state, void* slab, const uint8_t* buf, int32_t offset, int32_t chunk, int32_t closing, uint8_t* out, int32_t outCap);
// ZstdInputStream's frames without a content size, a step at a time (zstd_decompress_pipe.hip)
int64_t zstd_stream_carry_bytes();
void zstd_stream_carry_init(void* hostCarry);
int64_t zstd_stream_step_scratch_bytes(int32_t blocks);
hipError_t launch_zstd_stream_step(hipStream_t stream, void* scratch, int64_t scratchBytes, void* carryDev, const uint8_t* dSrc, int32_t srcLen, int32_t blocks, uint8_t* dOut,
                                   int32_t startPos, int32_t outLimit, int32_t closing, int32_t hasChecksum, uint32_t expected, int32_t* result, const KernelSettings& ks);

// ---- containers: LZ4 frames, x-snappy-framed, Hadoop block streams (the readers pass `ks` on to the two-pass decoders) ----
hipError_t launch_lz4frame_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, int variant, const AuxScratch* aux, const KernelSettings& ks);
int64_t lz4frame_decompress_scratch_bytes(int32_t nItems, int variant);
// acceleration: KernelSettings::lz4Acceleration of the context (1: the kernel as it was)
hipError_t launch_lz4frame_compress(const BatchArgs& a, hipStream_t stream, void* scratch, int64_t scratchBytes, int32_t acceleration = 1);
int64_t lz4frame_compress_scratch_bytes(int32_t items, bool least);
// the block-list writer (lz4_frame_writer.hip): what every LZ4 frame encode takes when lz4f_list_writer(ks) (achip_settings.h) -- frames by ks.lz4f*, blocks at
// ks.lz4Acceleration; it asks bound::lz4frame_list of dstCap, which launch_lz4frame_list_bound works out per item for achip_compress_bound_batch
hipError_t launch_lz4frame_list_compress(const BatchArgs& a, hipStream_t stream, void* scratch, const KernelSettings& ks);
int64_t lz4frame_list_compress_scratch_bytes(int32_t nStreams);
hipError_t launch_lz4frame_list_bound(const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t nBlocks, hipStream_t stream, const KernelSettings& ks);
hipError_t launch_snappyframed_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, int variant, const AuxScratch* aux, const KernelSettings& ks);
int64_t snappyframed_decompress_scratch_bytes(int32_t nStreams);
// ks: the writer's constructor arguments (KernelSettings::snf*; the defaults: the stream as new SnappyFramedOutputStream(compressor, out) writes it); the readers take
// snfVerifyChecksums from the `ks` they have
hipError_t launch_snappyframed_compress(const BatchArgs& a, hipStream_t stream, void* scratch, int variant, const KernelSettings& ks);
int64_t snappyframed_compress_scratch_bytes(int32_t nStreams);
hipError_t launch_hadoop_decompress(const BatchArgs& a, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize, int variant, const AuxScratch* aux, const KernelSettings& ks);
int64_t hadoop_decompress_scratch_bytes(int32_t nStreams, int32_t bufferSize);
hipError_t launch_hadoop_compress(const BatchArgs& a, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize);
int64_t hadoop_compress_scratch_bytes(int32_t nStreams);
// ... and their window forms (WindowArgs, achip_device.h): an item is a piece of a stream that begins at a unit boundary; `w` says per item what was taken and why the call stopped
hipError_t launch_snappyframed_window_decompress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, int variant, const AuxScratch* aux, const KernelSettings& ks);
int64_t snappyframed_window_decompress_scratch_bytes(int32_t nStreams);
hipError_t launch_snappyframed_window_compress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, const KernelSettings& ks);
int64_t snappyframed_window_compress_scratch_bytes(int32_t nStreams);
hipError_t launch_hadoop_window_decompress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize, int variant, const AuxScratch* aux,
                                           const KernelSettings& ks);
int64_t hadoop_window_decompress_scratch_bytes(int32_t nStreams, int32_t bufferSize);
hipError_t launch_hadoop_window_compress(const BatchArgs& a, const WindowArgs& w, hipStream_t stream, void* scratch, bool snappy, int32_t bufferSize);
int64_t hadoop_window_compress_scratch_bytes(int32_t nStreams);

// ---- decoded sizes and the output planner (decoded_size.hip) ----
// A batch to be sized: item i reads srcBase[srcOff[i] .. + srcLen[i]) and reports outSize[i], status[i], errOffset[i]
struct SizeArgs {
    const uint8_t* __restrict__ srcBase;
    const int64_t* __restrict__ srcOff;
    const int32_t* __restrict__ srcLen;
    int64_t* __restrict__ outSize;
    int32_t* __restrict__ status;
    int64_t* __restrict__ errOffset;
    int32_t nBlocks;
    int32_t lz4fLinked = 0;               // ACHIP_OP_LZ4FRAME_DECOMPRESS: KernelSettings::lz4fLinkedBlocks of the context (1: frames of linked blocks are sized, not refused)
    const int32_t* nBlocksDev = nullptr;  // when set: the number of items is this device word (<= nBlocks): the LZ4 blocks a container's streams listed
};
// `op`: one of the seven ACHIP_OP_*_DECOMPRESS (anything else is an error); scratch: decoded_size_scratch_bytes(op, nBlocks) bytes
hipError_t launch_decoded_size(int32_t op, const SizeArgs& s, hipStream_t stream, void* scratch);
int64_t decoded_size_scratch_bytes(int32_t op, int32_t nBlocks);
// align: a power of two; total[0] = bytes of output, total[1] = items left out
hipError_t launch_plan_outputs(const int64_t* outSize, const int32_t* status, int32_t nBlocks, int32_t align, int64_t* dstOff, int32_t* dstCap, int64_t* total, void* scratch,
                               hipStream_t stream);
int64_t plan_outputs_scratch_bytes(int32_t nBlocks);

// ---- compress bounds and the dense copy of a compressed batch (pack_outputs.hip) ----
// `op`: one of the eight ACHIP_OP_*_COMPRESS (achip_compress_bound_batch has refused any other); hadoopBufferSize: the context's, for the two Hadoop ops;
// snfBlockSize: the context's x-snappy-framed block size, for that op
hipError_t launch_compress_bound(int32_t op, const int32_t* srcLen, int64_t* outSize, int32_t* status, int32_t nBlocks, int32_t hadoopBufferSize, hipStream_t stream,
                                 int32_t snfBlockSize);
// The copy's unit of work: this many bytes of destination address.  Chosen by the kernel's shape, not by a sweep: a workgroup of 256 lanes keeps eight 16-byte
// loads per lane in flight (8 x 256 x 16), which amortises the two searches a tile costs and still cuts a 64 KiB-block batch's ~1.5 GiB stream into ~50 000 tiles,
// 25 per workgroup of the grid.  Not tuned on a device (profiles/pack_rate.txt).
constexpr int64_t PACK_TILE_BYTES = 32768;
struct PackArgs {
    const uint8_t* srcBase;  // a compress call's dstBase / dstOff / outLen / status
    const int64_t* srcOff;
    const int32_t* outLen;
    const int32_t* status;
    const uint8_t* rawBase;  // all three null, or the plaintexts: an item whose compressed form is no smaller is taken from here
    const int64_t* rawOff;
    const int32_t* rawLen;
    int32_t nBlocks, align;
    uint8_t* packedBase;  // null: plan only
    int64_t packedCap;
    int64_t* packedOff;
    int32_t* packedLen;
    int32_t* stored;  // null iff the raw arrays are
    int64_t* total;   // [0] bytes of the dense stream, [1] items left out, [2] 1: the bytes were copied
};
// scan (achip_plan.h) and, if packedBase is given, the copy, which reads total[0] on the device and returns at once when the stream does not fit
hipError_t launch_pack_outputs(const PackArgs& p, void* scratch, hipStream_t stream);
int64_t pack_outputs_scratch_bytes(int32_t nBlocks);

// ---- mixed batches, host-pointer staging, hashes (batch_mix.hip, xxhash.hip, xxhash3.hip) ----
hipError_t launch_mix_gather(const int32_t* perm, int32_t n, const BatchArgs& a, int64_t* gSrcOff, int32_t* gSrcLen, int64_t* gDstOff, int32_t* gDstCap, hipStream_t stream);
hipError_t launch_mix_scatter(const int32_t* perm, int32_t n, const int32_t* gOutLen, const int32_t* gStatus, const int64_t* gErr, const BatchArgs& a, hipStream_t stream);
hipError_t launch_blit(void* dst, const void* src, int64_t bytes, int workgroups, hipStream_t stream);
hipError_t launch_xxh64_batch(const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, uint64_t seed, int64_t* out, hipStream_t stream);
hipError_t launch_xxh32_batch(const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, uint32_t seed, int32_t* out, hipStream_t stream);
// XXH3 (xxhash3.hip): out[i] = 64-bit hash, or out[2i], out[2i + 1] = low, high of the 128-bit hash (wide)
hipError_t launch_xxh3_batch(const void* srcBase, const int64_t* srcOff, const int32_t* srcLen, int32_t n, uint64_t seed, bool wide, int64_t* out, hipStream_t stream);

}  // namespace achip
