// tools/hostemu/emu_zstd.cpp -- the Zstd decode pipeline (zstd_decompress_pipe.hip: parse / literals / sequences / execute / checksum, and
// the multi-block stages) under the fiber emulator.  The sequence stage gives an item to a quad of lanes: its DPP broadcasts and LDS
// hand-overs are quad-level rendezvous here (hip/hip_runtime.h).  The one-kernel decoder that takes the pipeline's fallback list moves
// bytes between lanes in hardware order and is NOT emulated: items on the fallback list are reported to the caller instead.
// The ring executor (zstd_pipe_execute_kernel: four lanes an item over achip_rings.h) needs the rings' group rendezvous, as tools/hostemu/emu.cpp has them.
#define HOSTEMU_RINGS_LOCKSTEP 1  // achip_rings.h: the lanes of a group meet where the device's lockstep makes them meet
#include "emu_preamble.h"
#include "../../aircompressor_amd/csrc/zstd_decompress_pipe.hip"
#include "../../aircompressor_amd/csrc/zstd_default_tables.h"
#include "../../aircompressor_amd/csrc/achip_zstd_frame.h"
#include <vector>
namespace achip {
namespace {
std::vector<int32_t> g_fallback;
}  // namespace
hipError_t launch_zstd_decompress_prepare(hipStream_t, void* generalScratch, const zd::FseTable** dflt)
{
    zd::FseTable* t = (zd::FseTable*)((uint8_t*)generalScratch + 4096);
    hipLaunchKernelGGL(zstd_default_tables_kernel, dim3(1), dim3(64), 0, nullptr, t);  // (the product's own build)
    *dflt = t;
    return hipSuccess;
}
hipError_t launch_zstd_decompress_list(const BatchArgs&, hipStream_t, void*, const int32_t* list, const int32_t* listCount)
{
    g_fallback.assign(list, list + *listCount);
    return hipSuccess;
}
int64_t zstd_decompress_general_scratch_bytes() { return 4096 + (int64_t)sizeof(zd::FseTable) * 3 + 4096; }
}  // namespace achip

// runs the pipeline over the batch; items it handed to the fallback list get status -1000 and are listed in fallback[0 .. return value)
namespace {
std::vector<uint8_t> g_mbScratch;
int64_t g_mbMaxBytes = 0;  // > 0: larger requests are refused (the stages then ask for less)
void* emu_mb_get(void*, int64_t bytes)
{
    if (g_mbMaxBytes > 0 && bytes > g_mbMaxBytes) {
        return nullptr;
    }
    g_mbScratch.assign((size_t)bytes, 0xCD);
    return g_mbScratch.data();
}
}  // namespace

// a stream decoded a step at a time (launch_zstd_stream_step): the caller (check_zstd.py --stream) plays the host's part -- the stand-in frame header, the
// history -- with the product's own walk over frame header and block headers (achip_zstd_frame.h, as abi_zstd_stream.cpp calls it)
// out: state detail offset headerSize hasChecksum lookBack windowBeyondJava (the look-back for a reader that keeps at most 128 MiB, as the product's does)
extern "C" void emu_zstd_read_frame_header(const uint8_t* p, int64_t have, int64_t* out)
{
    const achip::zframe::FrameHeader h = achip::zframe::read_frame_header(p, have);
    const achip::zframe::FrameWindow w = achip::zframe::frame_window(h, 128LL << 20);
    const int64_t v[7] = {h.state, h.detail, h.offset, h.headerSize, h.hasChecksum, w.lookBack, w.windowBeyondJava};
    memcpy(out, v, sizeof(v));
}
// blocks: header dataPos dataLen streamBytes per listed block; info: bytes closing expected broken; returns the number of blocks
extern "C" int emu_zstd_list_step(const uint8_t* p, int64_t have, int32_t hasChecksum, int32_t windowBeyondJava, int32_t maxBlocks, int64_t* blocks, int64_t* info)
{
    const achip::zframe::Step s = achip::zframe::list_step(p, have, hasChecksum != 0, windowBeyondJava != 0, maxBlocks);
    for (size_t i = 0; i < s.blocks.size(); i++) {
        const achip::zframe::StepBlock& b = s.blocks[i];
        const int64_t v[4] = {b.header, (int64_t)b.dataPos, b.dataLen, b.streamBytes};
        memcpy(blocks + 4 * i, v, sizeof(v));
    }
    const int64_t v[4] = {s.bytes, s.closing, s.expected, s.broken};
    memcpy(info, v, sizeof(v));
    return (int)s.blocks.size();
}
extern "C" int64_t emu_zstd_stream_carry_bytes() { return achip::zstd_stream_carry_bytes(); }
extern "C" void emu_zstd_stream_carry_init(void* carry) { achip::zstd_stream_carry_init(carry); }
extern "C" int emu_zstd_stream_step(void* carry, const uint8_t* src, int32_t srcLen, int32_t blocks, uint8_t* out, int32_t startPos, int32_t outLimit, int32_t closing,
                                    int32_t hasChecksum, uint32_t expected, int32_t* result)
{
    static std::vector<uint8_t> scratch;
    const int64_t bytes = achip::zstd_stream_step_scratch_bytes(blocks);
    scratch.assign((size_t)bytes, 0xCD);
    return (int)achip::launch_zstd_stream_step(nullptr, scratch.data(), bytes, carry, src, srcLen, blocks, out, startPos, outLimit, closing, hasChecksum, expected, result, achip::KernelSettings());
}

// passBlocks: blocks per pass of the multi-block stages (0: multi-block frames go to the fallback list); counters: the pipeline's 64 counter words
extern "C" int emu_zstd_pipe(const uint8_t* srcBase, const int64_t* srcOff, const int32_t* srcLen, uint8_t* dstBase, const int64_t* dstOff, const int32_t* dstCap,
                             int32_t* outLen, int32_t* status, int64_t* errOffset, int32_t n, int32_t tile, int32_t execMode, int32_t* fallback, int32_t passBlocks,
                             int32_t* counters, int64_t mbMaxBytes)
{
    g_mbMaxBytes = mbMaxBytes;
    // (execMode bit 8: the product's default decompress.ring_pad of 80 -- the ring executor then stages far matches in LDS; otherwise 16: no staging area)
    achip::BatchArgs a{srcBase, srcOff, srcLen, dstBase, dstOff, dstCap, outLen, status, errOffset, n, (execMode >> 8) & 1 ? 80 : 16};
    static std::vector<uint8_t> scratch;
    const int64_t bytes = achip::zstd_decompress_pipe_scratch_bytes(n, tile);
    scratch.assign((size_t)bytes, 0xCD);
    achip::KernelSettings ks;
    ks.zstdExec = execMode & 3;
    ks.zstdSeqWaves = (execMode >> 4) & 7 ? (execMode >> 4) & 7 : 1;  // (bits 4 .. 6: wavefronts per workgroup of the sequence stage, with full workgroups)
    ks.zstdSeqSpread = (execMode >> 4) & 7 ? 1 : 256;
    ks.zstdLitItems = ((execMode >> 2) & 3) == 1 ? 8 : (((execMode >> 2) & 3) == 2 ? 10 : (((execMode >> 2) & 3) == 3 ? 13 : 16));  // (bits 2, 3: items per wavefront of the literal stage; 13: the split table layout)
    if ((execMode >> 7) & 1) ks.zstdLitItems = 20;  // (bit 7: 16 items, symbols and lengths by symbol)
    achip::g_fallback.clear();
    for (int32_t i = 0; i < n; i++) {
        status[i] = -999;  // "not written"
    }
    achip::ZstdMbProvider mbp{emu_mb_get, nullptr, passBlocks};
    achip::launch_zstd_decompress_pipe(a, nullptr, scratch.data(), achip::zstd_decompress_pipe_general_scratch(scratch.data(), n, tile), tile, passBlocks > 0 ? &mbp : nullptr, ks);
    memcpy(counters, scratch.data(), 256);
    for (size_t k = 0; k < achip::g_fallback.size(); k++) {
        fallback[k] = achip::g_fallback[k];
        status[achip::g_fallback[k]] = -1000;
    }
    return (int)achip::g_fallback.size();
}
