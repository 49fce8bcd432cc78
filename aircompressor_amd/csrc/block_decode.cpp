// block_decode.cpp -- the LZ4 / Snappy block decoders as one table, and the decode path of a batch a container reader listed on the device.
#include "achip_launch.h"

namespace achip {

#if !defined(__HIP_DEVICE_COMPILE__)  // (a table of host functions: the device pass of this unit, which has no kernel, must not emit it)
const BlockCodec kBlockCodecs[2] = {
    {launch_lz4_decompress_rings, launch_lz4_decompress_twopass, launch_lz4_sequence_sample, lz4_ring_group_for, LZ4_RECORD_BYTES_PER_BLOCK, LZ4_RECORD_BYTES_PER_BLOCK_MIN, 12},
    {launch_snappy_decompress_rings, launch_snappy_decompress_twopass, launch_snappy_element_sample, snappy_ring_group_for, SNAPPY_RECORD_BYTES_PER_BLOCK,
     SNAPPY_RECORD_BYTES_PER_BLOCK_MIN, 6},
};
#endif

// The contract (what the three readers did each on its own until they shared this):
//   !want.sync   no synchronisation.  The device count picks among launches sized for the capacity: Snappy 4 lanes per chunk (16 measured slower:
//                390 against 481 GiB/s); LZ4 two launches, 4 lanes per chunk from 32 768 chunks on and 16 below (721 -> 814 GiB/s fragments, 56 -> 83
//                corpus at 16 384 chunks: a stream's chunks are up to 256 KiB, a few thousand of them at 4 lanes each leave most of the chip idle).
//   want.sync    want.probe: the family's length probe runs on the list BEFORE the one synchronisation, which brings home the count and the probe's
//                words.  Then the two passes if !want.probe or the POOLED rule says short -- only the sampled lengths count here: a stream's last chunk
//                is a short one, so "compressed sizes within a 16-chunk group differ by 2x", the block API's sign of a mixed batch, holds for every
//                group of a batch of streams -- on an arena asked from `aux`; blocks whose records do not fit go to the rings at 16 (LZ4) / 4 (Snappy)
//                lanes.  Long sequences, or no arena and want.ringsWithoutArena: the rings at the lanes per block that fit the count, one launch of
//                that size, no probes.  Measured, 1024 streams x 4 MiB, fragments / corpus GiB/s (profiles/r03_notes.md): Hadoop LZ4 rings 818 / 83,
//                two passes 271 / 158; Hadoop Snappy 474 / 39 against 230 / 107; framed 804 / 116 against 456 / 236.
//   A count of 0 launches nothing.
hipError_t launch_listed_decode(const BatchArgs& listed, int fam, hipStream_t stream, const int32_t* counters, int32_t* stats, const AuxScratch* aux, const KernelSettings& ks,
                                const ListedWant& want, bool* decoded)
{
    const BlockCodec& c = kBlockCodecs[fam];
    *decoded = true;
    if (!want.sync) {
        if (fam == 1) {
            return c.rings(listed, stream, 4, 0, nullptr);
        }
        BatchArgs big = listed, small = listed;
        big.countLo = 32768;
        small.countHi = 32768;
        const hipError_t e = c.rings(big, stream, 4, 0, nullptr);
        return e != hipSuccess ? e : c.rings(small, stream, 16, 0, nullptr);
    }
    hipError_t e = want.probe ? c.sample(listed, stream, stats, 0, 0) : hipSuccess;
    if (e != hipSuccess) return e;
    int32_t head[64] = {0};
    const int32_t* v = head + (stats - counters);
    e = hipMemcpyAsync(head, counters, (size_t)(v + 4 - head) * sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    BatchArgs t = listed;
    t.nBlocks = head[1];
    t.nBlocksDev = nullptr;
    *decoded = false;
    if (t.nBlocks <= 0) {
        return hipSuccess;
    }
    if (!want.probe || (v[1] > 0 && (int64_t)v[2] < c.shortLimit * (int64_t)v[1])) {
        int64_t perBlock = c.recordBytes * want.recordScale;
        if (want.roomWord >= 0) {  // records by the blocks' room: 3/2 of it, as the family's 96 KiB of arena per 64 KiB of output
            long long room = 0;
            __builtin_memcpy(&room, head + want.roomWord, 8);
            const int64_t byRoom = ((room + t.nBlocks - 1) / t.nBlocks * 3 / 2 + 4095) & ~4095LL;
            perBlock = perBlock < byRoom ? byRoom : perBlock;
        }
        const int64_t bytes = twopass_scratch_bytes(t.nBlocks, perBlock);
        void* arena = aux != nullptr && aux->get != nullptr ? aux->get(aux->user, bytes) : nullptr;
        if (arena != nullptr) {
            *decoded = true;
            return c.twopass(t, stream, arena, bytes, fam == 0 ? 16 : 4, 0, nullptr, ks);
        }
        if (!want.ringsWithoutArena) {
            return hipSuccess;
        }
    }
    *decoded = true;
    return c.rings(t, stream, c.groupFor(t.nBlocks), 0, nullptr);
}

}  // namespace achip
