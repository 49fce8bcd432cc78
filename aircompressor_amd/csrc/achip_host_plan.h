// achip_host_plan.h -- the host side's decisions that are arithmetic: how a host-pointer batch is cut into pipeline chunks and where each array lies in a
// staging slot, the copy tasks over a chunk, the look at a block's first tokens, auto mode's rule on the host, the few-blocks arena, the multi-device partition.
// The units that act on them are abi_host_batch.cpp and abi_dispatch.cpp.  Plain C++17: no HIP, no device (tests/test_host_plan.py compiles it alone).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace achip {
namespace plan __attribute__((visibility("hidden"))) {  // (inline code of the host units: not the library's interface)

// A chunk's slot: [inputs | srcOff dstOff srcLen dstCap | pad | errOffset outLen status | pad | outputs] -- ONE upload (inputs + what the kernels
// read) and ONE download (what they wrote + the outputs) per chunk.
struct HostChunk {
    int64_t first = 0, count = 0;     // range of the processing order
    int32_t op = 0;
    int64_t srcBytes = 0, dstBytes = 0;
    int64_t oSrcOff = 0, oDstOff = 0, oSrcLen = 0, oDstCap = 0, inEnd = 0;  // uploaded: [0, inEnd)
    int64_t oErr = 0, oOutLen = 0, oStatus = 0, oDst = 0, end = 0;          // downloaded: [oErr, end)
    int32_t maxLen = 0;
};

struct ChunkPlan {
    bool negativeLength = false;      // an item's srcLen or dstCap is negative: nothing else is filled in
    std::vector<HostChunk> chunks;
    std::vector<int64_t> sOff, dOff;  // per processed item: offsets inside its chunk's input / output regions
    int64_t maxSlot = 0;              // the staging a slot needs to hold any of the chunks
};

inline int64_t staged(int32_t len) { return ((int64_t)len + 15) & ~15LL; }

// Cuts n items into chunks: homogeneous op, about chunkBytes of staging each, at least one item.  order[j] = caller's item index of the j-th processed item
// (nullptr: identity); ops: per item (mixed) or nullptr (all `op`).
// ramp: the pipeline's first stage has nothing to overlap with and neither has its last (a chunk's upload before the first kernel, the last chunk's download and
// scatter behind everything): the first chunks are smaller -- a quarter, half of chunkBytes -- and so are the last ones (half of what is left,
// down to a quarter).  (round 6: 16 384 blocks of 64 KiB 25 -> ~21 ms per call.)  A batch of at most chunkBytes is not ramped.
inline ChunkPlan cut_chunks(int64_t n, const int32_t* order, const int32_t* ops, int32_t op, const int32_t* srcLen, const int32_t* dstCap, int64_t chunkBytes, bool ramp)
{
    ChunkPlan p;
    auto item = [&](int64_t j) -> int64_t { return order ? order[j] : j; };
    int64_t totalBytes = 0;
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = item(j);
        if (srcLen[i] < 0 || dstCap[i] < 0) {
            p.negativeLength = true;
            return p;
        }
        totalBytes += staged(srcLen[i]) + staged(dstCap[i]);
    }
    p.sOff = std::vector<int64_t>((size_t)n);
    p.dOff = std::vector<int64_t>((size_t)n);
    HostChunk c;
    bool open = false;
    auto close = [&]() {
        int64_t m = (c.srcBytes + 15) & ~15LL;
        c.oSrcOff = m; m += c.count * 8;
        c.oDstOff = m; m += c.count * 8;
        c.oSrcLen = m; m += c.count * 4;
        c.oDstCap = m; m += c.count * 4;
        c.inEnd = m;
        m = (m + 63) & ~63LL;
        c.oErr = m; m += c.count * 8;
        c.oOutLen = m; m += c.count * 4;
        c.oStatus = m; m += c.count * 4;
        m = (m + 63) & ~63LL;
        c.oDst = m;
        c.end = m + c.dstBytes;
        p.maxSlot = std::max(p.maxSlot, c.end + 64);
        p.chunks.push_back(c);
        open = false;
    };
    ramp = ramp && totalBytes > chunkBytes;
    int64_t doneBytes = 0, limit = chunkBytes;
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = item(j);
        const int32_t o = ops ? ops[i] : op;
        const int64_t sb = staged(srcLen[i]), db = staged(dstCap[i]);
        if (open && (o != c.op || c.srcBytes + c.dstBytes + sb + db > limit)) close();
        if (!open) {
            c = HostChunk();
            c.first = j;
            c.op = o;
            open = true;
            if (ramp) {
                const int64_t head = p.chunks.size() == 0 ? chunkBytes / 4 : (p.chunks.size() == 1 ? chunkBytes / 2 : chunkBytes);
                const int64_t tail = std::max(chunkBytes / 4, (totalBytes - doneBytes) / 2);
                limit = std::min(head, tail);
            }
        }
        doneBytes += sb + db;
        p.sOff[(size_t)j] = c.srcBytes;
        p.dOff[(size_t)j] = c.dstBytes;
        c.srcBytes += sb;
        c.dstBytes += db;
        c.count++;
        c.maxLen = std::max(c.maxLen, srcLen[i]);
    }
    if (open) close();
    return p;
}

constexpr int64_t kCopyGrain = 256 << 10;  // bytes per copy task: small blocks are grouped

// The copy tasks over the processed items [first, first + count): consecutive items are grouped up to kCopyGrain bytes (bytesOf(j): what item j copies), task t
// is the items [cut[t], cut[t + 1]).
template <class BytesOf>
inline std::vector<int64_t> copy_cuts(int64_t first, int64_t count, BytesOf bytesOf)
{
    std::vector<int64_t> cut;
    cut.push_back(first);
    int64_t acc = 0;
    for (int64_t j = first; j < first + count; j++) {
        acc += bytesOf(j);
        if (acc >= kCopyGrain) {
            cut.push_back(j + 1);
            acc = 0;
        }
    }
    if (cut.back() != first + count) cut.push_back(first + count);
    return cut;
}

// The mean output bytes per sequence over a block's first 64 sequences (LZ4 tokens: M/lz4/Lz4RawDecompressor.java:59-140; Snappy elements:
// M/snappy/SnappyRawDecompressor.java:84-110), read on the host: 1 = short (below the decoders' auto-mode thresholds: 48 bytes for LZ4, 24 for
// Snappy), 2 = long, 0 = cannot tell.  Bounds-safe on any bytes.
inline int probe_sequences(bool snappy, const uint8_t* p, int64_t n)
{
    int64_t at = 0, out = 0;
    int seqs = 0;
    if (snappy) {
        for (int k = 0; k < 5 && at < n; k++) {  // the uncompressed length (a varint)
            if ((p[at++] & 0x80) == 0) break;
        }
        while (seqs < 64 && at < n) {
            const int tag = p[at++];
            int64_t len;
            if ((tag & 3) == 0) {
                len = (tag >> 2) + 1;
                if (len > 60) {
                    const int extra = (int)len - 60;
                    if (at + extra > n) break;
                    len = 0;
                    for (int b = 0; b < extra; b++) len |= (int64_t)p[at + b] << (8 * b);
                    len += 1;
                    at += extra;
                }
                at += len;
            }
            else {
                len = (tag & 3) == 1 ? ((tag >> 2) & 7) + 4 : (tag >> 2) + 1;
                at += (tag & 3) == 1 ? 1 : ((tag & 3) == 2 ? 2 : 4);
            }
            out += len;
            seqs++;
        }
        return seqs < 8 ? 0 : (out < 24LL * seqs ? 1 : 2);
    }
    while (seqs < 64 && at < n) {
        const int token = p[at++];
        int64_t lit = token >> 4, ml = token & 15;
        if (lit == 15) {
            int v;
            do {
                if (at >= n) return seqs < 8 ? 0 : (out < 48LL * seqs ? 1 : 2);
                v = p[at++];
                lit += v;
            } while (v == 255);
        }
        at += lit + 2;
        if (ml == 15) {
            int v;
            do {
                if (at >= n) return seqs < 8 ? 0 : (out < 48LL * seqs ? 1 : 2);
                v = p[at++];
                ml += v;
            } while (v == 255);
        }
        out += lit + ml + 4;
        seqs++;
    }
    return seqs < 8 ? 0 : (out < 48LL * seqs ? 1 : 2);
}

// The decoder auto mode picks from a call's probe statistics (the first six words) for a batch of `nBlocks` blocks of a codec family whose sequences count as
// short below `shortLimit` (achip_launch.h: BlockCodec): 3 two passes (a mixed or a short-sequence batch), 0 rings.  The rule of lz4_pick (achip_device.h), on the host.
inline int auto_pick(const int32_t* v, int32_t nBlocks, int32_t shortLimit)
{
    const bool mixed = (int64_t)v[0] * 4 > (nBlocks + 15) / 16;
    const bool pooledShort = v[1] > 0 && (int64_t)v[2] < shortLimit * (int64_t)v[1];
    const bool isShort = v[5] > 0 ? (int64_t)v[4] * 3 > (int64_t)v[5] : pooledShort;
    return (mixed || isShort) ? 3 : 0;
}

// Record bytes per block for the few-blocks route (a batch below the size auto mode probes from, its block sizes known on the device only): such blocks may be whole
// files -- a 4 MiB text block makes 6 MiB of records where the block codec's 64 KiB blocks make 96 KiB --, so the arena is sized as a whole: a GiB over however few
// blocks there are (as ever at most half of what the device has free; blocks that still do not fit go to the ring decoder, now at 64 lanes each).
inline int64_t few_blocks_record_bytes(int32_t nBlocks, int64_t perBlock)
{
    if (nBlocks >= 4096 || nBlocks <= 0) return perBlock;
    return std::max<int64_t>(perBlock, ((1LL << 30) / nBlocks) & ~4095LL);
}

// nParts contiguous slices of nBlocks items balanced by weight (nullptr: one each; negative weights count as 0): starts[p] is the smallest index whose prefix
// weight reaches p / nParts of the total, starts[nParts] = nBlocks.
inline void partition_blocks(const int64_t* weight, int32_t nBlocks, int32_t nParts, int32_t* starts)
{
    int64_t total = 0;
    for (int32_t i = 0; i < nBlocks; i++) {
        total += weight ? std::max<int64_t>(weight[i], 0) : 1;
    }
    starts[0] = 0;
    int64_t acc = 0;
    int32_t idx = 0;
    for (int32_t p = 1; p < nParts; p++) {
        const __int128 target = (__int128)total * p;
        while (idx < nBlocks && (__int128)acc * nParts < target) {
            acc += weight ? std::max<int64_t>(weight[idx], 0) : 1;
            idx++;
        }
        starts[p] = idx;
    }
    starts[nParts] = nBlocks;
}

}  // namespace plan
}  // namespace achip
