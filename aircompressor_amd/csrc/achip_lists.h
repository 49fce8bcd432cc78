// achip_lists.h -- what the container units (lz4_frame.hip, snappy_frame.hip, hadoop_streams.hip) share around their format-specific kernels:
// the carver that lays a unit's lists out in its scratch, the batch a reader assembles on the device for the block decoders, the list a
// writer plans its blocks into, and the kernel that seals either.  A list is filled by one lane per stream (`atomicAdd(counters, n)`
// reserves n entries), sealed (`counters[1] = min(counters[0], CAPACITY)`) and from then on read as `counters[1]` entries.
#pragma once
#include <stdint.h>

namespace achip {

struct BatchArgs;

namespace lists {

constexpr int32_t CAPACITY = 1 << 20;  // entries of a list; a stream whose entries do not fit takes its unit's other way
constexpr int64_t COUNTER_WORDS = 1024;  // a list's counters lead the scratch: one 4 KiB page, cleared by the launcher

// Lays arrays out one behind the other, each aligned to 16 bytes.  Over a null base it only MEASURES: take() returns null and used() is what
// the same calls need over a real one.  A unit carves each list in ONE function, called by its launcher (assign) and by its *_scratch_bytes
// (measure), so the size a context allocates is the size the kernels touch.
struct Carver {
    uint8_t* base;
    int64_t offset = 0;
    explicit Carver(void* scratch) : base((uint8_t*)scratch) {}
    template <class T>
    T* take(int64_t count)
    {
        constexpr int64_t ALIGN = alignof(T) > 16 ? (int64_t)alignof(T) : 16;
        offset = (offset + ALIGN - 1) & ~(ALIGN - 1);
        T* r = base != nullptr ? (T*)(base + offset) : nullptr;
        offset += count * (int64_t)sizeof(T);
        return r;
    }
    int64_t used() const { return offset; }
};

// A reader's device-assembled batch: one entry per chunk / block of the streams, in the shape the block decoders take (as_batch).
struct ChunkBatch {
    int64_t* cSrcOff;
    int32_t* cSrcLen;
    int64_t* cDstOff;
    int32_t* cDstCap;
    int32_t* cOutLen;
    int32_t* cStatus;
    int64_t* cErrOff;
    int32_t* counters;  // [0] entries allocated, [1] entries in the batch (sealed); the words behind them are the owner's
    void carve(Carver& k, int32_t* counterWords)
    {
        counters = counterWords;
        cSrcOff = k.take<int64_t>(CAPACITY);
        cDstOff = k.take<int64_t>(CAPACITY);
        cErrOff = k.take<int64_t>(CAPACITY);
        cSrcLen = k.take<int32_t>(CAPACITY);
        cDstCap = k.take<int32_t>(CAPACITY);
        cOutLen = k.take<int32_t>(CAPACITY);
        cStatus = k.take<int32_t>(CAPACITY);
    }
    // the entries as a batch whose size is known on the device only (launches are sized for `capacity`); every other field is the caller's
    BatchArgs as_batch(const BatchArgs& a, int32_t capacity) const;
};

// The Hadoop and x-snappy-framed writers' list: a stream's blocks, encoded at worst-case places by wavefronts that draw entries, then compacted.
struct WriterList {
    int32_t* sFirst;    // per stream
    int32_t* sCount;
    int32_t* sStatus;
    int32_t* sSerial;   // 1: the stream's entries did not fit, another kernel writes it (null where a unit has no such kernel)
    int32_t* bStream;   // per entry; -1: a hole (its stream did not fit)
    int32_t* bIndex;
    int32_t* bSize;     // bytes written at the worst-case place
    int32_t* counters;  // [0] entries allocated, at most the capacity, [1] entries in the list (sealed), [2] encode cursor, [3] compact cursor, [4, 5] the plan's 64-bit cursor
    void carve(Carver& k, int32_t* counterWords, int64_t nStreams, bool serialRoute)
    {
        counters = counterWords;
        sFirst = k.take<int32_t>(nStreams);
        sCount = k.take<int32_t>(nStreams);
        sStatus = k.take<int32_t>(nStreams);
        sSerial = serialRoute ? k.take<int32_t>(nStreams) : nullptr;
        bStream = k.take<int32_t>(CAPACITY);
        bIndex = k.take<int32_t>(CAPACITY);
        bSize = k.take<int32_t>(CAPACITY);
    }
};

}  // namespace lists
}  // namespace achip

#ifndef ACHIP_LISTS_LAYOUT_ONLY  // (the layout above needs no HIP: tests/test_lists.py compiles it with the host's C++ compiler)
#include "achip_device.h"

namespace achip {
namespace lists {

inline BatchArgs ChunkBatch::as_batch(const BatchArgs& a, int32_t capacity) const
{
    BatchArgs c = a;
    c.srcOff = cSrcOff;
    c.srcLen = cSrcLen;
    c.dstOff = cDstOff;
    c.dstCap = cDstCap;
    c.outLen = cOutLen;
    c.status = cStatus;
    c.errOffset = cErrOff;
    c.nBlocks = capacity;
    c.nBlocksDev = counters + 1;
    c.only = nullptr;
    c.onlyStats = nullptr;
    return c;
}

// A writer's plan, the part every stream shares: reserve `n` entries for `stream` and fill them in.  Returns whether they fit; what becomes of
// a stream that does not (an error, another kernel) is the caller's.  `capacity`: the entries the launcher seals the list at (<= CAPACITY).
// The reservation cannot wrap, whatever the batch: a stream with more entries than the whole list reserves nothing (with a block size of 1 one stream may
// bring 2^27 blocks), so every addition is at most `capacity` <= 2^20, and the cursor the additions go to is the 64-bit word at counters[4, 5] -- fewer than
// 2^31 streams of at most 2^20 entries stay below 2^51.  counters[0], which seal_kernel reads, is kept as min(reserved, capacity) by an atomicMax: no index
// below is ever negative or beyond `capacity`.
__device__ __forceinline__ bool plan_entries(const WriterList& L, int32_t stream, int32_t n, int32_t capacity = CAPACITY)
{
    if (n > capacity) {
        L.sFirst[stream] = 0;
        L.sCount[stream] = 0;
        return false;
    }
    const int64_t first = n > 0 ? (int64_t)atomicAdd((unsigned long long*)(L.counters + 4), (unsigned long long)n) : 0;
    const bool fits = first + n <= capacity;
    if (n > 0 && first < capacity) {
        atomicMax(L.counters, fits ? (int32_t)(first + n) : capacity);
    }
    L.sFirst[stream] = fits ? (int32_t)first : 0;
    L.sCount[stream] = fits ? n : 0;
    for (int64_t k = 0; k < n && first + k < capacity; k++) {
        L.bStream[first + k] = fits ? stream : -1;
        L.bIndex[first + k] = (int32_t)k;
    }
    return fits;
}

// the list holds the entries that fit: a stream that does not fit leaves a hole of entries nobody reads
static __global__ void seal_kernel(int32_t* counters, int32_t capacity)
{
    const int32_t allocated = counters[0];
    counters[1] = allocated < capacity ? allocated : capacity;
}

}  // namespace lists
}  // namespace achip
#endif
