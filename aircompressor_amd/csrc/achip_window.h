// achip_window.h -- what the windowed calls over the chunked containers (achip_window_*: hadoop_streams.hip, snappy_frame.hip) share beside WindowArgs
// (achip_device.h): the one place a window's verdict is written, and the kernel behind a window writer.  A window is a piece of one stream that begins at a unit
// boundary (a Hadoop block or zero length word, an x-snappy-framed chunk); the caller keeps the stream position, the kernels keep nothing.
#pragma once
#include "achip_device.h"

namespace achip {

namespace win {
// what a walk leaves for its fold beside the public stop codes
constexpr int32_t STOP_SERIAL = -1;  // the wavefront-per-stream kernel goes on from here: a unit of another shape, or one whose verdict needs its bytes decoded

__device__ __forceinline__ void report(const BatchArgs& a, const WindowArgs& w, int32_t i, int64_t consumed, int32_t produced, int32_t stop, int64_t need, int32_t status, int64_t eo)
{
    a.outLen[i] = produced;
    a.status[i] = status;
    a.errOffset[i] = status == 0 ? 0 : eo;
    w.consumed[i] = consumed;
    w.stop[i] = status != 0 ? ACHIP_STOP_FAILED : stop;
    w.need[i] = status != 0 ? 0 : need;
}

// behind a window writer's kernels: a window whose writer reported a status took nothing
static __global__ void writer_verdict_kernel(BatchArgs a, WindowArgs w)
{
    const int32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < a.nBlocks && a.status[i] != 0) {
        w.consumed[i] = 0;
        w.stop[i] = ACHIP_STOP_FAILED;
        w.need[i] = 0;
    }
}
}  // namespace win

}  // namespace achip
