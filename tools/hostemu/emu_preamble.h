// tools/hostemu/emu_preamble.h -- what opens every emulator unit, behind the HOSTEMU_* defines with which the unit picks its order-point model: the shim, the
// launch coordinates the shim declares, the development counters, and the guarded scratch of the units that hand a kernel one.
#pragma once
#include "hip/hip_runtime.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
extern "C" { long long achip_emu_counters[16]; }  // development counters of kernels under emulation (ACHIP_EMU_COUNT)
// A scratch of exactly the size a *_scratch_bytes function names, filled with 0xCD, and a guard tail behind it: a kernel that writes beyond the
// named size changes the tail, and check() ends the process (loud in every caller, whatever it does with a return value).
struct GuardedScratch {
    static constexpr size_t TAIL = 4096;
    std::vector<uint8_t> v;
    uint8_t* assign(int64_t bytes)
    {
        v.assign((size_t)bytes + TAIL, 0xCD);
        return v.data();
    }
    int64_t size() const { return (int64_t)(v.size() - TAIL); }
    int check(const char* what, int r) const
    {
        for (size_t i = v.size() - TAIL; i < v.size(); i++) {
            if (v[i] != 0xCD) {
                fprintf(stderr, "hostemu: %s wrote %zu bytes beyond its scratch of %lld bytes\n", what, i - (v.size() - TAIL), (long long)size());
                abort();
            }
        }
        return r;
    }
};
