// zstd_default_tables.h -- the kernel that builds Zstd's three predefined FSE tables, for every unit that decodes sequence sections: the one-kernel decoder
// and the pipeline (zstd_decompress.hip launches it for both), the size query (decoded_size.hip), the emulator (tools/hostemu/emu_zstd.cpp).
#pragma once
#include "zstd_dec_common.h"

namespace achip {

// the three predefined tables (literal lengths, offsets, match lengths) built by one wavefront into global memory, once per launch: for every unit that
// decodes sequence sections (each launches it on its own scratch)
static __global__ __launch_bounds__(64) void zstd_default_tables_kernel(zd::FseTable* dflt)
{
    using namespace zd;
    __shared__ TableShared sh;
    Ctx c = reader_ctx(nullptr, 0, threadIdx.x);
    const int16_t* norms[3] = {LL_DEFAULT_NORM, OF_DEFAULT_NORM, ML_DEFAULT_NORM};
    const int32_t maxSym[3] = {35, 28, 52};
    const int32_t logs[3] = {6, 5, 6};
    for (int k = 0; k < 3; k++) {
        __syncthreads();
        for (int i = c.lane; i <= maxSym[k]; i += 64) {
            sh.norm[i] = norms[k][i];
        }
        __syncthreads();
        fse_build(c, sh, sh.fse[k], maxSym[k], logs[k], 0);
        __syncthreads();
        for (int i = c.lane; i < 512; i += 64) {
            dflt[k].e[i] = sh.fse[k].e[i];
        }
    }
}
}  // namespace achip
