// crc32c_diag.h -- the two timing diagnostics of crc32c_kernels.hip (included
// by it alone): wall-clock stamps of k_fold's waves and of k_plan_map's
// blocks, and the readers the trace tools call.  Both are 0 in the product,
// where the stamps compile to nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "bmqcrc_internal.h"

#ifndef BMQCRC_FOLD_DIAG
#define BMQCRC_FOLD_DIAG 0  // 1: per-wave wall-clock stamps of the last k_fold launch
                            // (tools/fold_trace_diag.py)
#endif
#ifndef BMQCRC_PLAN_DIAG
#define BMQCRC_PLAN_DIAG 0  // 3: per-block phase stamps of the last k_plan_map launch
                            // (tools/plan_trace_diag.py)
#endif

#if BMQCRC_FOLD_DIAG
namespace bmqcrc {
// per wave (entry, prologue done, first loads issued, first group folded, last
// group's lines folded, loop done, end), read by bmqcrc_diag_fold_trace
constexpr int kFoldTraceWaves = 4096;
__device__ unsigned long long g_fold_trace[kFoldTraceWaves][8];
}  // namespace bmqcrc
// (k_fold: lane, and g0 = the wave's index in the grid)
#define FOLD_STAMP(k)                                                              \
    if (lane == 0 && g0 < (uint32_t)kFoldTraceWaves) {                             \
        g_fold_trace[g0][k] = wall_clock64();                                      \
    }
extern "C" __attribute__((visibility("default"))) int bmqcrc_diag_fold_trace(unsigned long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bmqcrc::g_fold_trace),
                               sizeof(bmqcrc::g_fold_trace)) == hipSuccess
               ? 0
               : -5;
}
#else
#define FOLD_STAMP(k)
#endif

#if BMQCRC_PLAN_DIAG
namespace bmqcrc {
// per block (start, first loads landed, first tile counted, phase 1 done, wait
// done, deferred writes issued, class bases done, end), read by
// bmqcrc_diag_plan_trace
__device__ unsigned long long g_plan_trace[kPlanMaxBlocks][8];
}  // namespace bmqcrc
#define PLAN_STAMP(k)                                                        \
    if (threadIdx.x == 0) {                                                  \
        g_plan_trace[blockIdx.x][k] = wall_clock64();                        \
    }
#define PLAN_STAMP_LANDED(k)                                                 \
    if (threadIdx.x == 0) {                                                  \
        __builtin_amdgcn_s_waitcnt(0);                                       \
        g_plan_trace[blockIdx.x][k] = wall_clock64();                        \
    }
extern "C" __attribute__((visibility("default"))) int bmqcrc_diag_plan_trace(unsigned long long* out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(bmqcrc::g_plan_trace),
                               sizeof(bmqcrc::g_plan_trace)) == hipSuccess
               ? 0
               : -5;
}
#else
#define PLAN_STAMP(k)
#define PLAN_STAMP_LANDED(k)
#endif
