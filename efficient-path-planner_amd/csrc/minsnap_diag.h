// minsnap_diag.h — the diagnostics build of the fused refit (-DEPP_REFIT_TL;
// scripts/refit_timeline.py): a phase timeline of solve_track (minsnap_solve.h) and
// refit_body (minsnap_refit.hip).  Thread 0 of each workgroup stamps s_memrealtime
// (100 MHz) at the phases' ends, and the shader clock around the block solve and in its
// loops.  In the product build the three macros expand to nothing.  The storage is per
// translation unit, as the solve's constants are; the epp_dbg_refit_tl export is in
// minsnap_refit.hip, with the kernels whose stamps it reads.
#pragma once

#ifdef EPP_REFIT_TL
namespace epp {
namespace {
__device__ unsigned long long g_refit_tl[2][16];
// (per-iteration shader clocks of the block solve's forward / backward loops)
__device__ unsigned long long g_refit_it[2][64];
}  // namespace
}  // namespace epp
#define EPP_TL(k)                                                                         \
    do {                                                                                  \
        if (threadIdx.x == 0) g_refit_tl[blockIdx.x & 1][k] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define EPP_TLI(k)                                                                           \
    do {                                                                                     \
        if (threadIdx.x == 0 && (k) < 64) g_refit_it[blockIdx.x & 1][k] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// (slots 14, 15: the shader clock, s_memtime, around the block solve)
#define EPP_TLC(k)                                                                        \
    do {                                                                                  \
        if (threadIdx.x == 0) g_refit_tl[blockIdx.x & 1][k] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define EPP_TLC(k) \
    do {           \
    } while (0)
#define EPP_TLI(k) \
    do {           \
    } while (0)
#define EPP_TL(k) \
    do {          \
    } while (0)
#endif
