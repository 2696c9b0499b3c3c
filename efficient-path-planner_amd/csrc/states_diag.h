// states_diag.h — the diagnostics build of k_states_v5 (-DEPP_STATES_TL;
// scripts/states_timeline.py): a per-wave timeline.  Lane 0 stamps s_memrealtime (100 MHz) at
// entry, after the staging barrier, when the first group's state data have arrived (right
// behind an explicit vmcnt(0) wait: single-pass instantiations only, a prefetching one would
// drain its next group there and leaves the stamp 0), after that group's classification, after
// its exact path, at the end; plus HW_ID.  Eight words per wave: stamps 0-5, HW_ID | counts,
// spare.  In the product build EPP_STL expands to nothing.  The storage (g_states_tl) and the
// epp_dbg_states_tl export are in states_v5.hip, with the kernel that stamps.
#pragma once

#ifdef EPP_STATES_TL
namespace epp {
constexpr int kTlWaves = 1 << 16;
constexpr int kTlWords = 8;
}  // namespace epp
// stamp k of this wave (BLOCK: the kernel's workgroup size)
#define EPP_STL(k)                                                                                  \
    do {                                                                                            \
        const int w_ = (int)((blockIdx.x * BLOCK + threadIdx.x) >> 6);                             \
        const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                             \
        if ((threadIdx.x & 63) == 0 && w_ < kTlWaves) g_states_tl[w_][k] = t_;                      \
    } while (0)
#else
#define EPP_STL(k) \
    do {           \
    } while (0)
#endif
