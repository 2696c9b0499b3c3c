// motions_diag.h — the diagnostics build of the motion kernels (-DEPP_MOTIONS_TL;
// scripts/motions_timeline.py): a per-wave time split in shader-clock cycles, six counters a
// wave (k_motions_v4: level-1/2 walk, flushes, total, list entries, queued pairs, cell pairs;
// k_motions_v5: filter + queue, flushes, total, candidate loop, queued pairs, staging).  In the
// product build every macro here expands to nothing.  A __device__ symbol cannot be shared
// between translation units, so each kernel file that stamps a timeline places
// EPP_MTL_STORAGE(its export) at global scope, ahead of its kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "epp_internal.h"

#ifdef EPP_MOTIONS_TL
namespace epp {
constexpr int kMtlWaves = 1 << 16;
}
// the file's timeline and the export that reads out the last launch's first `waves` records
#define EPP_MTL_STORAGE(export_name)                                                                          \
    namespace epp {                                                                                           \
    namespace {                                                                                               \
    __device__ unsigned long long g_motions_tl[kMtlWaves][6];                                                 \
    }                                                                                                         \
    }                                                                                                         \
    extern "C" epp_status export_name(unsigned long long* out, int64_t waves) {                               \
        return hipMemcpyFromSymbol(out, HIP_SYMBOL(epp::g_motions_tl),                                        \
                                   (size_t)std::min<int64_t>(waves, epp::kMtlWaves) * 48) == hipSuccess       \
                   ? EPP_OK                                                                                   \
                   : EPP_ERR_HIP;                                                                             \
    }
#define EPP_MTL_DECL unsigned long long tl_walk = 0, tl_flush = 0, tl_t0 = __builtin_readcyclecounter(), tl_e = 0, tl_q = 0, tl_c = 0
#define EPP_MTL_ADD(v, t) v += __builtin_readcyclecounter() - (t)
#define EPP_MTL_NOW(t) const unsigned long long t = __builtin_readcyclecounter()
#define EPP_MTL_CNT(v, x) v += (x)
#define EPP_MTL_SINCE_START(v) v = __builtin_readcyclecounter() - tl_t0
// the wave's record (block: the workgroup size; lane: the caller's lane id)
#define EPP_MTL_END(block, lane)                                                                      \
    do {                                                                                              \
        const int w_ = (int)((blockIdx.x * (block) + threadIdx.x) >> 6);                              \
        if ((lane) == 0 && w_ < kMtlWaves) {                                                          \
            g_motions_tl[w_][0] = tl_walk; g_motions_tl[w_][1] = tl_flush;                            \
            g_motions_tl[w_][2] = __builtin_readcyclecounter() - tl_t0; g_motions_tl[w_][3] = tl_e;   \
            g_motions_tl[w_][4] = tl_q; g_motions_tl[w_][5] = tl_c;                                   \
        }                                                                                             \
    } while (0)
#else
#define EPP_MTL_STORAGE(export_name)
#define EPP_MTL_DECL
#define EPP_MTL_ADD(v, t)
#define EPP_MTL_NOW(t)
#define EPP_MTL_CNT(v, x)
#define EPP_MTL_SINCE_START(v)
#define EPP_MTL_END(block, lane)
#endif
