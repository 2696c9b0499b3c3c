// knn_diag.h — the diagnostics build of the grid k-NN (-DEPP_KNN_DIAG; scripts/knn_timeline.py):
// per-block phase timeline of k_knn_tile, per-query timeline of k_knn_retry, device asserts of
// k_knn_tile's invariants, and the EPP_KNN_NPC grid-density knob.  In the product build every
// macro here expands to nothing.  The storage and the epp_dbg_knn_* exports are in knn_retry.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdlib>

#include "knn_kernels.h"

#ifdef EPP_KNN_DIAG
namespace epp {
constexpr int kKnnTlBlocks = 65536;  // timeline records (16 u64 per block)
constexpr int kKnnRetryTl = 4096;    // retried queries recorded (k_knn_retry)
// the zeroed timeline buffer for a k_knn_tile launch on s (its last argument)
unsigned long long* knn_tl_begin(hipStream_t s);
// EPP_KNN_NPC: the grid density, an exact-either-way A/B knob
inline double knn_nodes_per_cell() {
    const char* e = std::getenv("EPP_KNN_NPC");
    return e && *e ? std::max(0.5, std::atof(e)) : kNodesPerCell;
}
}  // namespace epp
#define EPP_KNN_NOW() __builtin_amdgcn_s_memrealtime() /* 10 ns ticks */
// k_knn_tile, per block: begin, halo sizes scanned, halo copied, first query round's pass 1 /
// pass 2 / exact phase done, all queries done, end (EPP_KTL(k) stamps phase k once); the
// record adds the block's queries and halo candidates and the workgroup it ran on
#define EPP_KTL_BEGIN unsigned long long tl[8] = {EPP_KNN_NOW(), 0, 0, 0, 0, 0, 0, 0}
#define EPP_KTL(k)                              \
    do {                                        \
        if (tl[k] == 0ull) tl[k] = EPP_KNN_NOW(); \
    } while (0)
#define EPP_KTL_RECORD(dbg, b, nq, halo)                                                                    \
    do {                                                                                                    \
        if (dbg && threadIdx.x == 0 && b < kKnnTlBlocks) { /* (thread 0 is a query lane of slot 0) */       \
            tl[7] = EPP_KNN_NOW();                                                                          \
            for (int k_ = 0; k_ < 8; ++k_) dbg[16 * b + k_] = tl[k_];                                       \
            dbg[16 * b + 8] = (unsigned long long)(nq);                                                     \
            dbg[16 * b + 9] = (unsigned long long)(halo);                                                   \
            dbg[16 * b + 10] = blockIdx.x;                                                                  \
        }                                                                                                   \
    } while (0)
// k_knn_retry, per retried query i: start, end, bound (f64 bits), node
#define EPP_KRTL_BEGIN const unsigned long long rtl_t0 = EPP_KNN_NOW()
#define EPP_KRTL_RECORD(i, bound, node)                                                   \
    do {                                                                                  \
        if ((threadIdx.x & 63) == 0 && i < kKnnRetryTl) {                                 \
            g_knn_retry_tl[i][0] = rtl_t0;                                                \
            g_knn_retry_tl[i][1] = EPP_KNN_NOW();                                         \
            g_knn_retry_tl[i][2] = (unsigned long long)__double_as_longlong(bound);       \
            g_knn_retry_tl[i][3] = (unsigned long long)(node);                            \
        }                                                                                 \
    } while (0)
// k_knn_tile's invariants; the product guards them instead (the query then takes the retry path)
#define EPP_KNN_ASSERT(c) assert(c)
#else
namespace epp {
inline unsigned long long* knn_tl_begin(hipStream_t) { return nullptr; }
inline double knn_nodes_per_cell() { return kNodesPerCell; }
}  // namespace epp
#define EPP_KTL_BEGIN
#define EPP_KTL(k)
#define EPP_KTL_RECORD(dbg, b, nq, halo)
#define EPP_KRTL_BEGIN
#define EPP_KRTL_RECORD(i, bound, node)
#define EPP_KNN_ASSERT(c)
#endif
