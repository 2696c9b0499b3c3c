// knn_kernels.h — the k nearest neighbours of every node, three exact implementations with
// one answer (candidates ranked by (distance, index)):
//
//   all pairs  : k_knn, LDS-tiled (small tables; the tests' second opinion)      knn_walk.hip
//   shell walk : k_knn_grid, one thread per query walks shells of grid cells
//                (EPP_KNN_TILE=0; k = 32)                                         knn_walk.hip
//   tile+retry : the default.  k_knn_tile, a workgroup per 4^3-cell block with
//                its halo in LDS (knn_tile.hip), then k_knn_retry, one wave for
//                each query the tile pass could not settle (knn_retry.hip)
//
// The last two query the uniform grid (knn_grid.h) and the cell-sorted copy of the nodes that
// knn_build.hip makes: k_knn_bounds_part / k_knn_setup or k_knn_prep, k_knn_count, k_knn_scan,
// k_knn_scatter.  knn.hip holds the epp_knn* entry points (include/epp.h): validate, take a
// workspace, build the grid, query, retry.  A -DEPP_KNN_DIAG build adds the per-block and
// per-retry timelines (knn_diag.h, scripts/knn_timeline.py).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "knn_grid.h"

namespace epp {

constexpr double kNodesPerCell = 1.5;  // mean nodes per grid cell (EPP_KNN_NPC overrides in -DEPP_KNN_DIAG builds; tuned for k_knn_tile: ~90 queries per 4^3 block -> 2 lanes each)
// k_knn_tile's blocks of kTileB^3 cells and their kTileH-cell halos (k_knn_retry starts past them)
constexpr int kTileB = 4, kTileH = 2, kTileE = kTileB + 2 * kTileH, kTileCells = kTileE * kTileE * kTileE;

// The squared search radius the kernels take (none: every node is in range).  One rule on every
// path: a neighbour is in range iff its squared distance is < r2max, exclusive -- k_knn's strict
// compare against the empty slots' r2max, the retry's ranked lists, and knn_insert's tie against
// an empty slot (r2max, kKnnNone), which a candidate at exactly the radius loses.
inline double knn_r2max(double max_dist) { return max_dist > 0 ? max_dist * max_dist : 1e300; }

// f(std::integral_constant<int, K>) for the runtime k: K = 4, 8 or 16, or 32 where the kernel
// has that instance (K32; k is validated by the entry points).
template <bool K32, class F>
inline void knn_for_k(int k, F&& f) {
    if (k == 4) f(std::integral_constant<int, 4>{});
    else if (k == 8) f(std::integral_constant<int, 8>{});
    else if (k == 16 || !K32) f(std::integral_constant<int, 16>{});
    else if constexpr (K32) f(std::integral_constant<int, 32>{});
}

// The workspace's parts (KnnLayout's offsets into buf) as pointers.
struct KnnWs {
    KnnGrid* g;
    double* part;
    int *cell_of, *sidx;
    double* sxyz;
    int *cnt, *fill;
    unsigned long long* stat;
    int* start;
    int* retry;  // = cell_of, free once the scatter has run
    double* retry_b;
    int cap, scan_blocks, nclr;
};
inline KnnWs knn_ws_parts(char* buf, const KnnLayout& L) {
    KnnWs w;
    w.g = reinterpret_cast<KnnGrid*>(buf);
    w.part = reinterpret_cast<double*>(buf + L.part);
    w.cell_of = w.retry = reinterpret_cast<int*>(buf + L.cell);
    w.sidx = reinterpret_cast<int*>(buf + L.sidx);
    w.sxyz = reinterpret_cast<double*>(buf + L.sxyz);
    w.cnt = reinterpret_cast<int*>(buf + L.cnt);
    w.fill = reinterpret_cast<int*>(buf + L.fill);
    w.stat = reinterpret_cast<unsigned long long*>(buf + L.stat);
    w.start = reinterpret_cast<int*>(buf + L.start);
    w.retry_b = reinterpret_cast<double*>(buf + L.rbnd);
    w.cap = L.cap;
    w.scan_blocks = L.scan_blocks;
    // cnt, fill and the scan's status words are adjacent: cleared together by the first
    // kernel (never run the scatter on stale counters, never let the look-back take a stale
    // word for a published one)
    w.nclr = (int)((L.start - L.cnt) / sizeof(int));
    return w;
}

// Each enqueues its kernels on s and returns; the caller reads the launch status (launch_error()).
// (knn_build.hip) the grid over box_lo .. box_hi (the caller's box: shape on the host) or, with
// none, over the nodes' bounding box (measured on the device); the cell-sorted copy of the nodes
void knn_build_launch(const double* nodes, int n, const KnnWs& w, hipStream_t s, const double* box_lo,
                      const double* box_hi);
// (knn_walk.hip) k = 4, 8, 16 or 32
void knn_brute_launch(int k, const double* nodes, int n, double r2, int32_t* nbr, hipStream_t s);
void knn_walk_launch(int k, int n, double r2, const KnnWs& w, int32_t* nbr, hipStream_t s);
// (knn_tile.hip, knn_retry.hip) k = 4, 8 or 16; the retry pass follows the tile pass
void knn_tile_launch(int k, int cus, const double* nodes, double r2, const KnnWs& w, int32_t* nbr, hipStream_t s);
void knn_retry_launch(int k, int cus, const double* nodes, double r2, const KnnWs& w, int32_t* nbr, hipStream_t s);

}  // namespace epp
