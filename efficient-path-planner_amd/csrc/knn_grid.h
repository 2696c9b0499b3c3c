// knn_grid.h — the uniform grid of the exact k-NN, shared by the k-NN kernels (knn_kernels.h) and the
// batched planner's (plan_batch.hip): the grid parameters and their shape (KnnGrid,
// knn_grid_shape, knn_cell_axis), the workspace layout (KnnLayout), the cell-count scan
// (knn_scan_block) and the per-query pieces: sorted top-K insert, the exact stopping rule,
// the shell walk from global memory, the row store.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "planner_common.h"

namespace epp {
namespace {

// ---- k-NN over a uniform grid (exact; same answer as k_knn) ------------------------
// Cells of edge h hold ~3 nodes; every query walks shells of cells around its own cell
// until the k-th best squared distance is below the squared distance to the nearest
// face of the searched block (minus a rounding margin) — then no unvisited node can
// enter the list.  Candidates are ranked by (distance, index), so the visiting order
// (atomics in the scatter) never changes the result.
struct KnnGrid {
    double lo[3];
    double h, inv_h;
    int dims[3];
    int ncell;
    int next;    // k_knn_tile's block queue
    int nretry;  // k_knn_tile's retry list length
    int why[4];  // retry causes (diagnostics): list overflow, K-th beyond Dcut, shell rule, crowded (or spilled)
    // (no reader since the single-problem row-restricted k-NN went; kept because k_knn_tile<8>
    // allocates its registers differently over the shorter struct)
    double qs[3], qg[3], qbound;
};

// (k_knn_bounds_part's launch shape: KnnLayout holds its kBoundsBlocks partials)
constexpr int kBoundsThreads = 1024;
constexpr int kBoundsBlocks = 64;

// The grid over the box [mn, mx] for n nodes: cells of edge h with ~npc nodes each (flat
// point sets: thin slabs), at most cap cells.  Host (caller-given box) and device (the
// nodes' bounding box) compute it the same way.
__host__ __device__ inline void knn_grid_shape(const double (&mn)[3], const double (&mx)[3], int n, int cap,
                                               double npc, KnnGrid* g) {
    double ext[3], vol = 1.0, emax = 0.0;
    for (int d = 0; d < 3; ++d) {
        ext[d] = mx[d] - mn[d];
        emax = fmax(emax, ext[d]);
    }
    const double floor_ext = fmax(emax, 1e-9) * 1e-3;
    for (int d = 0; d < 3; ++d) vol *= fmax(ext[d], floor_ext);
    double h = cbrt(npc * vol / (double)(n > 1 ? n : 1));
    h = fmax(h, 1e-12);
    int dims[3];
    long long cells;
    for (;;) {
        cells = 1;
        for (int d = 0; d < 3; ++d) {
            dims[d] = (int)fmin(ext[d] / h, 1023.0) + 1;
            cells *= dims[d];
        }
        if (cells <= cap) break;
        h *= 1.25;
    }
    for (int d = 0; d < 3; ++d) {
        g->lo[d] = mn[d];
        g->dims[d] = dims[d];
    }
    g->h = h;
    g->inv_h = 1.0 / h;
    g->ncell = (int)cells;
    g->next = 0;
    g->nretry = 0;
    for (int i = 0; i < 4; ++i) g->why[i] = 0;
    for (int d = 0; d < 3; ++d) g->qs[d] = g->qg[d] = 0.0;
    g->qbound = 1e300;
}

__device__ __forceinline__ int knn_cell_axis(double v, const KnnGrid& g, int d) {
    const int c = (int)((v - g.lo[d]) * g.inv_h);
    return c < 0 ? 0 : (c >= g.dims[d] ? g.dims[d] - 1 : c);
}

// exclusive scan of cnt[0..ncell) into start[0..ncell]: block b scans cells
// [b kScanTile, (b+1) kScanTile), 16 consecutive counts per thread (16-byte loads and
// stores), its offset by look-back (lb_exclusive).  The grid is
// sized for the largest possible cell count (the count itself is on the device); blocks
// past it exit (no block waits on a later one).
constexpr int kScanThreads = 256, kScanPer = 16, kScanTile = kScanThreads * kScanPer;
__device__ __forceinline__ void knn_scan_block(const KnnGrid* __restrict__ gp, const int* __restrict__ cnt,
                                               int* __restrict__ start, unsigned long long* __restrict__ st,
                                               uint32_t tag, const int b) {
    static_assert(kScanPer % 4 == 0, "16-byte runs");
    __shared__ int wsum[kScanThreads / 64];
    __shared__ int s_excl;
    const int nc = gp->ncell;
    if (b * kScanTile > nc) return;  // (block-uniform; the block holding nc itself writes start[nc])
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b0 = b * kScanTile + kScanPer * threadIdx.x;
    int v[kScanPer];
    if (b0 + kScanPer <= nc) {  // (cnt and start are 256-byte aligned, b0 a multiple of 16)
#pragma unroll
        for (int u = 0; u < kScanPer / 4; ++u) {
            const int4 q = reinterpret_cast<const int4*>(cnt + b0)[u];
            v[4 * u] = q.x;
            v[4 * u + 1] = q.y;
            v[4 * u + 2] = q.z;
            v[4 * u + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < kScanPer; ++u) v[u] = b0 + u < nc ? cnt[b0 + u] : 0;
    }
    int sum = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) sum += v[u];
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int wbase = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
        wbase += w < wv ? wsum[w] : 0;
        tile += wsum[w];
    }
    if (wv == 0) {
        if (lane == 0) lb_publish(st, b, tag, b == 0, tile);
        const long long ex = b == 0 ? 0ll : lb_exclusive(st, b, tag);
        if (lane == 0) {
            if (b > 0) lb_publish(st, b, tag, true, ex + tile);
            s_excl = (int)ex;
        }
    }
    __syncthreads();
    int acc = s_excl + wbase + incl - sum;
    if (b0 + kScanPer <= nc) {
#pragma unroll
        for (int u = 0; u < kScanPer / 4; ++u) {
            int4 q;
            q.x = acc;
            q.y = q.x + v[4 * u];
            q.z = q.y + v[4 * u + 1];
            q.w = q.z + v[4 * u + 2];
            acc = q.w + v[4 * u + 3];
            reinterpret_cast<int4*>(start + b0)[u] = q;
        }
    } else {
#pragma unroll
        for (int u = 0; u < kScanPer; ++u) {
            if (b0 + u <= nc) start[b0 + u] = acc;  // (b0 + u == nc: the total)
            acc += v[u];
        }
    }
}

// An empty slot of a top-K list is (r2max, kKnnNone): the index below every node's, so a
// candidate at exactly the radius loses the tie against it and knn_insert keeps the one
// radius rule of every k-NN path -- in range iff d < max_dist^2 (epp.h).  It is also what
// the table holds for a missing neighbour, so the rows are stored as they are.
constexpr int kKnnNone = -1;

// Insert candidate (d, j) into the sorted top-K (distance, then index): ties keep the
// lower index first, so the visiting order never changes the result.  Branch-free: the
// entries ahead of (d, j) form a prefix of the list; each slot keeps its entry, takes
// (d, j), or takes its predecessor -- independent selects instead of a shifting chain of
// per-slot branches (which compiled to ~12 instructions, an exec-mask branch and four
// 64-bit moves per slot).
template <int K>
__device__ __forceinline__ void knn_insert(double (&bd)[K], int (&bi)[K], double d, int j) {
    if (!((d < bd[K - 1]) | ((d == bd[K - 1]) & (j < bi[K - 1])))) return;
    bool ahead[K];  // (bitwise, not short-circuit: no branches)
#pragma unroll
    for (int k = 0; k < K; ++k) ahead[k] = (bd[k] < d) | ((bd[k] == d) & (bi[k] < j));
#pragma unroll
    for (int k = K - 1; k >= 1; --k) {  // (reads slot k-1 before it is rewritten)
        bd[k] = ahead[k] ? bd[k] : (ahead[k - 1] ? d : bd[k - 1]);
        bi[k] = ahead[k] ? bi[k] : (ahead[k - 1] ? j : bi[k - 1]);
    }
    bd[0] = ahead[0] ? bd[0] : d;
    bi[0] = ahead[0] ? bi[0] : j;
}

// Exact stopping rule after shell r: the K-th best squared distance is below the squared
// distance from p to the nearest face of the searched (2r+1)^3 block that has cells
// beyond it (minus a rounding margin).  Also true when no cells are left.
// knn_bound returns that squared distance (+inf: no cells left; 0: never).
__device__ __forceinline__ double knn_bound(const KnnGrid& g, const int (&c)[3], const double (&p)[3], int r) {
    double dmin = 1e300;
    bool all = true;
    for (int d = 0; d < 3; ++d) {
        if (c[d] - r > 0) {
            dmin = fmin(dmin, p[d] - (g.lo[d] + (double)(c[d] - r) * g.h));
            all = false;
        }
        if (c[d] + r < g.dims[d] - 1) {
            dmin = fmin(dmin, (g.lo[d] + (double)(c[d] + r + 1) * g.h) - p[d]);
            all = false;
        }
    }
    if (all) return INFINITY;
    dmin -= g.h * 1e-6;  // cell assignment rounds; stay conservative
    return dmin > 0 ? dmin * dmin : 0.0;
}

template <int K>
__device__ __forceinline__ bool knn_done(const KnnGrid& g, const int (&c)[3], const double (&p)[3], int r,
                                         const double (&bd)[K]) {
    const double b = knn_bound(g, c, p, r);
    return b == INFINITY || bd[K - 1] < b;
}

// Shells r_from, r_from + 1, ... from global memory until knn_done (candidates BATCH
// at a time: their loads are in flight together).
template <int K, int BATCH = 4>
__device__ void knn_walk(const KnnGrid& g, const int (&c)[3], const double (&p)[3], int self, double (&bd)[K],
                         int (&bi)[K], const double* __restrict__ sxyz, const int* __restrict__ sidx,
                         const int* __restrict__ start, int r_from) {
    const int rmax = max(g.dims[0], max(g.dims[1], g.dims[2]));
    for (int r = r_from; r <= rmax; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = c[2] + dz;
            if (z < 0 || z >= g.dims[2]) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = c[1] + dy;
                if (y < 0 || y >= g.dims[1]) continue;
                const bool face = (dz == -r || dz == r || dy == -r || dy == r);
                const int step = (face || r == 0) ? 1 : 2 * r;
                for (int dx = -r; dx <= r; dx += step) {
                    const int x = c[0] + dx;
                    if (x < 0 || x >= g.dims[0]) continue;
                    const int cell = (z * g.dims[1] + y) * g.dims[0] + x;
                    const int e = start[cell + 1];
                    for (int q0 = start[cell]; q0 < e; q0 += BATCH) {
                        double dd[BATCH];
                        int jj[BATCH];
#pragma unroll
                        for (int u = 0; u < BATCH; ++u) {
                            const int q = min(q0 + u, e - 1);
                            jj[u] = q0 + u < e ? sidx[q] : self;  // past the cell: skipped below
                            const double ddx = sxyz[3 * q] - p[0], ddy = sxyz[3 * q + 1] - p[1], ddz = sxyz[3 * q + 2] - p[2];
                            dd[u] = (ddx * ddx + ddy * ddy) + ddz * ddz;
                        }
#pragma unroll
                        for (int u = 0; u < BATCH; ++u)
                            if (jj[u] != self) knn_insert<K>(bd, bi, dd[u], jj[u]);
                    }
                }
            }
        }
        if (knn_done<K>(g, c, p, r, bd)) break;
    }
}

template <int K>
__device__ __forceinline__ void knn_store(int32_t* __restrict__ nbr, int self, const int (&bi)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) nbr[(int64_t)self * K + k] = bi[k];  // (kKnnNone = -1: a missing neighbour)
}

// Scratch of the grid k-NN, every part 256-byte aligned: grid params | bounds partials | cell_of[n] |
// sidx[n] | sxyz[3n] | cnt[cap+1] | fill[cap+1] | scan status words | start[cap+1] | retry
// bounds[n]  (cap = max(64, n)).  cnt, fill and the status words are one range, cleared by
// the launch's first kernel: the workspace may hold anything when a launch starts (a caller
// workspace carved from a buffer that held other data, a tag of an earlier launch).
struct KnnLayout {
    size_t part, cell, sidx, sxyz, cnt, start, fill, rbnd, stat, bytes;
    int cap, scan_blocks;
};
inline KnnLayout knn_layout(int n) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    KnnLayout L;
    L.cap = max(64, n);
    L.part = 256;                                   // kBoundsBlocks x 6 doubles (3 KB)
    L.cell = L.part + al((size_t)kBoundsBlocks * 48);
    L.sidx = L.cell + al((size_t)n * 4);
    L.sxyz = L.sidx + al((size_t)n * 4);
    L.cnt = L.sxyz + al((size_t)n * 24);
    L.fill = L.cnt + al((size_t)(L.cap + 1) * 4);
    L.stat = L.fill + al((size_t)(L.cap + 1) * 4);
    L.scan_blocks = (L.cap + 1 + kScanTile) / kScanTile;  // cells <= cap; start[ncell] too
    L.start = L.stat + al((size_t)L.scan_blocks * 8);
    L.rbnd = L.start + al((size_t)(L.cap + 1) * 4);
    L.bytes = L.rbnd + al((size_t)std::max(n, 1) * 8);
    return L;
}

}  // namespace
}  // namespace epp
