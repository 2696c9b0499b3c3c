// knn.hip — the k nearest neighbours of every node, three exact implementations with one
// answer (candidates ranked by (distance, index)):
//
//   k_knn          : brute force, LDS-tiled (small tables; the tests' second opinion)
//   k_knn_bounds_part / k_knn_setup / k_knn_prep, k_knn_count, k_knn_scan, k_knn_scatter :
//                    the uniform grid (knn_grid.h) and the cell-sorted copy of the nodes
//   k_knn_grid     : one thread per query walks shells of cells (EPP_KNN_TILE=0; k = 32)
//   k_knn_tile     : the default: a workgroup per 4^3-cell block, its halo in LDS
//   k_knn_wave     : a wavefront per query out of the same halos (EPP_KNN_TILE=2)
//   k_knn_retry    : the queries the tile / wave pass could not settle, one wave each
//
// knn_grid_launch runs the grid pipeline on a workspace (KnnLayout); the epp_knn* entry
// points (include/epp.h) validate and pick brute force or grid.  A -DEPP_KNN_DIAG build adds
// the per-block and per-retry timelines (scripts/knn_timeline.py) and the timing ablations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <string>

#include "cached_ws.h"
#include "epp_internal.h"
#include "knn_grid.h"

namespace epp {
namespace {

constexpr int kKnnBlock = 256;

template <int K>
__global__ __launch_bounds__(kKnnBlock) void k_knn(const double* __restrict__ nodes, int n, double r2max,
                                                   int32_t* __restrict__ nbr) {
    __shared__ double tile[kKnnBlock * 3];
    const int i = blockIdx.x * kKnnBlock + threadIdx.x;
    double px = 0, py = 0, pz = 0;
    if (i < n) {
        px = nodes[3 * i];
        py = nodes[3 * i + 1];
        pz = nodes[3 * i + 2];
    }
    double bd[K];
    int bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bd[k] = r2max;
        bi[k] = -1;
    }
    for (int t0 = 0; t0 < n; t0 += kKnnBlock) {
        const int j = t0 + threadIdx.x;
        __syncthreads();
        if (j < n) {
            tile[3 * threadIdx.x] = nodes[3 * j];
            tile[3 * threadIdx.x + 1] = nodes[3 * j + 1];
            tile[3 * threadIdx.x + 2] = nodes[3 * j + 2];
        }
        __syncthreads();
        const int m = min(kKnnBlock, n - t0);
        for (int c = 0; c < m; ++c) {
            const double dx = tile[3 * c] - px, dy = tile[3 * c + 1] - py, dz = tile[3 * c + 2] - pz;
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d < bd[K - 1] && t0 + c != i) {  // strict: earlier index wins ties
                double vd = d;
                int vi = t0 + c;
                bool shift = false;  // once placed, the tail shifts down by one (keeps tie order)
#pragma unroll
                for (int k = 0; k < K; ++k) {  // insertion after any equal distances
                    shift = shift || vd < bd[k];
                    if (shift) {
                        const double td = bd[k];
                        const int ti = bi[k];
                        bd[k] = vd;
                        bi[k] = vi;
                        vd = td;
                        vi = ti;
                    }
                }
            }
        }
    }
    if (i < n)
#pragma unroll
        for (int k = 0; k < K; ++k) nbr[(int64_t)i * K + k] = bi[k];
}

constexpr int kKnnDefaultTile = 1;     // grid k-NN kernel without EPP_KNN_TILE: 1 k_knn_tile, 2 k_knn_wave
constexpr double kNodesPerCell = 1.5;  // mean nodes per grid cell (EPP_KNN_NPC overrides in -DEPP_KNN_DIAG builds; tuned for k_knn_tile: ~90 queries per 4^3 block -> 2 lanes each)

// Per-block min/max of the node coordinates: part[6 * block] = (min xyz, max xyz).  Also
// clears the cell counters (cnt and fill, nclr ints) for k_knn_count / k_knn_scatter.
__global__ __launch_bounds__(kBoundsThreads) void k_knn_bounds_part(const double* __restrict__ nodes, int n,
                                                                    double* __restrict__ part, int* __restrict__ clr,
                                                                    int nclr) {
    for (int i = blockIdx.x * kBoundsThreads + threadIdx.x; i < nclr; i += gridDim.x * kBoundsThreads) clr[i] = 0;
    __shared__ double smin[3][kBoundsThreads / 64], smax[3][kBoundsThreads / 64];
    double mn[3] = {1e308, 1e308, 1e308}, mx[3] = {-1e308, -1e308, -1e308};
    for (int i = blockIdx.x * kBoundsThreads + threadIdx.x; i < n; i += gridDim.x * kBoundsThreads)
        for (int d = 0; d < 3; ++d) {
            const double v = nodes[3 * i + d];
            mn[d] = fmin(mn[d], v);
            mx[d] = fmax(mx[d], v);
        }
    for (int d = 0; d < 3; ++d)
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = fmin(mn[d], __shfl_xor(mn[d], o, 64));
            mx[d] = fmax(mx[d], __shfl_xor(mx[d], o, 64));
        }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int d = 0; d < 3; ++d) {
            smin[d][wv] = mn[d];
            smax[d][wv] = mx[d];
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBoundsThreads / 64; ++w)
            for (int d = 0; d < 3; ++d) {
                mn[d] = fmin(mn[d], smin[d][w]);
                mx[d] = fmax(mx[d], smax[d][w]);
            }
        for (int d = 0; d < 3; ++d) {
            part[6 * blockIdx.x + d] = mn[d];
            part[6 * blockIdx.x + 3 + d] = mx[d];
        }
    }
}

// Grid shape from the block partials (one thread).
__global__ void k_knn_setup(const double* __restrict__ part, int nparts, int n, int cell_cap, double npc,
                            KnnGrid* __restrict__ g) {
    if (threadIdx.x >= 64 || blockIdx.x != 0) return;
    // one wave folds the partials (all loads in flight at once), lane 0 does the rest
    double mn[3] = {1e308, 1e308, 1e308}, mx[3] = {-1e308, -1e308, -1e308};
    for (int b = threadIdx.x; b < nparts; b += 64)
        for (int d = 0; d < 3; ++d) {
            mn[d] = fmin(mn[d], part[6 * b + d]);
            mx[d] = fmax(mx[d], part[6 * b + 3 + d]);
        }
    for (int d = 0; d < 3; ++d)
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = fmin(mn[d], __shfl_xor(mn[d], o, 64));
            mx[d] = fmax(mx[d], __shfl_xor(mx[d], o, 64));
        }
    if (threadIdx.x != 0) return;
    knn_grid_shape(mn, mx, n, cell_cap, npc, g);
}

// The caller-box path: the grid computed on the host, written here; clears the counters.
__global__ __launch_bounds__(kBoundsThreads) void k_knn_prep(KnnGrid gv, KnnGrid* __restrict__ g,
                                                             int* __restrict__ clr, int nclr) {
    for (int i = blockIdx.x * kBoundsThreads + threadIdx.x; i < nclr; i += gridDim.x * kBoundsThreads) clr[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *g = gv;
}

__global__ void k_knn_count(const double* __restrict__ nodes, int n, const KnnGrid* __restrict__ gp,
                            int* __restrict__ cell_of, int* __restrict__ cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const KnnGrid g = *gp;
    const int cx = knn_cell_axis(nodes[3 * i], g, 0), cy = knn_cell_axis(nodes[3 * i + 1], g, 1),
              cz = knn_cell_axis(nodes[3 * i + 2], g, 2);
    const int c = (cz * g.dims[1] + cy) * g.dims[0] + cx;
    cell_of[i] = c;
    atomicAdd(&cnt[c], 1);
}

__global__ __launch_bounds__(kScanThreads) void k_knn_scan(const KnnGrid* __restrict__ gp,
                                                           const int* __restrict__ cnt,
                                                           int* __restrict__ start,
                                                           unsigned long long* __restrict__ st, uint32_t tag) {
    knn_scan_block(gp, cnt, start, st, tag, blockIdx.x);
}

__global__ void k_knn_scatter(const double* __restrict__ nodes, int n, const int* __restrict__ cell_of,
                              const int* __restrict__ start, int* __restrict__ fill,
                              double* __restrict__ sxyz, int* __restrict__ sidx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = cell_of[i];
    const int pos = start[c] + atomicAdd(&fill[c], 1);
    if (pos >= start[c + 1]) return;  // cannot happen with cleared counters; never write out of range
    sidx[pos] = i;
    sxyz[3 * pos] = nodes[3 * i];
    sxyz[3 * pos + 1] = nodes[3 * i + 1];
    sxyz[3 * pos + 2] = nodes[3 * i + 2];
}

template <int K>
__global__ __launch_bounds__(256) void k_knn_grid(const KnnGrid* __restrict__ gp, int n, double r2max,
                                                  const double* __restrict__ sxyz,
                                                  const int* __restrict__ sidx,
                                                  const int* __restrict__ start,
                                                  int32_t* __restrict__ nbr) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;  // queries in cell order: coherent walks
    if (t >= n) return;
    const KnnGrid g = *gp;
    const int self = sidx[t];
    const double p[3] = {sxyz[3 * t], sxyz[3 * t + 1], sxyz[3 * t + 2]};
    const int c[3] = {knn_cell_axis(p[0], g, 0), knn_cell_axis(p[1], g, 1), knn_cell_axis(p[2], g, 2)};
    double bd[K];
    int bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bd[k] = r2max;
        bi[k] = 0x7fffffff;
    }
    knn_walk<K>(g, c, p, self, bd, bi, sxyz, sidx, start, 0);
#pragma unroll
    for (int k = 0; k < K; ++k) nbr[(int64_t)self * K + k] = bi[k] == 0x7fffffff ? -1 : bi[k];
}

// ---- tiled grid k-NN ----------------------------------------------------------------
// A workgroup takes a block of kTileB^3 cells: the block plus a kTileH-cell halo is
// copied into LDS and every query of the block looks at the kTileW^3 cube of cells
// around its own (shells 0..kTileH) out of LDS.  The per-query walk of k_knn_grid is
// bound by dependent global round trips; here they are LDS reads.
//
// Selection.  The sorted top-K insert costs ~K*12 VALU per candidate, and a wave pays
// it whenever any of its lanes inserts -- nearly always.  So the cube is scanned twice
// on float coordinates (relative to the block centre, one 16-byte LDS record per
// candidate): pass 1 histograms the squared distances into kTileNB quarter-octave bins;
// the bin where the running count reaches K gives a bound Dcut; pass 2 lists the
// candidates with float distance below Dcut + 2*delta (<= kTileL per query).  Only the
// listed candidates get an exact (double, from global memory) distance and the insert.
// delta bounds the float error of a squared distance within a halo (<= ~1e-4 h^2; 1e-3
// h^2 is used), so every candidate with exact d <= Dcut is listed; if the exact K-th
// distance is <= Dcut the result is therefore exact.  Queries where that check, the
// list size or the exact stopping rule after shell kTileH fails -- and all queries of a
// halo over capacity -- go to a retry list that k_knn_retry walks from global memory.
//
// Lanes per query: a block holds ~64..160 queries at ~2 nodes per cell; with fewer
// queries than threads, 2 or 4 adjacent lanes share one query (cube rows split between
// them; the histogram and the list are shared through LDS atomics), so blocks take about
// the same time whatever their query count.  Blocks come from a queue (costs differ).
// (Splitting blocks of more than 128 queries into two z-layer work units was tried in
// round 4: at ~1.5 nodes per cell the C4 tables have as many blocks as resident
// workgroups, so a second half only starts once a workgroup is free -- it lengthened the
// launch, 99 -> 110 us in the isolated trace.  A per-lane register histogram in pass 1
// instead of the LDS atomics was tried too; its build faulted in the crowded-cluster test
// and was withdrawn.  So was a first pass-1 stage over the 3^3 cells around the query: its
// cut alone is a valid but looser bound (exact phase 22 -> 29 us p50), and completing the
// bins below it from the rest of the cube takes two walks where one did (pass 1 19.8 ->
// 24.2 us p50; blocks at the grid's edges, where the 3^3 cells hold fewer than K, 42-50).)
#ifdef EPP_KNN_DIAG
constexpr int kKnnTlBlocks = 65536;  // timeline records
constexpr int kKnnRetryTl = 4096;    // retried queries recorded (k_knn_retry)
__device__ unsigned long long g_knn_retry_tl[kKnnRetryTl][4];
#endif
// Device asserts of k_knn_tile's invariants in the diagnostics build (-DEPP_KNN_DIAG); the
// product guards them instead (the query then takes the retry path)
#ifdef EPP_KNN_DIAG
#define EPP_KNN_ASSERT(c) assert(c)
#else
#define EPP_KNN_ASSERT(c) \
    do {                 \
    } while (0)
#endif
constexpr int kTileB = 4, kTileH = 2, kTileE = kTileB + 2 * kTileH, kTileCells = kTileE * kTileE * kTileE;
constexpr int kTileW = 2 * kTileH + 1;  // cube edge around the query's cell
constexpr int kTileRows = kTileW * kTileW;
constexpr int kTileCap = 1344;          // candidates a halo may hold (else its queries retry)
constexpr int kTileThreads = 256;
constexpr int kTileL = 32;              // per-query list length
constexpr int kTileNB = 16;             // histogram bins (16-bit counters, two per word)
constexpr int kTileSpill = 32;          // queries past 128 a block sends to the retry list (see below)
constexpr double kTileDelta = 1e-3;     // float error allowance, in h^2
constexpr double kPass1R2 = 4.5;        // pass 1 first visits the cells within sqrt(4.5) h

// A halo candidate in LDS: float x, y, z relative to the block centre + the node's sorted
// position (16 B).
typedef float4 TileCand;
typedef float4 TileQ;
__device__ __forceinline__ TileQ tile_q(const float4 c) { return c; }
__device__ __forceinline__ float tile_d(const float4 c, const float4& pf, float) {
    const float dx = c.x - pf.x, dy = c.y - pf.y, dz = c.z - pf.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ int tile_key(const float4 c, int) { return __float_as_int(c.w); }  // (sorted position)

// Visits the candidates of cube rows row0, row0 + rstep, ... around a query (a row =
// kTileW consecutive halo cells along x, one contiguous LDS range), four candidates at a
// time so their LDS reads are in flight together.  f(q, d_float, key, valid), key = what
// the self test compares (tile_key).
template <class F>
__device__ __forceinline__ void tile_rows(const int* cst, const TileCand* cand, int h0, int row0, int rstep,
                                          const TileQ& pf, float kq2, F&& f) {
    for (int row = row0; row < kTileRows; row += rstep) {
        const int a = h0 + ((row / kTileW) * kTileE + row % kTileW) * kTileE;
        const int q1 = cst[a + kTileW];
        for (int q = cst[a]; q < q1; q += 4) {
            TileCand c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) c[u] = cand[min(q + u, q1 - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qq = min(q + u, q1 - 1);
                f(qq, tile_d(c[u], pf, kq2), tile_key(c[u], qq), q + u < q1);
            }
        }
    }
}

// tile_rows restricted to the cells that can hold a candidate with squared distance
// <= thr: a row is skipped when its (y, z) gap alone exceeds thr, else trimmed to the x
// cells within reach (still one contiguous LDS range).  fr = the query's offset inside its
// own cell per axis; gaps are shrunk by a hair, so the culling only ever keeps too much.
__device__ __forceinline__ double tile_gap(int off, double fr, double h) {
    const double g = off < 0 ? fr + (double)(-off - 1) * h : (off > 0 ? (h - fr) + (double)(off - 1) * h : 0.0);
    return fmax(g - 1e-6 * h, 0.0);
}

template <class F>
__device__ __forceinline__ void tile_rows_near(const int* cst, const TileCand* cand, int h0, int row0, int rstep,
                                               const TileQ& pf, float kq2, const double (&fr)[3], double h, double thr,
                                               F&& f) {
    const double gx1 = tile_gap(1, fr[0], h), gx2 = tile_gap(2, fr[0], h);
    const double gxm1 = tile_gap(-1, fr[0], h), gxm2 = tile_gap(-2, fr[0], h);
    for (int row = row0; row < kTileRows; row += rstep) {
        const int rz = row / kTileW, ry = row % kTileW;
        const double gy = tile_gap(ry - kTileH, fr[1], h), gz = tile_gap(rz - kTileH, fr[2], h);
        const double gyz = gy * gy + gz * gz;
        if (gyz > thr) continue;
        const double rem = thr - gyz;
        const int xa = gxm2 * gxm2 <= rem ? 0 : (gxm1 * gxm1 <= rem ? 1 : 2);
        const int xb = gx2 * gx2 <= rem ? 4 : (gx1 * gx1 <= rem ? 3 : 2);
        const int a = h0 + (rz * kTileE + ry) * kTileE;
        const int q1 = cst[a + xb + 1];
        for (int q = cst[a + xa]; q < q1; q += 4) {
            TileCand c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) c[u] = cand[min(q + u, q1 - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qq = min(q + u, q1 - 1);
                f(qq, tile_d(c[u], pf, kq2), tile_key(c[u], qq), q + u < q1);
            }
        }
    }
}
static_assert(kTileW == 5 && kTileH == 2, "tile_rows_near trims rows of 5 cells");

// Queries the tile pass could not settle (rare: sparse corners, crowded halos), one
// wave per query so a single far walk does not serialise on dependent global loads:
// lanes take x-rows of cells (each one contiguous range of the cell-sorted nodes) and
// keep their own top-K.  First the cube of radius kTileH + 1, then one shell at a time
// until the stopping rule holds -- tested cheaply as ">= K listed candidates below the
// bound" over all lanes -- then K rounds of a wave-wide (distance, index) arg-min merge
// the lane lists; lane 0 writes the result.  Called by whole waves.
template <int K>
__device__ __forceinline__ void knn_retry_wave(const KnnGrid& g, double r2max, const double* __restrict__ nodes,
                               const double* __restrict__ sxyz, const int* __restrict__ sidx,
                               const int* __restrict__ start, int self, double bound2, int32_t* __restrict__ nbr) {
    const int lane = threadIdx.x & 63;
    const int rmax = max(g.dims[0], max(g.dims[1], g.dims[2]));
    const double p[3] = {nodes[3 * (int64_t)self], nodes[3 * (int64_t)self + 1], nodes[3 * (int64_t)self + 2]};
    const int c[3] = {knn_cell_axis(p[0], g, 0), knn_cell_axis(p[1], g, 1), knn_cell_axis(p[2], g, 2)};
    // Without a bound (a crowded or spilled tile query) a trial bound of (1.6h)^2 is tried
    // first: it holds ~26 nodes at the grid's density (~35 in the dense blocks that spill),
    // and the list is exact whenever it holds at least K (every node outside is farther
    // than every listed one); else the per-lane shell walk below.  ((2h)^2 held ~70 nodes
    // in a spilling block: those retries took 7-16 us against 4.7 for the bounded ones.)
    const bool trial = !(bound2 < 1e299);
    const double b2 = trial ? 2.56 * g.h * g.h : bound2;
    if (b2 < 1e299) {  // wave-uniform
        // K actual candidates lie within sqrt(bound2) (the tile pass found them, with the
        // same exact distances), so the true top K is among the candidates with
        // d <= bound2 in the box p +- sqrt(bound2) (cell mapping monotone; the radius is
        // padded against the rounding of p +- r).  Rows of the box are spread over the
        // lanes; every candidate within the bound goes to an LDS list (a few dozen), and
        // each listed entry's rank in (distance, index) order is counted against the whole
        // list: the K lowest ranks are the answer.  No per-lane sorted lists, no merge
        // rounds.  (A list over capacity falls through to the per-lane walk below.)
        constexpr int kCap = 512;
        __shared__ double s_d[kCap];
        __shared__ int s_j[kCap];
        __shared__ int s_n;
        if (lane == 0) s_n = 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the clear before any append
        const double r = sqrt(b2) * (1.0 + 1e-9) + 1e-12 * (1.0 + fabs(p[0]) + fabs(p[1]) + fabs(p[2]));
        int lo[3], hi[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = knn_cell_axis(p[d] - r, g, d);
            hi[d] = knn_cell_axis(p[d] + r, g, d);
        }
        const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
        for (int row = lane; row < ny * nz; row += 64) {
            const int a = ((lo[2] + row / ny) * g.dims[1] + lo[1] + row % ny) * g.dims[0];
            const int e = start[a + hi[0] + 1];
            for (int q0 = start[a + lo[0]]; q0 < e; q0 += 4) {
                double dd[4];
                int jj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = min(q0 + u, e - 1);
                    jj[u] = q0 + u < e ? sidx[q] : self;  // past the row: skipped below
                    const double ddx = sxyz[3 * q] - p[0], ddy = sxyz[3 * q + 1] - p[1], ddz = sxyz[3 * q + 2] - p[2];
                    dd[u] = (ddx * ddx + ddy * ddy) + ddz * ddz;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (jj[u] != self && dd[u] <= b2 && dd[u] < r2max) {
                        const int at = atomicAdd(&s_n, 1);
                        if (at < kCap) {
                            s_d[at] = dd[u];
                            s_j[at] = jj[u];
                        }
                    }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's appends are complete
        const int cnt = s_n;
        if (cnt <= 64 && (!trial || cnt >= K)) {  // wave-uniform: entry i on lane i
            // ranks against the other entries read by v_readlane (no LDS round trip per
            // entry, which the loop below waits out)
            const bool mine = lane < cnt;
            const double di = mine ? s_d[lane] : 0.0;
            const int ji = mine ? s_j[lane] : 0;
            const int dlo = __double2loint(di), dhi = __double2hiint(di);
            int rank = 0;
            for (int f = 0; f < cnt; ++f) {
                const double df = __hiloint2double(__builtin_amdgcn_readlane(dhi, f), __builtin_amdgcn_readlane(dlo, f));
                rank += ((df < di) | ((df == di) & (__builtin_amdgcn_readlane(ji, f) < ji))) ? 1 : 0;
            }
            if (mine && rank < K) nbr[(int64_t)self * K + rank] = ji;
            if (lane >= cnt && lane < K) nbr[(int64_t)self * K + lane] = -1;  // (fewer than K)
            return;
        }
        if (cnt <= kCap && (!trial || cnt >= K)) {  // wave-uniform
            for (int i = lane; i < cnt; i += 64) {
                const double di = s_d[i];
                const int ji = s_j[i];
                int rank = 0;
                for (int f = 0; f < cnt; ++f) {  // (every lane reads entry f: LDS broadcast)
                    const double df = s_d[f];
                    rank += ((df < di) | ((df == di) & (s_j[f] < ji))) ? 1 : 0;
                }
                if (rank < K) nbr[(int64_t)self * K + rank] = ji;
            }
            for (int k = cnt + lane; k < K; k += 64) nbr[(int64_t)self * K + k] = -1;  // (fewer than K)
            return;
        }
    }
    double bd[K];
    int bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bd[k] = r2max;
        bi[k] = 0x7fffffff;
    }
    // candidates of cells [xa, xb] of row (y, z) into the lane's list
    auto scan = [&](int y, int z, int xa, int xb) {
        const int a = (z * g.dims[1] + y) * g.dims[0];
        const int e = start[a + xb + 1];
        for (int q0 = start[a + xa]; q0 < e; q0 += 4) {
            double dd[4];
            int jj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(q0 + u, e - 1);
                jj[u] = q0 + u < e ? sidx[q] : self;  // past the row: skipped below
                const double ddx = sxyz[3 * q] - p[0], ddy = sxyz[3 * q + 1] - p[1], ddz = sxyz[3 * q + 2] - p[2];
                dd[u] = (ddx * ddx + ddy * ddy) + ddz * ddz;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (jj[u] != self) knn_insert<K>(bd, bi, dd[u], jj[u]);
        }
    };
    if (bound2 < 1e299) {  // wave-uniform
        // K actual candidates lie within sqrt(bound2) (the tile pass found them), so every
        // candidate of the true top K does too: one pass over the cells of the box
        // p +- sqrt(bound2) (the cell mapping is monotone; the radius is padded against
        // the rounding of p +- r), rows spread over the lanes, no stopping rule
        const double r = sqrt(bound2) * (1.0 + 1e-9) + 1e-12 * (1.0 + fabs(p[0]) + fabs(p[1]) + fabs(p[2]));
        int lo[3], hi[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = knn_cell_axis(p[d] - r, g, d);
            hi[d] = knn_cell_axis(p[d] + r, g, d);
        }
        const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
        for (int row = lane; row < ny * nz; row += 64) scan(lo[1] + row % ny, lo[2] + row / ny, lo[0], hi[0]);
    } else {
    for (int R = kTileH + 1;; ++R) {  // wave-uniform
        // rows of shell R (the whole cube the first time)
        const bool cube = R == kTileH + 1;
        const int w = 2 * R + 1;
        for (int row = lane; row < w * w; row += 64) {
            const int dz = row / w - R, dy = row % w - R;
            const int z = c[2] + dz, y = c[1] + dy;
            if (z < 0 || z >= g.dims[2] || y < 0 || y >= g.dims[1]) continue;
            const int xa = max(c[0] - R, 0), xb = min(c[0] + R, g.dims[0] - 1);
            if (cube || dz == -R || dz == R || dy == -R || dy == R) {
                scan(y, z, xa, xb);
            } else {  // inner rows: only the shell's two end cells
                if (c[0] - R >= 0) scan(y, z, c[0] - R, c[0] - R);
                if (c[0] + R < g.dims[0]) scan(y, z, c[0] + R, c[0] + R);
            }
        }
        const double bound = knn_bound(g, c, p, R);
        if (bound != INFINITY && R < rmax && !(r2max < bound)) {  // (radius below it: done)
            int below = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) below += (bi[k] != 0x7fffffff && bd[k] < bound) ? 1 : 0;
            for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
            if (below < K) continue;
        }
        break;
    }
    }
    // merge: K rounds of arg-min over the lane list heads
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double md = bd[0];
        int mi = bi[0];
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(md, o, 64);
            const int oi = __shfl_xor(mi, o, 64);
            if (od < md || (od == md && oi < mi)) {
                md = od;
                mi = oi;
            }
        }
        if (lane == 0) nbr[(int64_t)self * K + k] = mi == 0x7fffffff ? -1 : mi;
        if (mi != 0x7fffffff && bi[0] == mi) {  // the winning lane drops its head
#pragma unroll
            for (int t = 0; t + 1 < K; ++t) {
                bd[t] = bd[t + 1];
                bi[t] = bi[t + 1];
            }
            bd[K - 1] = r2max;
            bi[K - 1] = 0x7fffffff;
        }
    }
}

// (An LDS copy of the halo's exact coordinates for the exact phase was tried: with it two
// workgroups fit per CU instead of three, and the kernel was slower.  So was an exact phase
// with one wavefront per query -- its candidates one per lane, ranks counted by v_readlane,
// 145 -> 114 VGPRs: each query then waits out its own gathers one after another, ~3 us per
// query and wave against ~22 us for all of a block's queries at once on one thread each;
// 126 -> 185 us per table.  And four workgroups per CU (halo cap 992, 24-entry lane lists,
// 128 VGPRs with 5 spilled): 126 -> 142 us per table.)
template <int K>
__global__ __launch_bounds__(kTileThreads, 3) void k_knn_tile(KnnGrid* __restrict__ gp, double r2max,
                                                           const double* __restrict__ nodes,
                                                           const double* __restrict__ sxyz,
                                                           const int* __restrict__ sidx,
                                                           const int* __restrict__ start,
                                                           int* __restrict__ retry, double* __restrict__ retry_b,
                                                           int32_t* __restrict__ nbr, int mode,
                                                           unsigned long long* __restrict__ dbg) {
    __shared__ TileCand cand[kTileCap];                    // x, y, z (block-centre relative), sorted position
#define EPP_SPOS(q) __float_as_int(cand[q].w)
    __shared__ uint16_t qh[kTileCap];                      // the block's queries (LDS positions)
    __shared__ int cst[kTileCells + 1];                    // halo cell -> LDS offset
    __shared__ uint32_t hist[kTileNB / 2][kTileThreads];  // [bin pair][query slot]
    __shared__ uint16_t lst[kTileL][kTileThreads];         // [entry][lane]: each lane's own list
    __shared__ int wsum[kTileThreads / 64];
    __shared__ uint8_t s_nown[kTileThreads];  // list entries per lane (saturated)
    __shared__ int8_t s_cut[kTileThreads];    // histogram cut per query slot
    __shared__ int s_nq, s_b;
    const KnnGrid g = *gp;
    const int nbx = (g.dims[0] + kTileB - 1) / kTileB, nby = (g.dims[1] + kTileB - 1) / kTileB,
              nbz = (g.dims[2] + kTileB - 1) / kTileB;
    const int nblocks = nbx * nby * nbz;
    const int n_nodes = start[g.ncell];  // (the guards below: retry appends, sorted positions)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr int kPer = kTileCells / kTileThreads;  // halo cells per thread
    static_assert(kTileCells % kTileThreads == 0, "");
    // histogram origin: bins span d in [t0, 16 t0), t0 ~ a quarter of the expected K-th
    // squared distance at ~2 nodes per cell (~(K/16)^(2/3) * 1.5 h^2)
    const float kscale = K <= 4 ? 0.40f : K <= 8 ? 0.63f : 1.0f;
    const double t0 = g.h * g.h * 0.35 * kscale;
    const float inv_t0 = (float)(1.0 / t0);
    const double delta = kTileDelta * g.h * g.h;
    const float kq2 = 1.0f;
    for (;;) {
        if (threadIdx.x == 0) s_b = atomicAdd(&gp->next, 1);
        __syncthreads();
        const int b = s_b;  // block-uniform
        if (b >= nblocks) break;
        const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
        const int ox = bx * kTileB - kTileH, oy = by * kTileB - kTileH, oz = bz * kTileB - kTileH;
        const double cen[3] = {g.lo[0] + (ox + 0.5 * kTileE) * g.h, g.lo[1] + (oy + 0.5 * kTileE) * g.h,
                               g.lo[2] + (oz + 0.5 * kTileE) * g.h};
#ifdef EPP_KNN_DIAG
        // phase timeline (diagnostics builds): begin, halo sizes scanned, halo copied, first
        // query round's pass 1 / pass 2 / exact phase done, all queries done, end; counts
        unsigned long long tl[8] = {__builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0, 0, 0, 0};
#define EPP_KTL(k) \
    do {           \
        if (tl[k] == 0ull) tl[k] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define EPP_KTL(k) \
    do {           \
    } while (0)
#endif
        // 1. halo cell sizes -> exclusive scan (thread t owns halo cells kPer*t ..)
        int cnt[kPer], cell0[kPer], tot = 0;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int t = kPer * threadIdx.x + u;
            const int x = ox + t % kTileE, y = oy + (t / kTileE) % kTileE, z = oz + t / (kTileE * kTileE);
            const bool in = x >= 0 && x < g.dims[0] && y >= 0 && y < g.dims[1] && z >= 0 && z < g.dims[2];
            const int cell = in ? (z * g.dims[1] + y) * g.dims[0] + x : 0;
            const int s0 = start[cell], s1 = start[cell + 1];
            cnt[u] = in ? s1 - s0 : 0;
            cell0[u] = s0;
            tot += cnt[u];
        }
        int incl = tot;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kTileThreads / 64; ++w) {
            base += w < wv ? wsum[w] : 0;
            total += wsum[w];
        }
        base += incl - tot;
        {
            int acc = base;
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                cst[kPer * threadIdx.x + u] = acc;
                acc += cnt[u];
            }
        }
        if (threadIdx.x == 0) {
            cst[kTileCells] = total;
            s_nq = 0;
        }
        __syncthreads();
        EPP_KTL(1);
        if (total <= kTileCap) {  // block-uniform
            // 2. copy the halo's candidates; list the block's own nodes as queries
            int acc = base;
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int t = kPer * threadIdx.x + u;
                const int hx = t % kTileE, hy = (t / kTileE) % kTileE, hz = t / (kTileE * kTileE);
                const bool inner = hx >= kTileH && hx < kTileH + kTileB && hy >= kTileH && hy < kTileH + kTileB &&
                                   hz >= kTileH && hz < kTileH + kTileB;
                const int q0 = (inner && cnt[u]) ? atomicAdd(&s_nq, cnt[u]) : 0;
                for (int q = 0; q < cnt[u]; ++q) {
                    const int sg = cell0[u] + q;
                    const double x = sxyz[3 * sg], y = sxyz[3 * sg + 1], z = sxyz[3 * sg + 2];
                    cand[acc + q] = make_float4((float)(x - cen[0]), (float)(y - cen[1]), (float)(z - cen[2]),
                                                __int_as_float(sg));  // (sorted position: see the exact phase)
                    if (inner) qh[q0 + q] = (uint16_t)(acc + q);
                }
                acc += cnt[u];
            }
            __syncthreads();
            EPP_KTL(2);
            // 3. queries, lpq adjacent lanes per query
#ifdef EPP_KNN_DIAG
            const int nq_all = mode == 4 ? 0 : s_nq;  // mode 4: timing ablation (inexact; diagnostics builds only)
#else
            const int nq_all = s_nq;
#endif
            // block-uniform; one lane per query only above 128 + kTileSpill queries (a second
            // round of queries would cost the block ~45 us).  A block just past 128 queries
            // keeps two lanes per query for its first 128 and sends the rest to the retry list
            // (one wave each in k_knn_retry, in parallel): with one lane per query such a
            // block was the launch's slowest (~104 us against ~85 for the next).
            const bool spill = nq_all > kTileThreads / 2 && nq_all <= kTileThreads / 2 + kTileSpill;
            const int nq = spill ? kTileThreads / 2 : nq_all;
            if (spill)
                for (int q = nq + (int)threadIdx.x; q < nq_all; q += kTileThreads) {
                    const int at = atomicAdd(&gp->nretry, 1);
                    EPP_KNN_ASSERT(at < n_nodes);
                    if (at >= n_nodes) continue;
                    retry[at] = sidx[EPP_SPOS(qh[q])];
                    retry_b[at] = INFINITY;
                    atomicAdd(&gp->why[3], 1);
                }
            const int lpq = nq <= kTileThreads / 4 ? 4 : nq <= kTileThreads / 2 ? 2 : 1;
            const int slot = threadIdx.x / lpq, sub = threadIdx.x % lpq;
            // (a query's lpq lanes are adjacent lanes of one wave: its histogram needs no
            // workgroup barrier; the exact phase reads the lists on other threads, after one)
            for (int qb = 0; qb < nq; qb += kTileThreads / lpq) {  // block-uniform
                const int qi = qb + slot;
                const bool live = qi < nq;
                const int me = live ? qh[qi] : 0;
                const TileQ pf = tile_q(cand[me]);
                const int sself = EPP_SPOS(me);  // the query's sorted position
                const int skey = tile_key(cand[me], me);  // what its self test compares
                // exact coordinates and cell (the row offsets; the final distances)
                const double p[3] = {sxyz[3 * (int64_t)sself], sxyz[3 * (int64_t)sself + 1], sxyz[3 * (int64_t)sself + 2]};
                const int c[3] = {knn_cell_axis(p[0], g, 0), knn_cell_axis(p[1], g, 1), knn_cell_axis(p[2], g, 2)};
                const int h0 = ((c[2] - oz - kTileH) * kTileE + (c[1] - oy - kTileH)) * kTileE + (c[0] - ox - kTileH);
                const double fr[3] = {p[0] - (g.lo[0] + (double)c[0] * g.h), p[1] - (g.lo[1] + (double)c[1] * g.h),
                                      p[2] - (g.lo[2] + (double)c[2] * g.h)};
                // pass 1: histogram of bin keys (exponent + two mantissa bits of d / t0): the
                // query's slot of `hist`, LDS atomics from its lanes (one wave: in-order LDS
                // operations order the clear before them and the read after).  First over
                // the cells within sqrt(kPass1R2) h only (about half the cube); its counts
                // are complete for every bin ending below kPass1R2 h^2 - delta (a candidate
                // of a skipped cell has exact d > kPass1R2 h^2, float d > that - delta), so
                // its cut stands when it ends there -- nearly always; else the whole cube.
                int cut = -1;
                for (int full = 0; full < 2; ++full) {  // query-uniform (the slot's lanes read one histogram)
                    if (sub == 0) {
#pragma unroll
                        for (int w = 0; w < kTileNB / 2; ++w) hist[w][slot] = 0u;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    auto bin = [&](int, float d, int j, bool valid) {
                        const int kb = max((int)(__float_as_uint(d * inv_t0) >> 21) - (127 << 2), 0);
                        if (valid && j != skey && kb < kTileNB) atomicAdd(&hist[kb >> 1][slot], 1u << ((kb & 1) << 4));
                    };
                    if (live) {
                        if (full) tile_rows(cst, cand, h0, sub, lpq, pf, kq2, bin);
                        else tile_rows_near(cst, cand, h0, sub, lpq, pf, kq2, fr, g.h, kPass1R2 * g.h * g.h, bin);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    int run = 0;
                    cut = -1;
#pragma unroll
                    for (int w = 0; w < kTileNB / 2; ++w) {
                        const uint32_t hv = hist[w][slot];
                        run += hv & 0xffff;
                        if (run >= K && cut < 0) cut = 2 * w;
                        run += hv >> 16;
                        if (run >= K && cut < 0) cut = 2 * w + 1;
                    }
                    const double edge = cut < 0 ? INFINITY : (double)__uint_as_float((uint32_t)(cut + 1 + (127 << 2)) << 21) * t0;
                    if (full || edge <= kPass1R2 * g.h * g.h - delta) break;
                }
                EPP_KTL(3);
                // Dcut: upper edge of bin `cut` (none reached K: no bound)
                const double dcut = cut < 0 ? INFINITY : (double)__uint_as_float((uint32_t)(cut + 1 + (127 << 2)) << 21) * t0;
                const float dlist = (float)(dcut + 2.0 * delta);
                // pass 2: list the candidates below Dcut + 2 delta, visiting only the cells
                // within Dcut + 3 delta (a candidate's float distance is within delta of
                // its exact one, which is at least its cell's distance); every lane keeps
                // its own list (its column of lst: no atomics)
                int nown = 0;
                if (live) {
                    const double thr2 = cut < 0 ? INFINITY : dcut + 3.0 * delta;
                    tile_rows_near(cst, cand, h0, sub, lpq, pf, kq2, fr, g.h, thr2, [&](int q, float d, int j, bool valid) {
                        if (valid && j != skey && d < dlist) {
                            if (nown < kTileL) lst[nown][threadIdx.x] = (uint16_t)q;
                            ++nown;
                        }
                    });
                }
                // The exact phase runs compacted: query slot t on thread t, i.e. the first
                // 256 / lpq threads as full waves (with lpq lanes per query only one lane of
                // each would work, and the idle lanes would still take the SIMD's issue
                // cycles).  The list counts and cuts go through LDS, ordered by a barrier.
                s_nown[threadIdx.x] = (uint8_t)min(nown, 255);
                if (sub == 0) s_cut[slot] = (int8_t)cut;
                __syncthreads();
                EPP_KTL(4);
                const int qx = qb + (int)threadIdx.x;
                if ((int)threadIdx.x < kTileThreads / lpq && qx < nq) {
                const int tcol = (int)threadIdx.x * lpq;  // the query's first list column
                const int sx = EPP_SPOS(qh[qx]);
                const int self = sidx[sx];
                const double p[3] = {sxyz[3 * (int64_t)sx], sxyz[3 * (int64_t)sx + 1], sxyz[3 * (int64_t)sx + 2]};
                const int c[3] = {knn_cell_axis(p[0], g, 0), knn_cell_axis(p[1], g, 1), knn_cell_axis(p[2], g, 2)};
                const int cutx = s_cut[threadIdx.x];
                const double dcut = cutx < 0 ? INFINITY : (double)__uint_as_float((uint32_t)(cutx + 1 + (127 << 2)) << 21) * t0;
                int ncol[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) ncol[o] = o < lpq ? (int)s_nown[tcol + o] : 0;
                int nl = 0;
                bool ok = true;
                double rbound = INFINITY;  // (none: the retry walks shells)
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (o < lpq) {
                        nl += ncol[o];
                        ok = ok && ncol[o] <= kTileL;
                    }
                if (ok) {
                    double bd[K];
                    int bi[K];
                    bool guard_ok = true;
                    const int tot_halo = cst[kTileCells];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        bd[k] = r2max;
                        bi[k] = 0x7fffffff;
                    }
                    // exact distances of the listed candidates (the query's lanes' columns in
                    // turn), kLoads at a time in flight
                    constexpr int kLoads = 4;
                    for (int i0 = 0; i0 < nl; i0 += kLoads) {
                        double dd[kLoads];
                        int jj[kLoads];
#pragma unroll
                        for (int u = 0; u < kLoads; ++u) {
                            int e = min(i0 + u, nl - 1), col = 0;  // entry e -> (lane column, row)
                            bool go = true;
#pragma unroll
                            for (int o = 0; o < 3; ++o) {
                                const bool past = (go & (o + 1 < lpq)) & (e >= ncol[o]);
                                e -= past ? ncol[o] : 0;
                                col += past ? 1 : 0;
                                go = past;
                            }
                            // (the halo's entries are its cells' contiguous runs of the cell-sorted
                            // copy: these gathers hit the few KB the block's queries share in L1,
                            // where the nodes' original order scattered them over the table)
                            // (guards: a listed LDS position inside the halo, its sorted position
                            // inside the table -- what a wrong pass-1 cut or list could break; a
                            // failed guard sends the query to the retry instead of reading out of
                            // range; the diagnostics build asserts them)
                            const int q0 = lst[e][tcol + col];
                            const bool qok = q0 >= 0 && q0 < tot_halo;
                            const int q = qok ? q0 : 0;
                            const int sg0 = EPP_SPOS(q);
                            const bool sok = sg0 >= 0 && sg0 < n_nodes;
                            EPP_KNN_ASSERT(qok && sok);
                            guard_ok = guard_ok && qok && sok;
                            const int sg = sok ? sg0 : 0;
                            jj[u] = sidx[sg];
                            const double ddx = sxyz[3 * (int64_t)sg] - p[0], ddy = sxyz[3 * (int64_t)sg + 1] - p[1],
                                         ddz = sxyz[3 * (int64_t)sg + 2] - p[2];
                            dd[u] = (ddx * ddx + ddy * ddy) + ddz * ddz;
                        }
#ifdef EPP_KNN_DIAG
                        if (mode == 5 || mode == 6) {  // timing ablation (inexact): no inserts
                            bd[0] = fmin(bd[0], fmin(fmin(dd[0], dd[1]), fmin(dd[2], dd[3])));
                            continue;
                        }
#endif
#pragma unroll
                        for (int u = 0; u < kLoads; ++u)
                            if (i0 + u < nl) knn_insert<K>(bd, bi, dd[u], jj[u]);
                    }
                    // exact when the K-th distance is within the listed range and the cube
                    // suffices (stopping rule after shell kTileH)
                    const bool in_range = bd[K - 1] <= dcut;
                    ok = guard_ok && in_range && knn_done<K>(g, c, p, kTileH, bd);
#ifdef EPP_KNN_DIAG
                    if (mode == 5 || mode == 6) ok = true;  // (ablation: no retries, no answer)
                    else
#endif
                    if (ok) knn_store<K>(nbr, self, bi);
                    else atomicAdd(&gp->why[in_range ? 2 : 1], 1);
                    // a retry's search bound: K actual candidates within bd[K-1] (<= r2max)
                    rbound = bd[K - 1];
                } else {
                    atomicAdd(&gp->why[0], 1);
                }
                if (!ok) {
                    const int at = atomicAdd(&gp->nretry, 1);
                    EPP_KNN_ASSERT(at < n_nodes);
                    if (at < n_nodes) {  // (each node retries at most once: at < n)
                        retry[at] = self;
                        retry_b[at] = rbound;
                    }
                }
#ifdef EPP_KNN_DIAG
                if (tl[5] == 0ull) tl[5] = __builtin_amdgcn_s_memrealtime();
#endif
                }
                __syncthreads();  // the next round rewrites the lists, histograms and counts
            }
            EPP_KTL(6);
        } else {
            // crowded halo: the block's queries retry from global memory
            for (int t2 = threadIdx.x; t2 < kTileB * kTileB * kTileB; t2 += kTileThreads) {
                const int x = bx * kTileB + t2 % kTileB, y = by * kTileB + (t2 / kTileB) % kTileB,
                          z = bz * kTileB + t2 / (kTileB * kTileB);
                if (x >= g.dims[0] || y >= g.dims[1] || z >= g.dims[2]) continue;
                const int cell = (z * g.dims[1] + y) * g.dims[0] + x;
                const int e = start[cell + 1];
                for (int t = start[cell]; t < e; ++t) {
                    const int at = atomicAdd(&gp->nretry, 1);
                    EPP_KNN_ASSERT(at < n_nodes);
                    if (at >= n_nodes) continue;
                    retry[at] = sidx[t];
                    retry_b[at] = INFINITY;
                }
                if (e > start[cell]) atomicAdd(&gp->why[3], e - start[cell]);
            }
        }
        __syncthreads();  // the LDS tile is rewritten by the next block
#ifdef EPP_KNN_DIAG
        if (dbg && threadIdx.x == 0 && b < kKnnTlBlocks) {  // (thread 0 is a query lane of slot 0)
            tl[7] = __builtin_amdgcn_s_memrealtime();
            for (int k = 0; k < 8; ++k) dbg[16 * b + k] = tl[k];
            dbg[16 * b + 8] = (unsigned long long)s_nq;
            dbg[16 * b + 9] = (unsigned long long)total;
            dbg[16 * b + 10] = blockIdx.x;
        }
#endif
    }
}

// Retry list of k_knn_tile: one wave per query (knn_retry_wave).
// One wavefront per workgroup.  (knn_retry_wave is inlined: as a call it took the grid
// parameters by reference to the caller's local copy, which then lived in scratch --
// global-memory round trips on every cell index.)
template <int K>
__global__ __launch_bounds__(64) void k_knn_retry(const KnnGrid* __restrict__ gp, double r2max,
                                                   const double* __restrict__ nodes,
                                                   const double* __restrict__ sxyz,
                                                   const int* __restrict__ sidx,
                                                   const int* __restrict__ start,
                                                   const int* __restrict__ retry,
                                                   const double* __restrict__ retry_b,
                                                   int32_t* __restrict__ nbr) {
    const KnnGrid g = *gp;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const int nq = min(g.nretry, start[g.ncell]);  // (the list holds at most one entry per node)
    for (int i = wave; i < nq; i += nwaves) {  // wave-uniform
#ifdef EPP_KNN_DIAG
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
#endif
        knn_retry_wave<K>(g, r2max, nodes, sxyz, sidx, start, retry[i], retry_b[i], nbr);
#ifdef EPP_KNN_DIAG
        // (diagnostics builds) per retried query: start, end (10 ns ticks), bound, node
        if ((threadIdx.x & 63) == 0 && i < kKnnRetryTl) {
            g_knn_retry_tl[i][0] = t0;
            g_knn_retry_tl[i][1] = __builtin_amdgcn_s_memrealtime();
            g_knn_retry_tl[i][2] = (unsigned long long)__double_as_longlong(retry_b[i]);
            g_knn_retry_tl[i][3] = (unsigned long long)retry[i];
        }
#endif
    }
}

// ---- wave-per-query grid k-NN (k_knn_wave) ---------------------------------------------
// The same 4^3-cell blocks, 2-cell halos and block queue as k_knn_tile, but the halo's
// exact coordinates sit in LDS (SoA doubles) and one wavefront takes one query at a time:
//   1. the query's 5^3-cell cube is five z-slabs; each slab's five y-rows are one
//      contiguous LDS range (rows ly-2..ly+2 of the halo, x cells outside lx-2..lx+2
//      filtered by the halo x index kept with the node id).  The ranges are concatenated
//      and spread over the lanes, up to kWaveSlots candidates per lane, every lane doing
//      the same work (no per-query loop lengths, no divergence);
//   2. exact squared distance per candidate (the oracle's (dx dx + dy dy) + dz dz), and a
//      key: one of 128 linear bins of d over [0, 8 h^2) (monotone in d: every candidate at or below
//      the K-th distance has a key at or below the K-th one's);
//   3. the smallest cut with >= K keys at or below it, by bisection over the bins on
//      wave ballots (no histogram, no atomics);
//   4. the candidates at or below the cut (K plus a fraction of a bin, on average) go to a
//      per-wave LDS list; each listed entry's rank in (distance, index) order is counted
//      against the list: ranks < K are the answer, the rank K-1 entry the K-th distance for
//      the stopping rule after shell kTileH (knn_done).
// A query whose cube holds more than 64 kWaveSlots positions or whose list exceeds
// kWaveList, or that fails the stopping rule, goes to the retry list (k_knn_retry), as in
// k_knn_tile.  k_knn_tile's lanes-per-query scheme runs ~375 wave-instructions per query
// and waits on long dependent LDS chains of its busiest lane (SQ_WAIT_ANY ~66 % of its
// wave cycles); here a query is ~10 short LDS round trips and a fixed instruction count.
constexpr int kWaveThreads = 512;                // = kTileCells: one halo cell per thread
constexpr int kWaveCap = 1344;                   // halo candidates (else the block's queries retry)
constexpr int kWaveSlots = 6;                    // candidate slots per lane: 384 cube positions (~278 at 1.5 nodes per cell)
constexpr int kWaveList = 64;                    // listed candidates per query (else retry)
constexpr int kWaveBins = 128;                   // distance keys: linear bins over [0, 8 h^2)
static_assert(kTileCells == kWaveThreads, "one halo cell per thread");

template <int K>
__global__ __launch_bounds__(kWaveThreads, 6) void k_knn_wave(KnnGrid* __restrict__ gp, double r2max,
                                                              const double* __restrict__ sxyz,
                                                              const int* __restrict__ sidx,
                                                              const int* __restrict__ start,
                                                              int* __restrict__ retry, double* __restrict__ retry_b,
                                                              int32_t* __restrict__ nbr,
                                                              unsigned long long* __restrict__ dbg) {
    static_assert(K <= kWaveList && K <= 64, "");
    constexpr int kWaves = kWaveThreads / 64;
    __shared__ double hxv[kWaveCap], hyv[kWaveCap], hzv[kWaveCap];  // exact coordinates
    __shared__ int hid[kWaveCap];                                   // node id | halo x index << 29
    __shared__ uint32_t qh[kWaveCap];  // the block's queries: LDS position | halo x, y, z << 11, 14, 17
    __shared__ int cst[kTileCells + 1];                              // halo cell -> LDS offset
    __shared__ double ld[kWaves][kWaveList];                         // per-wave list: distances
    __shared__ int lj[kWaves][kWaveList];                            //                node ids
    __shared__ int wsum[kWaves];
    __shared__ int s_nq, s_b;
    __shared__ KnnGrid s_g;
    if (threadIdx.x == 0) s_g = *gp;  // (visible after the loop's first barrier)
    // (the grid parameters are read where they are used -- from gp or the LDS copy -- not
    // held in registers through the query loop: the scalar register file is this kernel's
    // tight resource)
    const int dims0 = gp->dims[0], dims1 = gp->dims[1], dims2 = gp->dims[2];
    const int nbx = (dims0 + kTileB - 1) / kTileB, nby = (dims1 + kTileB - 1) / kTileB,
              nbz = (dims2 + kTileB - 1) / kTileB;
    const int nblocks = nbx * nby * nbz;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double inv_w = (double)kWaveBins / (8.0 * gp->h * gp->h);  // bins per unit of squared distance
    const int t = threadIdx.x;
    const int hx = t % kTileE, hy = (t / kTileE) % kTileE, hz = t / (kTileE * kTileE);  // this thread's halo cell
    for (;;) {
        if (t == 0) s_b = atomicAdd(&gp->next, 1);
        __syncthreads();
        const int b = s_b;  // block-uniform
        if (b >= nblocks) break;
        const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
        const int ox = bx * kTileB - kTileH, oy = by * kTileB - kTileH, oz = bz * kTileB - kTileH;
#ifdef EPP_KNN_DIAG
        // phase timeline (diagnostics builds; scripts/knn_timeline.py): begin, halo scanned,
        // halo copied, wave 0's first query done, wave 0's queries done, (same), all waves
        // done, end; wave 0's query count and s_memtime cycles in its query loop
        unsigned long long tl[8] = {__builtin_amdgcn_s_memrealtime(), 0, 0, 0, 0, 0, 0, 0};
        unsigned long long cyc0 = 0, nq0 = 0;
#endif
        // 1. halo cell sizes -> exclusive scan
        const int x = ox + hx, y = oy + hy, z = oz + hz;
        const bool in = x >= 0 && x < dims0 && y >= 0 && y < dims1 && z >= 0 && z < dims2;
        const int cell = in ? (z * dims1 + y) * dims0 + x : 0;
        const int s0 = start[cell];
        const int cnt = in ? start[cell + 1] - s0 : 0;
        int incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wv] = incl;
        if (t == 0) s_nq = 0;
        __syncthreads();
        int base = incl - cnt, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            base += w < wv ? wsum[w] : 0;
            total += wsum[w];
        }
        cst[t] = base;
        if (t == 0) cst[kTileCells] = total;
#ifdef EPP_KNN_DIAG
        tl[1] = __builtin_amdgcn_s_memrealtime();
#endif
        if (total <= kWaveCap) {  // block-uniform
            // 2. copy the halo's nodes; list the block's own as queries
            const bool inner = hx >= kTileH && hx < kTileH + kTileB && hy >= kTileH && hy < kTileH + kTileB &&
                               hz >= kTileH && hz < kTileH + kTileB;
            const int q0 = (inner && cnt) ? atomicAdd(&s_nq, cnt) : 0;
            for (int q = 0; q < cnt; ++q) {
                const int sg = s0 + q, pos = base + q;
                hxv[pos] = sxyz[3 * (int64_t)sg];
                hyv[pos] = sxyz[3 * (int64_t)sg + 1];
                hzv[pos] = sxyz[3 * (int64_t)sg + 2];
                hid[pos] = sidx[sg] | (hx << 29);
                if (inner) qh[q0 + q] = (uint32_t)pos | ((uint32_t)hx << 11) | ((uint32_t)hy << 14) | ((uint32_t)hz << 17);
            }
            __syncthreads();
            const int nq = s_nq;
#ifdef EPP_KNN_DIAG
            tl[2] = __builtin_amdgcn_s_memrealtime();
            cyc0 = __builtin_amdgcn_s_memtime();
#endif
            // 3. one query per wave at a time
            for (int qi = wv; qi < nq; qi += kWaves) {  // wave-uniform
                // (the query's values are wave-uniform: moved to scalar registers, which
                // keeps the vector file for the candidate slots)
                const uint32_t qv = (uint32_t)__builtin_amdgcn_readfirstlane((int)qh[qi]);
                const int me = (int)(qv & 2047u);
                const int lx = (int)((qv >> 11) & 7u), ly = (int)((qv >> 14) & 7u), lz = (int)((qv >> 17) & 7u);
                auto uni = [](double v) {
                    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
                };
                const double px = uni(hxv[me]), py = uni(hyv[me]), pz = uni(hzv[me]);
                const int self = __builtin_amdgcn_readfirstlane(hid[me]) & 0x1fffffff;
                double bnd;  // the stopping rule's bound after shell kTileH (knn_bound)
                {
                    const KnnGrid g = s_g;  // (LDS: a global load here would wait out an L2 round trip per query)
                    const int c[3] = {ox + lx, oy + ly, oz + lz};
                    const double p[3] = {px, py, pz};
                    bnd = knn_bound(g, c, p, kTileH);
                }
                // the five slab ranges [A_d, B_d): lanes 0-4 read A, lanes 5-9 read B
                int rv = 0;
                if (lane < 10) {
                    const int d = lane < 5 ? lane : lane - 5;
                    const int row = (lz - kTileH + d) * kTileE + (lane < 5 ? ly - kTileH : ly + kTileH);
                    rv = cst[row * kTileE + (lane < 5 ? lx - kTileH : lx + kTileH + 1)];
                }
                int A[5], P[6];
                P[0] = 0;
#pragma unroll
                for (int d = 0; d < 5; ++d) {
                    A[d] = __builtin_amdgcn_readlane(rv, d);
                    P[d + 1] = P[d] + (__builtin_amdgcn_readlane(rv, 5 + d) - A[d]);
                }
                const int T = P[5];  // positions in the five ranges
                int gap[5];          // v -> LDS position: v + A_0 + the gaps between ranges behind v
#pragma unroll
                for (int d = 1; d < 5; ++d) gap[d] = A[d] - (A[d - 1] + (P[d] - P[d - 1]));
                bool done = false;
                double dk = r2max;  // the K-th distance (r2max: fewer than K candidates)
                if (T <= kWaveSlots * 64) {  // wave-uniform
                    // per slot: the exact distance and (key << 11 | LDS position); key
                    // kWaveBins: no candidate
                    double dv[kWaveSlots];
                    uint32_t kp[kWaveSlots];
#pragma unroll
                    for (int s = 0; s < kWaveSlots; ++s) {
                        kp[s] = (uint32_t)kWaveBins << 11;
                        dv[s] = 0.0;
                        if (s * 64 < T) {  // wave-uniform
                            const int v = s * 64 + lane;
                            int pos = A[0] + v;
#pragma unroll
                            for (int d = 1; d < 5; ++d) pos += v >= P[d] ? gap[d] : 0;
                            const bool ok = v < T;
                            const int pc = ok ? pos : me;
                            const double dx = hxv[pc] - px, dy = hyv[pc] - py, dz = hzv[pc] - pz;
                            const double dd = (dx * dx + dy * dy) + dz * dz;
                            const uint32_t cx = ((uint32_t)hid[pc] >> 29) - (uint32_t)(lx - kTileH);  // x cell in the cube?
                            const bool el = ok & (pc != me) & (cx <= 4u) & (dd <= r2max);
                            const double kd = dd * inv_w;
                            const uint32_t key = el ? (kd < (double)(kWaveBins - 1) ? (uint32_t)kd : kWaveBins - 1u) : kWaveBins;
                            kp[s] = (key << 11) | (uint32_t)pc;
                            dv[s] = dd;
                        }
                    }
                    auto count_le = [&](int c) {  // candidates with key <= c
                        const uint32_t lim = (uint32_t)(c + 1) << 11;
                        int n = 0;
#pragma unroll
                        for (int s = 0; s < kWaveSlots; ++s) n += (int)__popcll(__ballot(kp[s] < lim));  // (unused slots: never)
                        return n;
                    };
                    // the smallest cut with >= K keys at or below it (all candidates when
                    // fewer than K)
                    int lo = 0, hi = kWaveBins - 1;
                    if (count_le(hi) >= K) {
                        while (lo < hi) {  // wave-uniform
                            const int mid = (lo + hi) >> 1;
                            if (count_le(mid) >= K) hi = mid;
                            else lo = mid + 1;
                        }
                    }
                    const uint32_t lim = (uint32_t)(hi + 1) << 11;
                    int m = 0;
#pragma unroll
                    for (int s = 0; s < kWaveSlots; ++s) {
                        const bool li = kp[s] < lim;
                        const unsigned long long bl = __ballot(li);
                        const int at = m + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bl >> 32),
                                                                          __builtin_amdgcn_mbcnt_lo((uint32_t)bl, 0u));
                        if (li && at < kWaveList) {
                            ld[wv][at] = dv[s];
                            lj[wv][at] = hid[kp[s] & 2047u] & 0x1fffffff;
                        }
                        m += (int)__popcll(bl);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the list is written
                    if (m <= kWaveList) {  // wave-uniform
                        const bool mine = lane < m;
                        const double di = mine ? ld[wv][lane] : 0.0;
                        const int ji = mine ? lj[wv][lane] : 0;
                        // entry f (on lane f) against every lane's own: v_readlane into scalar
                        // registers, no memory round trip per entry
                        const int dlo = __double2loint(di), dhi = __double2hiint(di);
                        int rank = 0;
                        for (int f = 0; f < m; ++f) {  // wave-uniform
                            const double df = __hiloint2double(__builtin_amdgcn_readlane(dhi, f),
                                                               __builtin_amdgcn_readlane(dlo, f));
                            const int jf = __builtin_amdgcn_readlane(ji, f);
                            rank += ((df < di) | ((df == di) & (jf < ji))) ? 1 : 0;
                        }
                        if (m >= K) {
                            const unsigned long long bk = __ballot(mine && rank == K - 1);
                            dk = __shfl(di, bk ? (int)__builtin_ctzll(bk) : 0, 64);  // (one lane: ranks are distinct)
                        }
                        done = bnd == INFINITY || dk < bnd;
                        if (done) {
                            if (mine && rank < K) nbr[(int64_t)self * K + rank] = ji;
                            if (lane >= m && lane < K) nbr[(int64_t)self * K + lane] = -1;  // (fewer than K)
                        } else if (lane == 0) {
                            atomicAdd(&gp->why[2], 1);
                        }
                    } else {
                        dk = INFINITY;  // (list over capacity: the retry walks shells)
                        if (lane == 0) atomicAdd(&gp->why[0], 1);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the list is rewritten next
                } else {
                    dk = INFINITY;
                    if (lane == 0) atomicAdd(&gp->why[0], 1);
                }
                if (!done && lane == 0) {
                    const int at = atomicAdd(&gp->nretry, 1);
                    retry[at] = self;
                    retry_b[at] = dk;
                }
#ifdef EPP_KNN_DIAG
                if (tl[3] == 0ull) tl[3] = __builtin_amdgcn_s_memrealtime();
                ++nq0;
#endif
            }
#ifdef EPP_KNN_DIAG
            tl[4] = tl[5] = __builtin_amdgcn_s_memrealtime();
            cyc0 = __builtin_amdgcn_s_memtime() - cyc0;
#endif
        } else {
            // crowded halo: the block's own nodes retry from global memory
            const bool inner = hx >= kTileH && hx < kTileH + kTileB && hy >= kTileH && hy < kTileH + kTileB &&
                               hz >= kTileH && hz < kTileH + kTileB;
            if (inner && cnt) {
                const int at = atomicAdd(&gp->nretry, cnt);
                for (int q = 0; q < cnt; ++q) {
                    retry[at + q] = sidx[s0 + q];
                    retry_b[at + q] = INFINITY;
                }
                atomicAdd(&gp->why[3], cnt);
            }
        }
        __syncthreads();  // the LDS tile is rewritten by the next block
#ifdef EPP_KNN_DIAG
        if (dbg && threadIdx.x == 0 && b < kKnnTlBlocks) {
            tl[6] = tl[7] = __builtin_amdgcn_s_memrealtime();
            for (int q = 0; q < 8; ++q) dbg[16 * b + q] = tl[q];
            dbg[16 * b + 8] = (unsigned long long)s_nq;
            dbg[16 * b + 9] = (unsigned long long)total;
            dbg[16 * b + 10] = blockIdx.x;
            dbg[16 * b + 11] = nq0;
            dbg[16 * b + 12] = cyc0;
        }
#endif
    }
}

#ifdef EPP_KNN_DIAG
// the k_knn_tile phase timeline (diagnostics builds): 16 u64 per block, see the kernel
unsigned long long* knn_tl_buffer() {
    static unsigned long long* buf = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        if (hipMalloc(&buf, (size_t)16 * 8 * kKnnTlBlocks) != hipSuccess) buf = nullptr;
    });
    return buf;
}
#endif

// k_knn_retry<k> (k = 4, 8 or 16) over the retry list, one wave per retried query: kRetryPerCu
// per CU (waves without a query exit at once; more retries than waves loop)
constexpr int kRetryPerCu = 8;
void knn_retry_launch(int k, int cus, hipStream_t s, const KnnGrid* g, double r2, const double* nodes,
                      const double* sxyz, const int* sidx, const int* start, const int* retry, const double* retry_b,
                      int32_t* nbr) {
    const dim3 gr((unsigned)std::max(1, cus * kRetryPerCu)), br(64);
    if (k == 4) hipLaunchKernelGGL(k_knn_retry<4>, gr, br, 0, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr);
    else if (k == 8) hipLaunchKernelGGL(k_knn_retry<8>, gr, br, 0, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr);
    else hipLaunchKernelGGL(k_knn_retry<16>, gr, br, 0, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr);
}

epp_status knn_grid_launch(const double* nodes, int n, int k, double max_dist, int32_t* nbr, char* buf,
                           const KnnLayout& L, hipStream_t s, const double* box_lo = nullptr,
                           const double* box_hi = nullptr) {
    KnnGrid* g = reinterpret_cast<KnnGrid*>(buf);
    int* cell_of = reinterpret_cast<int*>(buf + L.cell);
    int* sidx = reinterpret_cast<int*>(buf + L.sidx);
    double* sxyz = reinterpret_cast<double*>(buf + L.sxyz);
    int* cnt = reinterpret_cast<int*>(buf + L.cnt);
    int* start = reinterpret_cast<int*>(buf + L.start);
    int* fill = reinterpret_cast<int*>(buf + L.fill);
    const double r2 = max_dist > 0 ? max_dist * max_dist : 1e300;
    const dim3 g256((n + 255) / 256), b256(256);
    const int nb = std::max(1, std::min(kBoundsBlocks, (n + kBoundsThreads - 1) / kBoundsThreads));
#ifdef EPP_KNN_DIAG
    // (diagnostics builds only) EPP_KNN_NPC: the grid density, an exact-either-way A/B knob
    const char* npc_env = std::getenv("EPP_KNN_NPC");
    const double npc = npc_env && *npc_env ? std::max(0.5, std::atof(npc_env)) : kNodesPerCell;
#else
    const double npc = kNodesPerCell;
#endif
    // cnt, fill and the scan's status words are adjacent: cleared together by the first
    // kernel (never run the scatter on stale counters, never let the look-back take a stale
    // word for a published one)
    const int nclr = (int)((L.start - L.cnt) / sizeof(int));
    if (box_lo && box_hi) {  // the caller's box: the grid shape on the host, one kernel
        KnnGrid gv{};
        const double mn[3] = {box_lo[0], box_lo[1], box_lo[2]}, mx[3] = {box_hi[0], box_hi[1], box_hi[2]};
        knn_grid_shape(mn, mx, n, L.cap, npc, &gv);
        hipLaunchKernelGGL(k_knn_prep, dim3(nb), dim3(kBoundsThreads), 0, s, gv, g, cnt, nclr);
    } else {
        double* part = reinterpret_cast<double*>(buf + L.part);
        hipLaunchKernelGGL(k_knn_bounds_part, dim3(nb), dim3(kBoundsThreads), 0, s, nodes, n, part, cnt, nclr);
        hipLaunchKernelGGL(k_knn_setup, dim3(1), dim3(64), 0, s, part, nb, n, L.cap, npc, g);
    }
    hipLaunchKernelGGL(k_knn_count, g256, b256, 0, s, nodes, n, g, cell_of, cnt);
    hipLaunchKernelGGL(k_knn_scan, dim3(L.scan_blocks), dim3(kScanThreads), 0, s, g, cnt, start,
                       reinterpret_cast<unsigned long long*>(buf + L.stat), next_scan_tag());
    hipLaunchKernelGGL(k_knn_scatter, g256, b256, 0, s, nodes, n, cell_of, start, fill, sxyz, sidx);
    // EPP_KNN_TILE=0 selects the untiled grid walk, 2 the wave-per-query k_knn_wave (same
    // answers; test hooks); the default is k_knn_tile.  The timing ablations and the
    // per-block dump exist only in a -DEPP_KNN_DIAG diagnostics build.  (A one-query-per-
    // lane variant that keeps the exact
    // top-K in registers straight out of an LDS copy of the halo was tried: 425 us per
    // 63k-node table against k_knn_tile's 134 us -- the sorted insert then runs for nearly
    // every candidate of every lane.)
    const char* tile_env = std::getenv("EPP_KNN_TILE");
    const int tile_sel = tile_env && *tile_env ? std::atoi(tile_env) : kKnnDefaultTile;
    const bool tiled = tile_sel != 0;
    int* const retry = cell_of;  // free once the scatter has run
    double* const retry_b = reinterpret_cast<double*>(buf + L.rbnd);
    // (node ids share a word with the halo x index in k_knn_wave: below 2^29)
    if (tile_sel == 2 && (k == 4 || k == 8 || k == 16) && n < (1 << 29)) {
        const int cus = cu_count_planner();
        const dim3 gw((unsigned)std::max(1, cus * 3)), bw(kWaveThreads);  // (LDS: three workgroups per CU)
#ifdef EPP_KNN_DIAG
        unsigned long long* d = knn_tl_buffer();
        if (d) (void)hipMemsetAsync(d, 0, (size_t)16 * 8 * kKnnTlBlocks, s);
#else
        unsigned long long* d = nullptr;
#endif
        if (k == 4) hipLaunchKernelGGL(k_knn_wave<4>, gw, bw, 0, s, g, r2, sxyz, sidx, start, retry, retry_b, nbr, d);
        else if (k == 8) hipLaunchKernelGGL(k_knn_wave<8>, gw, bw, 0, s, g, r2, sxyz, sidx, start, retry, retry_b, nbr, d);
        else hipLaunchKernelGGL(k_knn_wave<16>, gw, bw, 0, s, g, r2, sxyz, sidx, start, retry, retry_b, nbr, d);
        knn_retry_launch(k, cus, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr);
    } else if (tiled && (k == 4 || k == 8 || k == 16)) {
        // persistent: the block count is only known on the device (grid shape)
        const int cus = cu_count_planner();
        const dim3 gt((unsigned)std::max(1, cus * 3)), bt(kTileThreads);  // (LDS: three workgroups per CU)
#ifdef EPP_KNN_DIAG
        const int mode = tile_env ? std::atoi(tile_env) : 1;  // 4: timing ablation (inexact)
        unsigned long long* d = knn_tl_buffer();
        if (d) (void)hipMemsetAsync(d, 0, (size_t)16 * 8 * kKnnTlBlocks, s);
#else
        const int mode = 1;
        unsigned long long* d = nullptr;
#endif
        if (k == 4) hipLaunchKernelGGL(k_knn_tile<4>, gt, bt, 0, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr, mode, d);
        else if (k == 8) hipLaunchKernelGGL(k_knn_tile<8>, gt, bt, 0, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr, mode, d);
        else hipLaunchKernelGGL(k_knn_tile<16>, gt, bt, 0, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr, mode, d);
        knn_retry_launch(k, cus, s, g, r2, nodes, sxyz, sidx, start, retry, retry_b, nbr);
    } else {
        switch (k) {
            case 4: hipLaunchKernelGGL(k_knn_grid<4>, g256, b256, 0, s, g, n, r2, sxyz, sidx, start, nbr); break;
            case 8: hipLaunchKernelGGL(k_knn_grid<8>, g256, b256, 0, s, g, n, r2, sxyz, sidx, start, nbr); break;
            case 16: hipLaunchKernelGGL(k_knn_grid<16>, g256, b256, 0, s, g, n, r2, sxyz, sidx, start, nbr); break;
            default: hipLaunchKernelGGL(k_knn_grid<32>, g256, b256, 0, s, g, n, r2, sxyz, sidx, start, nbr); break;
        }
    }
    return last("epp_knn_grid");
}

CachedWs g_knn_ws[64];

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_knn_bruteforce(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr,
                              void* stream) {
    if (n < 0 || (n > 0 && (!nodes || !nbr)) || (k != 4 && k != 8 && k != 16 && k != 32)) {
        set_error("epp_knn: invalid argument (k must be 4, 8, 16 or 32)");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    const double r2 = max_dist > 0 ? max_dist * max_dist : 1e300;
    const dim3 grid((n + kKnnBlock - 1) / kKnnBlock), block(kKnnBlock);
    hipStream_t s = (hipStream_t)stream;
    switch (k) {
        case 4: hipLaunchKernelGGL(k_knn<4>, grid, block, 0, s, nodes, n, r2, nbr); break;
        case 8: hipLaunchKernelGGL(k_knn<8>, grid, block, 0, s, nodes, n, r2, nbr); break;
        case 16: hipLaunchKernelGGL(k_knn<16>, grid, block, 0, s, nodes, n, r2, nbr); break;
        default: hipLaunchKernelGGL(k_knn<32>, grid, block, 0, s, nodes, n, r2, nbr); break;
    }
    return last("epp_knn_bruteforce");
}

epp_status epp_knn(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* stream) {
    // the grid pays off from a few thousand nodes; both give the same answer
    // (EPP_KNN_IMPL=1 / 2 forces all-pairs / grid: diagnostics)
    const char* f = std::getenv("EPP_KNN_IMPL");
    const int impl = f && *f ? std::atoi(f) : 0;
    const bool brute = impl == 1 || (impl == 0 && n <= 2048);
    return brute ? epp_knn_bruteforce(nodes, n, k, max_dist, nbr, stream)
                 : epp_knn_grid(nodes, n, k, max_dist, nbr, stream);
}

uint64_t epp_knn_workspace_size(int32_t n) { return n <= 0 ? 0 : (uint64_t)knn_layout(n).bytes; }

#ifdef EPP_KNN_DIAG
// (diagnostics builds only) the last k_knn_tile launch's phase timeline: 16 u64 per block
epp_status epp_dbg_knn_tl(unsigned long long* out, int64_t blocks) {
    unsigned long long* d = knn_tl_buffer();
    if (!d || blocks > kKnnTlBlocks) return EPP_ERR_RUNTIME;
    return hipMemcpy(out, d, (size_t)blocks * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess ? EPP_OK : EPP_ERR_HIP;
}
// (diagnostics builds only) the last k_knn_retry launch: per retried query start, end,
// bound (f64 bits), node -- 4 u64 each
epp_status epp_dbg_knn_retry_tl(unsigned long long* out, int64_t n) {
    if (n > kKnnRetryTl) n = kKnnRetryTl;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_knn_retry_tl), (size_t)n * 32) == hipSuccess ? EPP_OK : EPP_ERR_HIP;
}
#endif

epp_status epp_knn_ws(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* ws,
                      uint64_t ws_bytes, void* stream) {
    if (n > 2048) return epp_knn_grid_ws(nodes, n, k, max_dist, nbr, ws, ws_bytes, stream);
    return epp_knn_bruteforce(nodes, n, k, max_dist, nbr, stream);
}

epp_status epp_knn_grid_ws_box(const double* nodes, int32_t n, int32_t k, double max_dist, const double lo[3],
                               const double hi[3], int32_t* nbr, void* ws, uint64_t ws_bytes, void* stream) {
    if (n < 0 || (n > 0 && (!nodes || !nbr)) || (k != 4 && k != 8 && k != 16 && k != 32) || !lo || !hi ||
        !(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) {
        set_error("epp_knn_grid_ws_box: invalid argument (k must be 4, 8, 16 or 32; lo <= hi)");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    const KnnLayout L = knn_layout(n);
    if (!ws || ws_bytes < L.bytes || (reinterpret_cast<uintptr_t>(ws) & 255)) {
        set_error("epp_knn_grid_ws_box: workspace missing, unaligned or smaller than epp_knn_workspace_size(n)");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    return knn_grid_launch(nodes, n, k, max_dist, nbr, static_cast<char*>(ws), L, (hipStream_t)stream, lo, hi);
}

epp_status epp_knn_ws_box(const double* nodes, int32_t n, int32_t k, double max_dist, const double lo[3],
                          const double hi[3], int32_t* nbr, void* ws, uint64_t ws_bytes, void* stream) {
    if (n > 2048) return epp_knn_grid_ws_box(nodes, n, k, max_dist, lo, hi, nbr, ws, ws_bytes, stream);
    return epp_knn_bruteforce(nodes, n, k, max_dist, nbr, stream);
}

epp_status epp_knn_grid_ws(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* ws,
                           uint64_t ws_bytes, void* stream) {
    if (n < 0 || (n > 0 && (!nodes || !nbr)) || (k != 4 && k != 8 && k != 16 && k != 32)) {
        set_error("epp_knn_grid: invalid argument (k must be 4, 8, 16 or 32)");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    const KnnLayout L = knn_layout(n);
    if (!ws || ws_bytes < L.bytes || (reinterpret_cast<uintptr_t>(ws) & 255)) {
        set_error("epp_knn_grid: workspace missing, unaligned or smaller than epp_knn_workspace_size(n)");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    return knn_grid_launch(nodes, n, k, max_dist, nbr, static_cast<char*>(ws), L, (hipStream_t)stream);
}

// Without a caller workspace: one cached workspace per device.  Reuse is ordered on the
// GPU (the next user's stream waits for the previous user's completion event), growth
// frees the old buffer only after the device drained it (hipFree synchronises).
epp_status epp_knn_grid(const double* nodes, int32_t n, int32_t k, double max_dist, int32_t* nbr, void* stream) {
    if (n < 0 || (n > 0 && (!nodes || !nbr)) || (k != 4 && k != 8 && k != 16 && k != 32)) {
        set_error("epp_knn_grid: invalid argument (k must be 4, 8, 16 or 32)");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    CachedWs& c = g_knn_ws[dev & 63];
    std::lock_guard<std::mutex> lk(c.mu);
    hipStream_t s = (hipStream_t)stream;
    const KnnLayout L = knn_layout(n);
    hipError_t e = hipSuccess;
    e = c.acquire(s, L.bytes);
    if (e != hipSuccess) {
        set_error(std::string("epp_knn_grid: workspace: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    const epp_status rc = knn_grid_launch(nodes, n, k, max_dist, nbr, static_cast<char*>(c.buf), L, s);
    c.release(s);
    return rc;
}

}  // extern "C"
