// knn_tile.hip — the tile pass of the default exact k-NN (knn_kernels.h): k_knn_tile, a
// workgroup per 4^3-cell block of the grid with the block's halo in LDS.  The queries it cannot
// settle go to the retry list (knn_retry.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "knn_diag.h"
#include "knn_kernels.h"

namespace epp {
namespace {

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
__device__ __forceinline__ float tile_d(const TileCand c, const TileCand& pf) {
    const float dx = c.x - pf.x, dy = c.y - pf.y, dz = c.z - pf.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ int tile_spos(const TileCand& c) { return __float_as_int(c.w); }  // (sorted position)

// Visits the candidates of cube rows row0, row0 + rstep, ... around a query (a row =
// kTileW consecutive halo cells along x, one contiguous LDS range), four candidates at a
// time so their LDS reads are in flight together.  f(q, d_float, spos, valid), spos = the
// candidate's sorted position (what the self test compares).
template <class F>
__device__ __forceinline__ void tile_rows(const int* cst, const TileCand* cand, int h0, int row0, int rstep,
                                          const TileCand& pf, F&& f) {
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
                f(qq, tile_d(c[u], pf), tile_spos(c[u]), q + u < q1);
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
                                               const TileCand& pf, const double (&fr)[3], double h, double thr,
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
                f(qq, tile_d(c[u], pf), tile_spos(c[u]), q + u < q1);
            }
        }
    }
}
static_assert(kTileW == 5 && kTileH == 2, "tile_rows_near trims rows of 5 cells");

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
                                                           int32_t* __restrict__ nbr,
                                                           unsigned long long* __restrict__ dbg) {
    __shared__ TileCand cand[kTileCap];                    // x, y, z (block-centre relative), sorted position
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
    for (;;) {
        if (threadIdx.x == 0) s_b = atomicAdd(&gp->next, 1);
        __syncthreads();
        const int b = s_b;  // block-uniform
        if (b >= nblocks) break;
        const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
        const int ox = bx * kTileB - kTileH, oy = by * kTileB - kTileH, oz = bz * kTileB - kTileH;
        const double cen[3] = {g.lo[0] + (ox + 0.5 * kTileE) * g.h, g.lo[1] + (oy + 0.5 * kTileE) * g.h,
                               g.lo[2] + (oz + 0.5 * kTileE) * g.h};
        EPP_KTL_BEGIN;  // (the phase timeline of a diagnostics build, knn_diag.h)
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
            const int nq_all = s_nq;
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
                    retry[at] = sidx[tile_spos(cand[qh[q]])];
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
                const TileCand pf = cand[me];
                const int sself = tile_spos(cand[me]);  // the query's sorted position
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
                        if (valid && j != sself && kb < kTileNB) atomicAdd(&hist[kb >> 1][slot], 1u << ((kb & 1) << 4));
                    };
                    if (live) {
                        if (full) tile_rows(cst, cand, h0, sub, lpq, pf, bin);
                        else tile_rows_near(cst, cand, h0, sub, lpq, pf, fr, g.h, kPass1R2 * g.h * g.h, bin);
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
                    tile_rows_near(cst, cand, h0, sub, lpq, pf, fr, g.h, thr2, [&](int q, float d, int j, bool valid) {
                        if (valid && j != sself && d < dlist) {
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
                const int sx = tile_spos(cand[qh[qx]]);
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
                        bi[k] = kKnnNone;
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
                            const int sg0 = tile_spos(cand[q]);
                            const bool sok = sg0 >= 0 && sg0 < n_nodes;
                            EPP_KNN_ASSERT(qok && sok);
                            guard_ok = guard_ok && qok && sok;
                            const int sg = sok ? sg0 : 0;
                            jj[u] = sidx[sg];
                            const double ddx = sxyz[3 * (int64_t)sg] - p[0], ddy = sxyz[3 * (int64_t)sg + 1] - p[1],
                                         ddz = sxyz[3 * (int64_t)sg + 2] - p[2];
                            dd[u] = (ddx * ddx + ddy * ddy) + ddz * ddz;
                        }
#pragma unroll
                        for (int u = 0; u < kLoads; ++u)
                            if (i0 + u < nl) knn_insert<K>(bd, bi, dd[u], jj[u]);
                    }
                    // exact when the K-th distance is within the listed range and the cube
                    // suffices (stopping rule after shell kTileH)
                    const bool in_range = bd[K - 1] <= dcut;
                    ok = guard_ok && in_range && knn_done<K>(g, c, p, kTileH, bd);
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
                EPP_KTL(5);
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
        EPP_KTL_RECORD(dbg, b, s_nq, total);
    }
}

}  // namespace

void knn_tile_launch(int k, int cus, const double* nodes, double r2, const KnnWs& w, int32_t* nbr, hipStream_t s) {
    // persistent: the block count is only known on the device (grid shape)
    const dim3 gt((unsigned)std::max(1, cus * 3)), bt(kTileThreads);  // (LDS: three workgroups per CU)
    unsigned long long* d = knn_tl_begin(s);  // (null but in a diagnostics build)
    knn_for_k<false>(k, [&](auto K) {
        hipLaunchKernelGGL(k_knn_tile<K.value>, gt, bt, 0, s, w.g, r2, nodes, w.sxyz, w.sidx, w.start, w.retry,
                           w.retry_b, nbr, d);
    });
}

}  // namespace epp
