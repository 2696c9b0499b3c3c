// plan_batch.hip — the batched planner's device side: one launch per stage for all of a
// batch's problems (host_planner.cpp drives it through plan_batch_layout / plan_batch_launch,
// epp_internal.h):
//
//   k_pb_sample      : every problem's samples, its cleared status words and its k-NN grid shape
//   k_pb_compact     : nodes = start, goal, the valid samples in order; grid membership, queries
//   k_pb_knn_scan / k_pb_knn_scatter : the problem's grid (knn_grid.h) over its member nodes
//   k_pb_rows        : the exact k-NN row of every listed query, one wave each
//   k_pb_number      : the referenced nodes numbered in node order
//   k_pb_emit        : the results into pinned host memory + the completion slots
//
// The state and motion checks between them are the collision kernels (states_kernels.h,
// motions_kernels.h).  EPP_PB_TRACE=1 times the stages; a -DEPP_PB_ROWS_TL build records
// k_pb_rows' per-query timeline (scripts/pb_rows_timeline.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "completion.h"
#include "epp_internal.h"
#include "knn_grid.h"

namespace epp {
namespace {

// ---- the batched planner: one launch per stage for all of a batch's problems ----------
// (epp_internal.h, PlanBatchLayout).  Problem p = blockIdx.y of the per-problem stages; its
// samples at xyz + p ns, its nodes at nodes + p NS (NS = 2^ns_log >= 65536: a node's id in
// its problem is the low bits of its global id p NS + node), its k-NN grid workspace at
// kws + p kws_stride (KnnLayout for ns + 2 nodes), its queries at query + row_off.  Node
// counts stay on the device.
constexpr int kPbSegSmall = 16;  // batches of up to this many problems: no upload (k_pb_sample)
struct PlanBatchDev {
    const PlanSeg* seg;
    const PlanSeg* seg_h;         // (<= kPbSegSmall problems) the pinned host copy, else null
    uint64_t seeds[kPbSegSmall];  // (<= kPbSegSmall problems) their seeds and capacities
    int32_t caps[kPbSegSmall];
    int S, k, ns_log, nbc, cap_total, nctr;
    int64_t ns, NS;
    double lo[3], hi[3];
    double* xyz;
    uint8_t* valid;
    double* nodes;
    unsigned long long* cstat;
    unsigned long long* nstat;  // k_pb_number's look-back status words: NS / 1024 per problem
    unsigned long long* ctr;
    char* kws;
    size_t kws_stride, l_cell, l_sidx, l_sxyz, l_cnt, l_start, l_fill, l_stat;
    int l_cap, nclr;
    int32_t* query;     // per problem (at row_off): its listed nodes (node ids)
    int32_t* ids32;     // row -> global node id
    int32_t* rows32;    // row -> its k neighbours (global ids)
    uint16_t* rows16;   // the same masked (node ids, then compact indices; 0xFFFF: none)
    uint8_t* mark;      // a byte per node: referenced by a row
    int32_t* map;       // node (global id) -> compact index (referenced nodes only)
    double* need;       // 3 doubles per referenced node (at need_off + compact index)
};

struct KnnSeg {
    KnnGrid* g;
    int* cell_of;
    int* sidx;
    double* sxyz;
    int* cnt;
    int* start;
    int* fill;
    unsigned long long* stat;
};
__device__ __forceinline__ KnnSeg knn_seg(const PlanBatchDev& P, int p) {
    char* b = P.kws + (size_t)p * P.kws_stride;
    return {reinterpret_cast<KnnGrid*>(b), reinterpret_cast<int*>(b + P.l_cell), reinterpret_cast<int*>(b + P.l_sidx),
            reinterpret_cast<double*>(b + P.l_sxyz), reinterpret_cast<int*>(b + P.l_cnt),
            reinterpret_cast<int*>(b + P.l_start), reinterpret_cast<int*>(b + P.l_fill),
            reinterpret_cast<unsigned long long*>(b + P.l_stat)};
}
__device__ __forceinline__ unsigned long long& pb_ctr(const PlanBatchDev& P, int field, int p) {
    return P.ctr[kPbPerSeg + field * P.S + p];
}
enum : int { kFQueries = 0, kFKept = 1, kFGoal = 2, kFNodes = 3, kFNeed = 4, kFInexact = 5 };

// samples (sample_uniform, as k_sample_uniform) + clears: the problem's compaction status words
// and node marks; problem 0 also the batch counters
// A batch of <= kPbSegSmall problems needs no upload of its own (a blit dispatch, ~5 us,
// before round 6): every workgroup takes its problem's seed and capacity from the launch
// arguments (P.seeds / P.caps), and workgroup (0, p) reads problem p from the pinned host
// copy and stores it into the device copy the later stages read.  Larger batches upload
// the problems first (P.seg_h null).
static_assert(sizeof(PlanSeg) % 8 == 0, "PlanSeg copied as 8-byte words");

__global__ __launch_bounds__(256) void k_pb_sample(PlanBatchDev P) {
    const int p = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool small = P.seg_h != nullptr;  // (uniform)
    if (small && blockIdx.x == 0 && threadIdx.x < (int)(sizeof(PlanSeg) / 8))
        reinterpret_cast<uint64_t*>(const_cast<PlanSeg*>(P.seg) + p)[threadIdx.x] =
            reinterpret_cast<const uint64_t*>(P.seg_h + p)[threadIdx.x];
    if (i < P.nbc) P.cstat[(int64_t)p * P.nbc + i] = 0ull;
    if (P.cap_total > 0 && i < P.NS / kCompactChunk) P.nstat[(int64_t)p * (P.NS / kCompactChunk) + i] = 0ull;
    // (the marks exist only when some problem has restricted rows: cap_total > 0)
    if (P.cap_total > 0 && i < (P.NS >> 4))
        reinterpret_cast<uint4*>(P.mark + ((int64_t)p << P.ns_log))[i] = make_uint4(0u, 0u, 0u, 0u);
    if (p == 0 && i < P.nctr) P.ctr[i] = 0ull;
    const uint64_t seed = small ? P.seeds[p] : P.seg[p].seed;
    const int32_t cap = small ? P.caps[p] : P.seg[p].cap;
    if (cap > 0) {  // the problem's k-NN grid: cleared cell counters and its shape
        const KnnSeg ks = knn_seg(P, p);
        if (i < P.nclr) ks.cnt[i] = 0;
        if (i == 0) {
            const PlanSeg q = small ? P.seg_h[p] : P.seg[p];
            KnnGrid gv{};
            int64_t cells = 1;
            double h = q.h;
            for (;;) {  // (cells bounded by the workspace's capacity; coarser if need be)
                cells = 1;
                for (int d = 0; d < 3; ++d) {
                    gv.dims[d] = (int)fmin((q.ghi[d] - q.glo[d]) / h, 1023.0) + 1;
                    cells *= gv.dims[d];
                }
                if (cells <= P.l_cap) break;
                h *= 1.25;
            }
            for (int d = 0; d < 3; ++d) gv.lo[d] = q.glo[d];
            gv.h = h;
            gv.inv_h = 1.0 / h;
            gv.ncell = (int)cells;
            gv.qbound = 1e300;
            *ks.g = gv;
        }
    }
    if (i >= P.ns) return;
    sample_uniform(seed, (uint64_t)i, P.lo, P.hi, P.xyz + ((int64_t)p * P.ns + i) * 3);
}

__device__ __forceinline__ double pb_ellipse(const PlanSeg& q, const double* x) {
    const double ds = sqrt((x[0] - q.s[0]) * (x[0] - q.s[0]) + (x[1] - q.s[1]) * (x[1] - q.s[1]) +
                           (x[2] - q.s[2]) * (x[2] - q.s[2]));
    const double dg = sqrt((x[0] - q.g[0]) * (x[0] - q.g[0]) + (x[1] - q.g[1]) * (x[1] - q.g[1]) +
                           (x[2] - q.g[2]) * (x[2] - q.g[2]));
    return ds + dg;
}

// Per node (problems with restricted rows): inside the grid ellipsoid -> its cell counted
// (cell_of, else -1); inside the row ellipsoid (widened by 1e-8 relative + 1e-6 m) ->
// listed as a query (ranks from one atomic per workgroup).
__device__ __forceinline__ bool pb_member(const PlanBatchDev& P, const PlanSeg& q, const KnnSeg& ks, const KnnGrid& g,
                                          int p, int node, const double* x) {
    const double f = pb_ellipse(q, x);
    int c = -1;
    if (f <= q.gbound) {
        const int cx = knn_cell_axis(x[0], g, 0), cy = knn_cell_axis(x[1], g, 1), cz = knn_cell_axis(x[2], g, 2);
        c = (cz * g.dims[1] + cy) * g.dims[0] + cx;
        atomicAdd(&ks.cnt[c], 1);
    }
    ks.cell_of[node] = c;
    return f <= q.bound * (1.0 + 1e-8) + 1e-6;
}

// nodes = start, goal, the valid samples in sample order (an ordered compaction, decoupled
// look-back as compact_block); the node count into the header; each node's membership
// (pb_member) as it is written, the queries listed.
__global__ __launch_bounds__(kCompactThreads) void k_pb_compact(PlanBatchDev P, uint32_t tag) {
    const int p = blockIdx.y, b = blockIdx.x, nb = gridDim.x;
    double* out = P.nodes + (int64_t)p * P.NS * 3;
    const PlanSeg& q = P.seg[p];
    const bool R = q.cap > 0;  // (block-uniform)
    const KnnSeg ks = knn_seg(P, p);
    KnnGrid g{};
    if (R) g = *ks.g;
    const double* xyz = P.xyz + (int64_t)p * P.ns * 3;
    const uint8_t* valid = P.valid + (int64_t)p * P.ns;
    unsigned long long* st = P.cstat + (int64_t)p * P.nbc;
    constexpr int NW = kCompactThreads / 64;
    __shared__ int wcnt[kCompactRounds * NW];
    __shared__ int qcnt[NW];
    __shared__ long long s_excl;
    __shared__ unsigned long long s_qbase;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool inq2 = false;  // start (thread 0) / goal (thread 1) of block 0: listed as queries
    if (b == 0 && threadIdx.x < 2) {
        const double* e = threadIdx.x == 0 ? q.s : q.g;
        out[3 * threadIdx.x] = e[0];
        out[3 * threadIdx.x + 1] = e[1];
        out[3 * threadIdx.x + 2] = e[2];
        if (R) inq2 = pb_member(P, q, ks, g, p, (int)threadIdx.x, e);
    }
    const int64_t i0 = (int64_t)b * kCompactChunk + threadIdx.x;
    bool v[kCompactRounds];
    unsigned long long bal[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int64_t i = i0 + r * kCompactThreads;
        v[r] = i < P.ns && valid[i] != 0;
    }
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        bal[r] = __ballot(v[r]);
        if (lane == 0) wcnt[r * NW + wv] = __popcll(bal[r]);
    }
    __syncthreads();
    int before[kCompactRounds], total = 0;
#pragma unroll
    for (int qq = 0; qq < kCompactRounds * NW; ++qq) {
#pragma unroll
        for (int r = 0; r < kCompactRounds; ++r)
            if (qq == r * NW + wv) before[r] = total;
        total += wcnt[qq];
    }
    if (wv == 0) {
        if (lane == 0) lb_publish(st, b, tag, b == 0, total);
        const long long ex = b == 0 ? 0ll : lb_exclusive(st, b, tag);
        if (lane == 0) {
            if (b > 0) lb_publish(st, b, tag, true, ex + total);
            s_excl = ex;
            if (b == nb - 1) pb_ctr(P, kFNodes, p) = (unsigned long long)(ex + total + 2);
        }
    }
    __syncthreads();
    const long long ex = s_excl;
    bool inq[kCompactRounds];
    int node[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        inq[r] = false;
        node[r] = 0;
        if (v[r]) {
            const int64_t i = i0 + r * kCompactThreads;
            const int64_t at = 2 + ex + before[r] +
                               (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal[r] >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)bal[r], 0u));
            const double x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
            out[3 * at] = x[0];
            out[3 * at + 1] = x[1];
            out[3 * at + 2] = x[2];
            node[r] = (int)at;
            if (R) inq[r] = pb_member(P, q, ks, g, p, (int)at, x);
        }
    }
    if (!R) return;  // (block-uniform)
    // the block's queries: one atomic per workgroup on the problem's query count
    unsigned long long qb[kCompactRounds + 1];
    int wq = 0;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        qb[r] = __ballot(inq[r]);
        wq += __popcll(qb[r]);
    }
    qb[kCompactRounds] = __ballot(inq2);
    wq += __popcll(qb[kCompactRounds]);
    if (lane == 0) qcnt[wv] = wq;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < NW; ++w) t += qcnt[w];
        s_qbase = t ? atomicAdd(&pb_ctr(P, kFQueries, p), (unsigned long long)t) : 0ull;
    }
    __syncthreads();
    unsigned long long rnk = s_qbase;
    for (int w = 0; w < wv; ++w) rnk += qcnt[w];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r <= kCompactRounds; ++r) {
        const bool mine = r < kCompactRounds ? inq[r] : inq2;
        const int nd = r < kCompactRounds ? node[r] : (int)threadIdx.x;
        if (mine) {
            const unsigned long long at = rnk + __popcll(qb[r] & below);
            if (at < (unsigned long long)q.cap) P.query[q.row_off + (int64_t)at] = nd;
        }
        rnk += __popcll(qb[r]);
    }
}

__global__ __launch_bounds__(kScanThreads) void k_pb_knn_scan(PlanBatchDev P, uint32_t tag) {
    if (P.seg[blockIdx.y].cap <= 0) return;
    const KnnSeg ks = knn_seg(P, blockIdx.y);
    knn_scan_block(ks.g, ks.cnt, ks.start, ks.stat, tag, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_pb_knn_scatter(PlanBatchDev P) {
    const int p = blockIdx.y;
    if (P.seg[p].cap <= 0) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (int)pb_ctr(P, kFNodes, p)) return;
    const KnnSeg ks = knn_seg(P, p);
    const int c = ks.cell_of[i];
    if (c < 0) return;
    const int pos = ks.start[c] + atomicAdd(&ks.fill[c], 1);
    if (pos >= ks.start[c + 1]) return;  // cannot happen with cleared counters
    const double* nd = P.nodes + ((int64_t)p * P.NS + i) * 3;
    ks.sidx[pos] = i;
    ks.sxyz[3 * pos] = nd[0];
    ks.sxyz[3 * pos + 1] = nd[1];
    ks.sxyz[3 * pos + 2] = nd[2];
}

// The exact k-NN row of one listed query from its problem's grid (whole wave).  Every node
// within distance r of x has |y - s| + |y - g| <= f(x) + 2 r, so while f(x) + 2 r <= gbound
// (with a margin far above the rounding) every such node is in the grid: the candidates
// within r are all the nodes within r.  r = 1.6 h first (~26 nodes at the grid's density),
// then x 1.5 until at least K are listed; each listed entry's rank in (distance, index)
// order is counted against the list (the order k_knn / the oracle use).  The box's x-runs of
// cells (one contiguous range of the cell-sorted nodes each) are laid out over all the lanes
// by a wave scan of their lengths, kU candidates per lane in flight.  Returns false when
// the radius would leave the grid ellipsoid or the list overflows (the row is then not
// exact, and the caller flags the problem).
#ifdef EPP_PB_ROWS_TL
// (diagnostics builds only: -DEPP_PB_ROWS_TL, scripts/pb_rows_timeline.py) per listed query
// d < kPbTl, lane 0's s_memrealtime (100 MHz) stamps: [0] query start, [1] first radius's
// run starts loaded, [2] its candidates listed, [3] row written, [4] radius iterations |
// candidates << 8 | wave << 32, [5] the wave's start
constexpr int kPbTl = 1 << 15;
__device__ unsigned long long g_pb_rows_tl[kPbTl][6];
#define EPP_PBTL(d, k, v)                                                     \
    do {                                                                      \
        if ((threadIdx.x & 63) == 0 && (d) < kPbTl) g_pb_rows_tl[(d)][(k)] = (v); \
    } while (0)
#define EPP_PBTL_NOW() __builtin_amdgcn_s_memrealtime()
#else
#define EPP_PBTL(d, k, v) \
    do {                  \
    } while (0)
#define EPP_PBTL_NOW() 0ull
#endif

template <int K>
__device__ __forceinline__ bool pb_query_row(const KnnGrid& g, const double* __restrict__ sxyz,
                                             const int* __restrict__ sidx, const int* __restrict__ start,
                                             const double (&p)[3], double f, double gbound, int self,
                                             int32_t* __restrict__ out, int64_t off, int tl_d = 0) {
    constexpr int kCap = 512;
    constexpr int kU = 2;  // candidates per lane in flight
    __shared__ double s_d[kCap];
    __shared__ int s_j[kCap];
    const int lane = threadIdx.x & 63;
    double r = 1.6 * g.h;
    for (int it = 0; it < 4; ++it, r *= 1.5) {  // wave-uniform
        if (!(f + 2.0 * r * (1.0 + 1e-9) + 1e-9 <= gbound)) return false;
        const double b2 = r * r;
        const double rb = r * (1.0 + 1e-9) + 1e-12 * (1.0 + fabs(p[0]) + fabs(p[1]) + fabs(p[2]));
        int lo[3], hi[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = knn_cell_axis(p[d] - rb, g, d);
            hi[d] = knn_cell_axis(p[d] + rb, g, d);
        }
        const int ny = hi[1] - lo[1] + 1, rows = ny * (hi[2] - lo[2] + 1);
        // (a row's x-run narrowed to the sphere's chord: the row's y / z cell ranges --
        // padded, the edge cells unbounded -- are at least dy / dz from p, so a node
        // within rb of p has |x - p.x| <= sqrt(rb^2 - dy^2 - dz^2); cells are monotone in x)
        const double pad = 1e-9 * (g.h + fabs(p[0]) + fabs(p[1]) + fabs(p[2]));
        auto gap = [&](int c, int d) {
            const double a = c == 0 ? -INFINITY : g.lo[d] + (double)c * g.h - pad;
            const double b = c == g.dims[d] - 1 ? INFINITY : g.lo[d] + (double)(c + 1) * g.h + pad;
            return p[d] < a ? a - p[d] : (p[d] > b ? p[d] - b : 0.0);
        };
        int cnt = 0;  // (wave-uniform)
        for (int rb0 = 0; rb0 < rows; rb0 += 64) {
            const int row = rb0 + lane;
            int s0 = 0, len = 0;
            if (row < rows) {
                const int cz = lo[2] + row / ny, cy = lo[1] + row % ny;
                const double dy = gap(cy, 1), dz = gap(cz, 2);
                const double rem2 = rb * rb - (dy * dy + dz * dz);
                if (rem2 >= 0.0) {
                    const double hx = sqrt(rem2) + pad;
                    const int x0 = max(lo[0], knn_cell_axis(p[0] - hx, g, 0));
                    const int x1 = min(hi[0], knn_cell_axis(p[0] + hx, g, 0));
                    const int a = (cz * g.dims[1] + cy) * g.dims[0];
                    s0 = start[a + x0];
                    len = start[a + x1 + 1] - s0;
                }
            }
            if (it == 0 && rb0 == 0) {
                [[maybe_unused]] const int lv = __shfl(len, 0, 64);  // (waits for the loads)
                EPP_PBTL(tl_d, 1, EPP_PBTL_NOW() + (unsigned long long)(lv & 0));
            }
            int incl = len;  // inclusive scan of the run lengths over the lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            const int excl = incl - len, T = __shfl(incl, 63, 64);
            for (int t0 = 0; t0 < T; t0 += 64 * kU) {
                double dd[kU];
                int jj[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const int t = t0 + u * 64 + lane;
                    // the run holding candidate t: the last lane whose exclusive start <= t
                    int a = 0;
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1)
                        if (__shfl(excl, a + step, 64) <= t) a += step;
                    const int q = __shfl(s0, a, 64) + (t - __shfl(excl, a, 64));
                    const bool ok = t < T;
                    const int qq = ok ? q : 0;  // (past the list: any valid entry, skipped below)
                    jj[u] = ok ? sidx[qq] : self;
                    const double ddx = sxyz[3 * qq] - p[0], ddy = sxyz[3 * qq + 1] - p[1], ddz = sxyz[3 * qq + 2] - p[2];
                    dd[u] = (ddx * ddx + ddy * ddy) + ddz * ddz;
                }
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const bool keep = jj[u] != self && dd[u] <= b2;
                    const unsigned long long kb = __ballot(keep);
                    const int at = cnt + __popcll(kb & ((1ull << lane) - 1ull));
                    if (keep && at < kCap) {
                        s_d[at] = dd[u];
                        s_j[at] = jj[u];
                    }
                    cnt += __popcll(kb);
                }
            }
        }
        if (it == 0) EPP_PBTL(tl_d, 2, EPP_PBTL_NOW());
        EPP_PBTL(tl_d, 4, (unsigned long long)(it + 1) | ((unsigned long long)cnt << 8));
        if (cnt > kCap) return false;
        if (cnt < K) continue;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's list is complete
        // entries [0, m) of the LDS list (m <= 64), entry i on lane i: each one's rank in
        // (distance, index) order counted against the others by v_readlane; ranks < K out
        auto rank_small = [&](int m) {
            const bool mine = lane < m;
            const double di = mine ? s_d[lane] : 0.0;
            const int ji = mine ? s_j[lane] : 0;
            const int dlo = __double2loint(di), dhi = __double2hiint(di);
            int rank = 0;
            for (int f2 = 0; f2 < m; ++f2) {
                const double df = __hiloint2double(__builtin_amdgcn_readlane(dhi, f2), __builtin_amdgcn_readlane(dlo, f2));
                rank += ((df < di) | ((df == di) & (__builtin_amdgcn_readlane(ji, f2) < ji))) ? 1 : 0;
            }
            if (mine && rank < K) out[rank] = (int32_t)(off + ji);
        };
        if (cnt <= 64) {
            rank_small(cnt);
        } else if (cnt <= 4 * 64) {
            // Longer lists (a second radius: 60-100 candidates): the K-th distance is
            // bracketed by bisection on wave ballots (the list in registers, four slots per
            // lane; 10 halvings of [0, r^2]), the entries at or below the bracket's top --
            // K plus the few that share its last interval -- are listed again and ranked
            // among themselves: an entry's preceding entries all lie in that list, so its
            // rank is its rank in the whole list.  (Instead of ranking every entry against
            // every other through LDS: 20 us for the slowest queries.)
            constexpr int kSl = 4;
            double dv[kSl];
            int jv[kSl];
#pragma unroll
            for (int sl = 0; sl < kSl; ++sl) {
                const int i = sl * 64 + lane;
                dv[sl] = i < cnt ? s_d[i] : INFINITY;
                jv[sl] = i < cnt ? s_j[i] : 0;
            }
            double lo = 0.0, hi = b2;  // count(d <= hi) >= K (every entry has d <= r^2)
            for (int step = 0; step < 10; ++step) {
                const double mid = 0.5 * (lo + hi);
                int c = 0;
#pragma unroll
                for (int sl = 0; sl < kSl; ++sl) c += __popcll(__ballot(dv[sl] <= mid));
                if (c >= K) hi = mid;
                else lo = mid;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the list is read: rewritten below)
            int m = 0;
#pragma unroll
            for (int sl = 0; sl < kSl; ++sl) {
                const bool in = dv[sl] <= hi;
                const unsigned long long b = __ballot(in);
                const int at = m + __popcll(b & ((1ull << lane) - 1ull));
                if (in && at < kCap) {
                    s_d[at] = dv[sl];
                    s_j[at] = jv[sl];
                }
                m += __popcll(b);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (m <= 64) {
                rank_small(m);
            } else {  // (many entries at one distance: rank every entry of the cut list)
                for (int i = lane; i < m; i += 64) {
                    const double di = s_d[i];
                    const int ji = s_j[i];
                    int rank = 0;
                    for (int f2 = 0; f2 < m; ++f2) {
                        const double df = s_d[f2];
                        rank += ((df < di) | ((df == di) & (s_j[f2] < ji))) ? 1 : 0;
                    }
                    if (rank < K) out[rank] = (int32_t)(off + ji);
                }
            }
        } else {
            for (int i = lane; i < cnt; i += 64) {
                const double di = s_d[i];
                const int ji = s_j[i];
                int rank = 0;
                for (int f2 = 0; f2 < cnt; ++f2) {  // (every lane reads entry f2: LDS broadcast)
                    const double df = s_d[f2];
                    rank += ((df < di) | ((df == di) & (s_j[f2] < ji))) ? 1 : 0;
                }
                if (rank < K) out[rank] = (int32_t)(off + ji);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the list is rewritten by the next query)
        return true;
    }
    return false;
}

// The listed queries' rows, dense in problem order (row d of problem p: its (d - first
// row of p)-th query), one wave per query: the row (global ids) and the row's node.
template <int K>
__global__ __launch_bounds__(64) void k_pb_rows(PlanBatchDev P) {
    const int lane = threadIdx.x;
    const int wave = blockIdx.x, nwaves = gridDim.x;  // (one wave per workgroup)
    // rows per problem (lane p holds problem p's) and their inclusive prefix
    int mine = 0;
    if (lane < P.S) mine = (int)min(pb_ctr(P, kFQueries, lane), (unsigned long long)max(P.seg[lane].cap, 0));
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int D = __shfl(incl, 63, 64);
    if (wave == 0 && lane == 0) P.ctr[kPbRows] = (unsigned long long)D;
    // The query's node and coordinates are loaded one query ahead (wave-uniform loads in
    // flight while the current query runs: two dependent round trips off every query).
    auto locate = [&](int d, int& p, int& self, double (&pt)[3]) {
        p = __popcll(__ballot(lane < P.S && incl <= d));  // problems whose rows end at or before d
        const int first = __builtin_amdgcn_readfirstlane(__shfl(incl - mine, p, 64));
        self = __builtin_amdgcn_readfirstlane(P.query[P.seg[p].row_off + (d - first)]);
        const double* x = P.nodes + (((int64_t)p << P.ns_log) + self) * 3;
        pt[0] = x[0];
        pt[1] = x[1];
        pt[2] = x[2];
    };
    int p_n = 0, self_n = 0;
    double pt_n[3] = {0.0, 0.0, 0.0};
    [[maybe_unused]] const unsigned long long tl_w0 = EPP_PBTL_NOW();
    if (wave < D) locate(wave, p_n, self_n, pt_n);
    // (static shares, d = wave + j nwaves: handing the queries out by one atomic counter
    // serialised ~19k same-address atomics at one L2 channel -- 0.17 -> 0.37 ms per batch;
    // and every load behind a pending atomic waits for it: vmcnt counts in order)
    for (int d = wave; d < D; d += nwaves) {  // wave-uniform
        EPP_PBTL(d, 0, EPP_PBTL_NOW());
        EPP_PBTL(d, 5, tl_w0);
        const int p = p_n, self = self_n;
        const double pt[3] = {pt_n[0], pt_n[1], pt_n[2]};
        if (d + nwaves < D) locate(d + nwaves, p_n, self_n, pt_n);
        const PlanSeg& q = P.seg[p];
        const int64_t off = (int64_t)p << P.ns_log;
        const KnnSeg ks = knn_seg(P, p);
        const KnnGrid g = *ks.g;
        const double f = pb_ellipse(q, pt);
        if (lane == 0) P.ids32[d] = (int32_t)(off + self);
        if (!pb_query_row<K>(g, ks.sxyz, ks.sidx, ks.start, pt, f, q.gbound, self, P.rows32 + (int64_t)d * K, off, d)) {
            if (lane == 0) pb_ctr(P, kFInexact, p) = 1ull;
            if (lane < K) P.rows32[(int64_t)d * K + lane] = -1;  // (the problem takes the whole table)
        }
#ifdef EPP_PB_ROWS_TL
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        EPP_PBTL(d, 3, EPP_PBTL_NOW());
        if ((threadIdx.x & 63) == 0 && d < kPbTl) g_pb_rows_tl[d][4] |= (unsigned long long)wave << 32;
#endif
    }
}

// Per problem: the marked nodes numbered in node order -- an ordered compaction of the
// marks, chunks of 1024 node ids per workgroup (4 rounds of 256), the chunk's offset by
// decoupled look-back (lb_exclusive); map[node] = its index, its coordinates listed at
// need_off + index.  The workgroup holding the problem's last node writes the count.
__global__ __launch_bounds__(kCompactThreads) void k_pb_number(PlanBatchDev P, uint32_t tag) {
    const int p = blockIdx.y;
    const PlanSeg& q = P.seg[p];
    if (q.cap <= 0) return;  // (block-uniform)
    const int n = (int)pb_ctr(P, kFNodes, p);
    const int b = blockIdx.x;
    if (b * kCompactChunk >= n) return;  // (no later chunk waits on it)
    constexpr int NW = kCompactThreads / 64;
    __shared__ int wcnt[kCompactRounds * NW];
    __shared__ long long s_excl;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t off = (int64_t)p << P.ns_log;
    unsigned long long* st = P.nstat + (int64_t)p * (P.NS / kCompactChunk);
    bool v[kCompactRounds];
    unsigned long long bal[kCompactRounds];
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const int i = b * kCompactChunk + r * kCompactThreads + threadIdx.x;
        v[r] = i < n && P.mark[off + i] != 0;
        bal[r] = __ballot(v[r]);
        if (lane == 0) wcnt[r * NW + wv] = __popcll(bal[r]);
    }
    __syncthreads();
    int before[kCompactRounds], total = 0;
#pragma unroll
    for (int qq = 0; qq < kCompactRounds * NW; ++qq) {
#pragma unroll
        for (int r = 0; r < kCompactRounds; ++r)
            if (qq == r * NW + wv) before[r] = total;
        total += wcnt[qq];
    }
    if (wv == 0) {
        if (lane == 0) lb_publish(st, b, tag, b == 0, total);
        const long long ex = b == 0 ? 0ll : lb_exclusive(st, b, tag);
        if (lane == 0) {
            if (b > 0) lb_publish(st, b, tag, true, ex + total);
            s_excl = ex;
            if ((b + 1) * kCompactChunk >= n) pb_ctr(P, kFNeed, p) = (unsigned long long)(ex + total);
        }
    }
    __syncthreads();
    const long long ex = s_excl;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        if (v[r]) {
            const int i = b * kCompactChunk + r * kCompactThreads + threadIdx.x;
            const long long at = ex + before[r] +
                                 (long long)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal[r] >> 32),
                                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)bal[r], 0u));
            P.map[off + i] = (int32_t)at;
            if (at < q.need_cap) {
                const double* x = P.nodes + (off + i) * 3;
                double* d = P.need + (q.need_off + at) * 3;
                d[0] = x[0];
                d[1] = x[1];
                d[2] = x[2];
            }
        }
    }
}

// The results into pinned host memory, only the bytes in use: the header (counters), the
// rows' problem and compact node index (u32), the masked rows in compact indices (u16,
// renumbered here through `map` as they are copied), every problem's referenced nodes
// (24 B each, at its own offset).  16-byte stores (the device parts are 16-byte padded).
// Each workgroup then publishes `seq` in its completion slot (publish_done, completion.h):
// the host polls the slots instead of synchronising the stream.
__global__ __launch_bounds__(256) void k_pb_emit(PlanBatchDev P, unsigned long long* __restrict__ hdr,
                                                  uint4* __restrict__ h_slot, uint4* __restrict__ h_rows,
                                                  uint4* __restrict__ h_need, uint32_t* __restrict__ done,
                                                  uint32_t seq) {
    __shared__ long long pre[65];  // 16-byte chunks of the referenced nodes before problem p (S <= 64)
    __shared__ long long first[64];
    const int64_t rows = (int64_t)P.ctr[kPbRows];
    if (threadIdx.x == 0) {
        long long a = 0;
        for (int p = 0; p < P.S; ++p) {
            pre[p] = a;
            // problem p's slots [need_off, need_off + cnt) as 16-byte chunks (24 B per node;
            // need_off is even, so the range starts on a chunk)
            const long long cnt = min((long long)pb_ctr(P, kFNeed, p), (long long)P.seg[p].need_cap);
            first[p] = P.seg[p].need_off * 3 / 2;
            a += (cnt * 3 + 1) / 2;
        }
        pre[P.S] = a;
    }
    __syncthreads();
    const int64_t c_slot = (rows * 4 + 15) / 16, c_rows = (rows * P.k * 2 + 15) / 16, c_need = pre[P.S];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid < P.nctr) hdr[tid] = P.ctr[tid];
    const uint4* d_rows = reinterpret_cast<const uint4*>(P.rows16);
    const uint4* d_need = reinterpret_cast<const uint4*>(P.need);
    const uint32_t lmask = (1u << P.ns_log) - 1u;
    // a row entry (node id in its problem, 0xFFFF: none) in compact indices
    auto remap = [&](int64_t e, uint32_t v) -> uint32_t {
        if (v == 0xFFFFu || e >= rows * P.k) return v;
        const int32_t u = P.ids32[e / P.k];
        return (uint32_t)P.map[(u & ~(int32_t)lmask) + (int32_t)v] & 0xFFFFu;
    };
    for (int64_t c = tid; c < c_slot + c_rows + c_need; c += (int64_t)gridDim.x * 256) {
        if (c < c_slot) {  // (p << 16 | the row's node, compact) for rows 4c .. 4c + 3
            uint32_t sv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t r = 4 * c + j;
                const int32_t u = r < rows ? P.ids32[r] : 0;
                sv[j] = r < rows ? (((uint32_t)u >> P.ns_log) << 16) | ((uint32_t)P.map[u] & 0xFFFFu) : 0u;
            }
            h_slot[c] = make_uint4(sv[0], sv[1], sv[2], sv[3]);
        } else if (c < c_slot + c_rows) {  // 8 row entries
            const int64_t cr = c - c_slot;
            const uint4 w = d_rows[cr];
            const uint32_t in[4] = {w.x, w.y, w.z, w.w};
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t e = 8 * cr + 2 * j;
                o[j] = remap(e, in[j] & 0xFFFFu) | (remap(e + 1, in[j] >> 16) << 16);
            }
            h_rows[cr] = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            const int64_t r = c - c_slot - c_rows;
            int p = 0;
            while (p + 1 < P.S && pre[p + 1] <= r) ++p;
            const int64_t at = first[p] + (r - pre[p]);
            h_need[at] = d_need[at];
        }
    }
    publish_done(done + blockIdx.x, seq);
}

constexpr int kPbEmitMax = 1024;  // emit workgroups (one completion slot each)

}  // namespace
}  // namespace epp

using namespace epp;

#ifdef EPP_PB_ROWS_TL
// (diagnostics builds only) the last k_pb_rows launch's per-query stamps: 6 u64 each
extern "C" epp_status epp_dbg_pb_rows_tl(unsigned long long* out, int64_t n) {
    if (n > kPbTl) n = kPbTl;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pb_rows_tl), (size_t)n * 48) == hipSuccess ? EPP_OK : EPP_ERR_HIP;
}
#endif

// ---- the batched planner's host side (epp_internal.h) ---------------------------------
epp::PlanBatchLayout epp::plan_batch_layout(int32_t S, int64_t ns, int32_t k, PlanSeg* segs) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    PlanBatchLayout L;
    L.S = S;
    L.k = k;
    L.ns = ns;
    L.ns_log = 16;
    while ((1ll << L.ns_log) < ns + 2) ++L.ns_log;
    L.NS = 1ll << L.ns_log;
    L.nbc = (int32_t)std::max<int64_t>(1, (ns + kCompactChunk - 1) / kCompactChunk);
    // rows: the problems' capacities; referenced nodes: a row's node and its k neighbours
    // per row, at most the problem's nodes (even counts: 24-byte entries on 16-byte chunks)
    int64_t rows = 0, need = 0;
    for (int p = 0; p < S; ++p) {
        segs[p].cap = std::max(0, segs[p].cap);
        segs[p].row_off = rows;
        rows += segs[p].cap;
        segs[p].need_off = need;
        segs[p].need_cap =
            segs[p].cap > 0 ? (int32_t)((std::min<int64_t>((int64_t)segs[p].cap * (k + 1) + 2, ns + 2) + 1) & ~1ll) : 0;
        need += segs[p].need_cap;
    }
    L.cap_total = (int32_t)rows;
    L.need_cap = need;
    L.nctr = kPbPerSeg + 6 * S;
    const bool R = rows > 0;
    const KnnLayout kl = knn_layout((int)(ns + 2));
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += al(bytes);
        return at;
    };
    L.o_seg = take((size_t)S * sizeof(PlanSeg));
    L.o_ctr = take((size_t)L.nctr * 8);
    L.o_xyz = take((size_t)S * ns * 24);
    L.o_valid = take((size_t)S * ns);
    L.o_nodes = take((size_t)S * L.NS * 24);
    L.o_cstat = take((size_t)S * L.nbc * 8);
    L.kws_stride = R ? al(kl.bytes) : 0;
    L.o_kws = take((size_t)S * L.kws_stride);
    const size_t capr = ((size_t)rows + 3) & ~size_t(3);
    L.o_query = take(capr * 4);
    L.o_ids32 = take(capr * 4);
    L.o_rows32 = take(capr * k * 4);
    L.o_rows16 = take(capr * k * 2);
    L.o_ev = take(capr * k);
    L.o_mark = take(R ? (size_t)S * L.NS : 0);
    L.o_map = take(R ? (size_t)S * L.NS * 4 : 0);
    L.o_nstat = take(R ? (size_t)S * (L.NS / kCompactChunk) * 8 : 0);
    L.o_need = take((size_t)L.need_cap * 24 + 16);
    L.dev_bytes = o;
    o = 0;
    L.h_seg = take((size_t)S * sizeof(PlanSeg));
    L.h_hdr = take((size_t)L.nctr * 8);
    L.h_slot = take(capr * 4);
    L.h_rows = take(capr * k * 2);
    L.h_need = take((size_t)L.need_cap * 24 + 16);
    {  // emit workgroups: each one's completion release writes back its XCD's L2 (once per
       // workgroup since completion.h; kernel trace, scripts/gpu_emit_ab.sh: 64 -> 26.6 us,
       // 128 -> 21.6, 256 -> 23.3, 512 -> 29.1)
        static const int eb = [] {
            const char* e = std::getenv("EPP_PB_EMIT_BLOCKS");  // (A/B knob: same results)
            const int v = e && *e ? std::atoi(e) : 128;
            return std::max(1, std::min(kPbEmitMax, v));
        }();
        L.done_n = eb;
    }
    L.h_done = take((size_t)L.done_n * 4);
    L.host_bytes = o;
    return L;
}

// EPP_PB_TRACE=1 (diagnostics knob, read once): events between the batch's stages on its
// stream; plan_batch_trace_print() (after the batch completed) prints each stage's time in
// microseconds to stderr, one line per batch.
namespace {
struct PbTrace {
    bool on = false;
    int n = 0;
    hipEvent_t ev[16] = {};
    const char* name[16] = {};
};
PbTrace& pb_trace() {
    static const bool on = [] {
        const char* e = std::getenv("EPP_PB_TRACE");
        return e && std::atoi(e) == 1;
    }();
    thread_local PbTrace t;
    if (on && !t.on) {
        t.on = true;
        for (auto& e : t.ev) (void)hipEventCreate(&e);
    }
    return t;
}
void pb_mark(hipStream_t s, const char* name) {
    PbTrace& t = pb_trace();
    if (!t.on || t.n >= 16) return;
    t.name[t.n] = name;
    (void)hipEventRecord(t.ev[t.n++], s);
}
}  // namespace

void epp::plan_batch_trace_print() {
    PbTrace& t = pb_trace();
    if (!t.on || t.n < 2) return;
    (void)hipEventSynchronize(t.ev[t.n - 1]);
    std::string line = "pb_trace:";
    float tot = 0;
    for (int i = 1; i < t.n; ++i) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, t.ev[i - 1], t.ev[i]);
        tot += ms;
        line += std::string(" ") + t.name[i] + "=" + std::to_string((int)(ms * 1000.0f + 0.5f));
    }
    line += " total=" + std::to_string((int)(tot * 1000.0f + 0.5f));
    std::fprintf(stderr, "%s\n", line.c_str());
    t.n = 0;
}

epp_status epp::plan_batch_launch(const epp_world* world, int32_t can_pass_gate, const double lo[3], const double hi[3],
                                  const PlanBatchLayout& L, void* dev, void* host, uint32_t seq, void* stream) {
    if (!world || !dev || !host || L.S < 1 || L.S > 64 || L.ns < 1 || (L.k != 4 && L.k != 8 && L.k != 16) ||
        ((int64_t)L.S << L.ns_log) >= (1ll << 31) || (reinterpret_cast<uintptr_t>(dev) & 255) ||
        (reinterpret_cast<uintptr_t>(host) & 255)) {
        set_error("plan_batch_launch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    char* d = static_cast<char*>(dev);
    char* h = static_cast<char*>(host);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const KnnLayout kl = knn_layout((int)(L.ns + 2));
    PlanBatchDev P{};
    P.seg = reinterpret_cast<const PlanSeg*>(d + L.o_seg);
    P.S = L.S;
    P.k = L.k;
    P.ns_log = L.ns_log;
    P.nbc = L.nbc;
    P.cap_total = L.cap_total;
    P.nctr = L.nctr;
    P.ns = L.ns;
    P.NS = L.NS;
    for (int i = 0; i < 3; ++i) {
        P.lo[i] = lo[i];
        P.hi[i] = hi[i];
    }
    P.xyz = reinterpret_cast<double*>(d + L.o_xyz);
    P.valid = reinterpret_cast<uint8_t*>(d + L.o_valid);
    P.nodes = reinterpret_cast<double*>(d + L.o_nodes);
    P.cstat = reinterpret_cast<unsigned long long*>(d + L.o_cstat);
    P.ctr = reinterpret_cast<unsigned long long*>(d + L.o_ctr);
    P.kws = d + L.o_kws;
    P.kws_stride = L.kws_stride;
    P.l_cell = kl.cell;
    P.l_sidx = kl.sidx;
    P.l_sxyz = kl.sxyz;
    P.l_cnt = kl.cnt;
    P.l_start = kl.start;
    P.l_fill = kl.fill;
    P.l_stat = kl.stat;
    P.l_cap = kl.cap;
    P.nclr = (int)((kl.start - kl.cnt) / sizeof(int));
    P.query = reinterpret_cast<int32_t*>(d + L.o_query);
    P.ids32 = reinterpret_cast<int32_t*>(d + L.o_ids32);
    P.rows32 = reinterpret_cast<int32_t*>(d + L.o_rows32);
    P.rows16 = reinterpret_cast<uint16_t*>(d + L.o_rows16);
    P.mark = reinterpret_cast<uint8_t*>(d + L.o_mark);
    P.nstat = reinterpret_cast<unsigned long long*>(d + L.o_nstat);
    P.map = reinterpret_cast<int32_t*>(d + L.o_map);
    P.need = reinterpret_cast<double*>(d + L.o_need);
    const unsigned S = (unsigned)L.S;
    const bool R = L.cap_total > 0;
    // the problems: in k_pb_sample's arguments (<= kPbSegSmall), else uploaded first; then
    // every stage on this stream
    P.seg_h = nullptr;
    if (L.S <= kPbSegSmall) {
        P.seg_h = reinterpret_cast<const PlanSeg*>(h + L.h_seg);
        for (int p = 0; p < L.S; ++p) {
            P.seeds[p] = P.seg_h[p].seed;
            P.caps[p] = P.seg_h[p].cap;
        }
    } else {
        if (hipMemcpyAsync(d + L.o_seg, h + L.h_seg, (size_t)L.S * sizeof(PlanSeg), hipMemcpyHostToDevice, s) !=
            hipSuccess)
            return launch_error("plan_batch_launch");
    }
    const int64_t clr = std::max<int64_t>({L.ns, R ? L.NS >> 4 : 0, R ? (int64_t)P.nclr : 0, (int64_t)L.nbc, (int64_t)L.nctr});
    pb_mark(s, "begin");
    hipLaunchKernelGGL(k_pb_sample, dim3((unsigned)((clr + 255) / 256), S), dim3(256), 0, s, P);
    if (const epp_status st = epp_check_states(world, P.xyz, (int64_t)L.S * L.ns, can_pass_gate, P.valid, nullptr,
                                               nullptr, stream))
        return st;
    pb_mark(s, "states");
    hipLaunchKernelGGL(k_pb_compact, dim3((unsigned)L.nbc, S), dim3(kCompactThreads), 0, s, P, next_scan_tag());
    if (R) {
        const unsigned gn = (unsigned)((L.ns + 2 + 255) / 256);
        pb_mark(s, "compact_member");
        hipLaunchKernelGGL(k_pb_knn_scan, dim3((unsigned)kl.scan_blocks, S), dim3(kScanThreads), 0, s, P, next_scan_tag());
        hipLaunchKernelGGL(k_pb_knn_scatter, dim3(gn, S), dim3(256), 0, s, P);
        pb_mark(s, "scan_scatter");
        // one wave per workgroup, 28 per CU (16 resident at ~110 VGPRs; a variant with four
        // queries per wave, 16 lanes each, was 1.9x slower: its 16-lane shuffles and LDS
        // ranking cost more issue than the overlapped loads saved)
        static const int rows_wg = [] {  // (A/B knob: one-wave workgroups per CU)
            const char* e = std::getenv("EPP_PB_ROWS_WG");
            const int v = e && *e ? std::atoi(e) : 28;
            return std::max(1, std::min(64, v));
        }();
        const dim3 gr((unsigned)std::max(1, cu_count() * rows_wg)), br(64);
        if (L.k == 4) hipLaunchKernelGGL(k_pb_rows<4>, gr, br, 0, s, P);
        else if (L.k == 8) hipLaunchKernelGGL(k_pb_rows<8>, gr, br, 0, s, P);
        else hipLaunchKernelGGL(k_pb_rows<16>, gr, br, 0, s, P);
        pb_mark(s, "rows");
        // the motions, with the marks of the referenced nodes and the per-problem kept /
        // goal edge counts folded into the launch
        MotionMask marks;
        marks.mark = P.mark;
        marks.pkept = P.ctr + kPbPerSeg + kFKept * L.S;
        marks.pgoal = P.ctr + kPbPerSeg + kFGoal * L.S;
        marks.ns_log = L.ns_log;
        marks.nprob = L.S;
        if (const epp_status st = check_knn_motions_rows(
                world, P.nodes, P.rows32, P.ids32, reinterpret_cast<const int64_t*>(P.ctr + kPbRows), L.cap_total,
                L.k, can_pass_gate, reinterpret_cast<uint8_t*>(d + L.o_ev), P.rows16, -1, nullptr, stream, &marks))
            return st;
        pb_mark(s, "motions_marks");
        hipLaunchKernelGGL(k_pb_number, dim3((unsigned)((L.ns + 2 + kCompactChunk - 1) / kCompactChunk), S),
                           dim3(kCompactThreads), 0, s, P, next_scan_tag());
        pb_mark(s, "number");
    }
    hipLaunchKernelGGL(k_pb_emit, dim3((unsigned)L.done_n), dim3(256), 0, s, P,
                       reinterpret_cast<unsigned long long*>(h + L.h_hdr), reinterpret_cast<uint4*>(h + L.h_slot),
                       reinterpret_cast<uint4*>(h + L.h_rows), reinterpret_cast<uint4*>(h + L.h_need),
                       reinterpret_cast<uint32_t*>(h + L.h_done), seq);
    pb_mark(s, "emit");
    return launch_error("plan_batch_launch");
}
