// knn_retry.hip — the retry pass of the tiled k-NN (knn_kernels.h): k_knn_retry, one wave for
// each query k_knn_tile put on the retry list.  Also the diagnostics build's storage and exports.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "epp_internal.h"
#include "knn_diag.h"
#include "knn_kernels.h"

#ifdef EPP_KNN_DIAG
// (diagnostics builds only) the timelines' storage and their read-out
namespace epp {
namespace {
__device__ unsigned long long g_knn_retry_tl[kKnnRetryTl][4];  // k_knn_retry's records
// k_knn_tile's records: 16 u64 per block
unsigned long long* knn_tl_buffer() {
    static unsigned long long* buf = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        if (hipMalloc(&buf, (size_t)16 * 8 * kKnnTlBlocks) != hipSuccess) buf = nullptr;
    });
    return buf;
}
}  // namespace
unsigned long long* knn_tl_begin(hipStream_t s) {
    unsigned long long* d = knn_tl_buffer();
    if (d) (void)hipMemsetAsync(d, 0, (size_t)16 * 8 * kKnnTlBlocks, s);
    return d;
}
}  // namespace epp
extern "C" {
// the last k_knn_tile launch's phase timeline: 16 u64 per block
epp_status epp_dbg_knn_tl(unsigned long long* out, int64_t blocks) {
    unsigned long long* d = epp::knn_tl_buffer();
    if (!d || blocks > epp::kKnnTlBlocks) return EPP_ERR_RUNTIME;
    return hipMemcpy(out, d, (size_t)blocks * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess ? EPP_OK : EPP_ERR_HIP;
}
// the last k_knn_retry launch: per retried query start, end, bound (f64 bits), node -- 4 u64 each
epp_status epp_dbg_knn_retry_tl(unsigned long long* out, int64_t n) {
    if (n > epp::kKnnRetryTl) n = epp::kKnnRetryTl;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(epp::g_knn_retry_tl), (size_t)n * 32) == hipSuccess ? EPP_OK
                                                                                                  : EPP_ERR_HIP;
}
}
#endif

namespace epp {
namespace {

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
        bi[k] = kKnnNone;
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
            for (int k = 0; k < K; ++k) below += (bi[k] != kKnnNone && bd[k] < bound) ? 1 : 0;
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
        if (lane == 0) nbr[(int64_t)self * K + k] = mi;  // (kKnnNone = -1: fewer than K)
        if (mi != kKnnNone && bi[0] == mi) {  // the winning lane drops its head
#pragma unroll
            for (int t = 0; t + 1 < K; ++t) {
                bd[t] = bd[t + 1];
                bi[t] = bi[t + 1];
            }
            bd[K - 1] = r2max;
            bi[K - 1] = kKnnNone;
        }
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
        EPP_KRTL_BEGIN;
        knn_retry_wave<K>(g, r2max, nodes, sxyz, sidx, start, retry[i], retry_b[i], nbr);
        EPP_KRTL_RECORD(i, retry_b[i], retry[i]);
    }
}

}  // namespace

// One wave per retried query: kRetryPerCu per CU (waves without a query exit at once; more
// retries than waves loop)
constexpr int kRetryPerCu = 8;
void knn_retry_launch(int k, int cus, const double* nodes, double r2, const KnnWs& w, int32_t* nbr, hipStream_t s) {
    const dim3 gr((unsigned)std::max(1, cus * kRetryPerCu)), br(64);
    knn_for_k<false>(k, [&](auto K) {
        hipLaunchKernelGGL(k_knn_retry<K.value>, gr, br, 0, s, w.g, r2, nodes, w.sxyz, w.sidx, w.start, w.retry,
                           w.retry_b, nbr);
    });
}

}  // namespace epp
