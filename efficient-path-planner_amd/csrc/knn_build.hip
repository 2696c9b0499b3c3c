// knn_build.hip — the grid build of the exact k-NN (knn_kernels.h): the grid's shape over the
// nodes' bounding box (k_knn_bounds_part, k_knn_setup) or over the caller's box (k_knn_prep), the
// nodes per cell (k_knn_count), the cells' first positions (k_knn_scan) and the cell-sorted copy
// of the nodes (k_knn_scatter).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "knn_diag.h"
#include "knn_kernels.h"

namespace epp {
namespace {

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

}  // namespace

void knn_build_launch(const double* nodes, int n, const KnnWs& w, hipStream_t s, const double* box_lo,
                      const double* box_hi) {
    const dim3 g256((n + 255) / 256), b256(256);
    const int nb = std::max(1, std::min(kBoundsBlocks, (n + kBoundsThreads - 1) / kBoundsThreads));
    const double npc = knn_nodes_per_cell();
    // the first kernel clears w.nclr ints from w.cnt on: cnt, fill and the scan's status words
    if (box_lo && box_hi) {  // the caller's box: the grid shape on the host, one kernel
        KnnGrid gv{};
        const double mn[3] = {box_lo[0], box_lo[1], box_lo[2]}, mx[3] = {box_hi[0], box_hi[1], box_hi[2]};
        knn_grid_shape(mn, mx, n, w.cap, npc, &gv);
        hipLaunchKernelGGL(k_knn_prep, dim3(nb), dim3(kBoundsThreads), 0, s, gv, w.g, w.cnt, w.nclr);
    } else {
        hipLaunchKernelGGL(k_knn_bounds_part, dim3(nb), dim3(kBoundsThreads), 0, s, nodes, n, w.part, w.cnt, w.nclr);
        hipLaunchKernelGGL(k_knn_setup, dim3(1), dim3(64), 0, s, w.part, nb, n, w.cap, npc, w.g);
    }
    hipLaunchKernelGGL(k_knn_count, g256, b256, 0, s, nodes, n, w.g, w.cell_of, w.cnt);
    hipLaunchKernelGGL(k_knn_scan, dim3(w.scan_blocks), dim3(kScanThreads), 0, s, w.g, w.cnt, w.start, w.stat,
                       next_scan_tag());
    hipLaunchKernelGGL(k_knn_scatter, g256, b256, 0, s, nodes, n, w.cell_of, w.start, w.fill, w.sxyz, w.sidx);
}

}  // namespace epp
