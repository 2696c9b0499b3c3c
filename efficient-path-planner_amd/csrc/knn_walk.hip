// knn_walk.hip — the two one-thread-per-query kernels of the exact k-NN (knn_kernels.h): k_knn
// over all pairs, k_knn_grid walking shells of grid cells (knn_grid.h's knn_walk).
#include <hip/hip_runtime.h>

#include "knn_kernels.h"

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
        bi[k] = kKnnNone;
    }
    knn_walk<K>(g, c, p, self, bd, bi, sxyz, sidx, start, 0);
    knn_store<K>(nbr, self, bi);
}

}  // namespace

void knn_brute_launch(int k, const double* nodes, int n, double r2, int32_t* nbr, hipStream_t s) {
    const dim3 grid((n + kKnnBlock - 1) / kKnnBlock), block(kKnnBlock);
    knn_for_k<true>(k, [&](auto K) { hipLaunchKernelGGL(k_knn<K.value>, grid, block, 0, s, nodes, n, r2, nbr); });
}

void knn_walk_launch(int k, int n, double r2, const KnnWs& w, int32_t* nbr, hipStream_t s) {
    const dim3 grid((n + 255) / 256), block(256);
    knn_for_k<true>(k, [&](auto K) {
        hipLaunchKernelGGL(k_knn_grid<K.value>, grid, block, 0, s, w.g, n, r2, w.sxyz, w.sidx, w.start, nbr);
    });
}

}  // namespace epp
