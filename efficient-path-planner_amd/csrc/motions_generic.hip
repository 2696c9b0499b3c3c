// motions_generic.hip — k_motions, the motion check for worlds too large for LDS
// (motions_kernels.h).
#include "collision_common.h"
#include "motions_kernels.h"

namespace epp {
namespace {

// Generic kernel (worlds whose coarse grid + records exceed LDS): one lane per edge, four
// edges per lane and iteration, the world read through L1/L2.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_motions(WorldView w, const double* __restrict__ s1,
                                                    const double* __restrict__ s2, int64_t n,
                                                    int can_pass, uint8_t* __restrict__ valid,
                                                    int aligned) {
    const Acc a = make_acc(w.blob, w.blob, w);
    const int64_t groups = (n + 3) / 4;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += stride) {
        const int64_t first = 4 * g;
        double vs[12], ve[12];
        load4(s1, first, n, aligned != 0, vs);
        load4(s2, first, n, aligned != 0, ve);
        uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (first + k < n) {
                const double* s = vs + 3 * k;
                const double* e = ve + 3 * k;
                f[k] = (MODE == 0 ? ray_valid(a, w, s, e, can_pass != 0)
                                  : ray_valid_d32(a, w, s, e, can_pass != 0))
                           ? 1u
                           : 0u;
            }
        store4(valid, first, n, f);
    }
}

}  // namespace

void launch_motions_generic(const WorldView& w, const double* s1, const double* s2, int64_t n, int32_t can_pass_gate,
                            int32_t mode, uint8_t* valid, hipStream_t st) {
    const int aligned = ((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 15) == 0;
    const int grid = grid_for((n + 3) / 4, 0);
    if (mode == 0)
        hipLaunchKernelGGL((k_motions<0>), dim3(grid), dim3(kBlock), 0, st, w, s1, s2, n, can_pass_gate, valid, aligned);
    else
        hipLaunchKernelGGL((k_motions<1>), dim3(grid), dim3(kBlock), 0, st, w, s1, s2, n, can_pass_gate, valid, aligned);
}

}  // namespace epp
