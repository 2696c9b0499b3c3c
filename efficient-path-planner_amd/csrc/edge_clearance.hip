// edge_clearance.hip — the distance from every straight edge of a batch to the nearest
// collision OBB, and where along the edge it is attained (gfx950): epp_motions_clearance.  No
// reference counterpart: the reference answers "does the inflated box block the edge?"
// (World::checkRayValid, src/World.cpp:130-162); this is the Euclidean distance between the
// segment and the box itself (edge_clearance.h), over every OBB of the world, so an edge that
// passes a bar between its two ends gets the margin it really keeps.
//
// Shape: k_states_clearance's (clearance.hip) with an edge in place of a state: one edge per
// lane, 256-thread workgroups, one group of edges each.  The world's records are staged into
// LDS as compact 64-byte entries in tiles of kClearTile (16 KB); every lane of a wave reads the
// same entry (a broadcast read), the body is branch-free and keeps a strict < minimum over the
// ascending OBB index.  A world larger than one tile loops over the tiles, two barriers each.
// The square root is taken once, after the minimum.
#include <climits>
#include <cmath>

#include "collision_common.h"
#include "edge_clearance.h"

namespace epp {
namespace {

constexpr int kEdgeClearBlock = 256;

__global__ __launch_bounds__(kEdgeClearBlock) void k_motions_clearance(const double* __restrict__ recs, int n_obb,
                                                                      const double* __restrict__ s1,
                                                                      const double* __restrict__ s2, int64_t n,
                                                                      double* __restrict__ dist,
                                                                      double* __restrict__ t_min,
                                                                      int32_t* __restrict__ nearest) {
    __shared__ __attribute__((aligned(16))) double tile[kClearTile * kClearDoubles];
    const int64_t i = (int64_t)blockIdx.x * kEdgeClearBlock + threadIdx.x;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;  // (a spare lane repeats the last edge and writes nothing)
    ClearEdge g;
    g.set(s1[3 * ii], s1[3 * ii + 1], s1[3 * ii + 2], s2[3 * ii], s2[3 * ii + 1], s2[3 * ii + 2]);
    double best = HUGE_VAL, t_best = -1.0;
    int obb = -1;
    // block-uniform trip count: every thread runs every iteration (barriers)
    for (int i0 = 0; i0 < n_obb; i0 += kClearTile) {
        const int cnt = min(kClearTile, n_obb - i0);
        if (i0) __syncthreads();  // the previous tile's readers are done
        clear_stage(recs, i0, cnt, tile, kEdgeClearBlock);
        __syncthreads();
        edge_min_tile(tile, i0, cnt, g, best, t_best, obb);
    }
    if (live) {
        dist[i] = sqrt(best);
        if (t_min) t_min[i] = t_best;
        if (nearest) nearest[i] = obb;
    }
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_motions_clearance(const epp_world* world, const double* s1, const double* s2, int64_t n, double* dist,
                                 double* t_min, int32_t* nearest, void* stream) {
    const int64_t groups = n > 0 ? (n + kEdgeClearBlock - 1) / kEdgeClearBlock : 0;
    if (!world || n < 0 || groups > INT_MAX || (n > 0 && (!s1 || !s2 || !dist))) {
        set_error("epp_motions_clearance: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    IndexLease ix;  // (a stale index is rebuilt here, as by epp_states_clearance)
    if (const epp_status st = ensure_index(world, &ix)) return st;
    const WorldView& v = ix.view;
    const double* recs = reinterpret_cast<const double*>(v.blob + v.off_aos);
    hipLaunchKernelGGL(k_motions_clearance, dim3((unsigned)groups), dim3(kEdgeClearBlock), 0, (hipStream_t)stream, recs,
                       v.n_obb, s1, s2, n, dist, t_min, nearest);
    return launch_error("epp_motions_clearance");
}

}  // extern "C"
