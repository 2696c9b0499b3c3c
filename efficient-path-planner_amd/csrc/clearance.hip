// clearance.hip — the distance from every state of a batch to the nearest collision OBB
// (gfx950): epp_states_clearance.  No reference counterpart: the reference answers "closer
// than minDistance?" per state (World::checkPointValidity, src/World.cpp:106-128), behind its
// rtree's AABB prefilter; this is the Euclidean distance itself (clearance.h), over every OBB
// of the world, so a state far from everything still gets its distance.
//
// Shape: one state per lane, 256-thread workgroups, one group of states each.  The world's
// records are staged into LDS as compact 64-byte entries in tiles of kClearTile (16 KB); every
// lane of a wave reads the same entry (a broadcast read), the body is branch-free and keeps a
// strict < minimum over the ascending OBB index, so the lowest index that attains the minimum
// is the nearest.  A world larger than one tile loops over the tiles, two barriers each.  The
// square root is taken once, after the minimum.
#include <climits>
#include <cmath>

#include "clearance.h"
#include "collision_common.h"

namespace epp {
namespace {

constexpr int kClearBlock = 256;

__global__ __launch_bounds__(kClearBlock) void k_states_clearance(const double* __restrict__ recs, int n_obb,
                                                                 const double* __restrict__ xyz, int64_t n,
                                                                 double* __restrict__ dist,
                                                                 int32_t* __restrict__ nearest) {
    __shared__ __attribute__((aligned(16))) double tile[kClearTile * kClearDoubles];
    const int64_t i = (int64_t)blockIdx.x * kClearBlock + threadIdx.x;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;  // (a spare lane repeats the last state and writes nothing)
    const double px = xyz[3 * ii], py = xyz[3 * ii + 1], pz = xyz[3 * ii + 2];
    double best = HUGE_VAL;
    int obb = -1;
    // block-uniform trip count: every thread runs every iteration (barriers)
    for (int i0 = 0; i0 < n_obb; i0 += kClearTile) {
        const int cnt = min(kClearTile, n_obb - i0);
        if (i0) __syncthreads();  // the previous tile's readers are done
        clear_stage(recs, i0, cnt, tile, kClearBlock);
        __syncthreads();
        clear_min_tile(tile, i0, cnt, px, py, pz, best, obb);
    }
    if (live) {
        dist[i] = sqrt(best);
        if (nearest) nearest[i] = obb;
    }
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_states_clearance(const epp_world* world, const double* xyz, int64_t n, double* dist, int32_t* nearest,
                                void* stream) {
    const int64_t groups = n > 0 ? (n + kClearBlock - 1) / kClearBlock : 0;
    if (!world || n < 0 || groups > INT_MAX || (n > 0 && (!xyz || !dist))) {
        set_error("epp_states_clearance: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    IndexLease ix;  // (a stale index is rebuilt here, as by epp_check_states_mindist)
    if (const epp_status st = ensure_index(world, &ix)) return st;
    const WorldView& v = ix.view;
    const double* recs = reinterpret_cast<const double*>(v.blob + v.off_aos);
    hipLaunchKernelGGL(k_states_clearance, dim3((unsigned)groups), dim3(kClearBlock), 0, (hipStream_t)stream, recs,
                       v.n_obb, xyz, n, dist, nearest);
    return launch_error("epp_states_clearance");
}

}  // extern "C"
