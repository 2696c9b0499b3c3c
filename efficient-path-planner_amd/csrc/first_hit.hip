// first_hit.hip — where along each straight edge of a batch the world first blocks it, and
// which OBB does (gfx950): epp_motions_first_hit.  The reference's
// MotionValidator::checkMotion(s1, s2, lastValid) (src/MotionValidator.cpp:19-22) is a stub;
// this is the entry parameter World::checkRayValid (src/World.cpp:130-162) computes per OBB
// (tMin of OBB::checkCollisionWithRay, src/OBB.cpp:10-61) and discards, minimised over the
// OBBs it would test (first_hit.h).
//
// Shape: one edge per lane, 256-thread workgroups, one group of edges each.  The world's
// 136-byte records are staged into LDS in tiles of kHitTile (34 KB); every lane of a wave reads
// the same record (a broadcast read), the body is branch-free -- the AABB prefilter and the
// filling skip are per-record compares folded into the select, no grid or tile filter takes
// part -- and keeps a strict < minimum over the ascending OBB index, so the lowest index that
// attains the minimum is the answer.  A world larger than one tile loops over the tiles, two
// barriers each.
#include <climits>
#include <cmath>

#include "first_hit.h"

namespace epp {
namespace {

constexpr int kHitBlock = 256;

__global__ __launch_bounds__(kHitBlock) void k_motions_first_hit(const double* __restrict__ recs, int n_obb, double rg,
                                                                 double ro, const double* __restrict__ s1,
                                                                 const double* __restrict__ s2, int64_t n, int can_pass,
                                                                 double* __restrict__ t_hit, int32_t* __restrict__ obb) {
    __shared__ __attribute__((aligned(16))) double tile[kHitTile * kRecDoubles];
    const int64_t i = (int64_t)blockIdx.x * kHitBlock + threadIdx.x;
    const bool live = i < n;
    const int64_t ii = live ? i : n - 1;  // (a spare lane repeats the last edge and writes nothing)
    HitEdge g;
    g.set(s1[3 * ii], s1[3 * ii + 1], s1[3 * ii + 2], s2[3 * ii], s2[3 * ii + 1], s2[3 * ii + 2]);
    const bool cp = can_pass != 0;
    double best = HUGE_VAL;
    int hit = -1;
    // block-uniform trip count: every thread runs every iteration (barriers)
    for (int i0 = 0; i0 < n_obb; i0 += kHitTile) {
        const int cnt = min(kHitTile, n_obb - i0);
        if (i0) __syncthreads();  // the previous tile's readers are done
        const double* src = recs + (size_t)i0 * kRecDoubles;
        for (int k = threadIdx.x; k < cnt * kRecDoubles; k += kHitBlock) tile[k] = src[k];
        __syncthreads();
        hit_min(tile, 0, cnt, 1, i0, g, rg, ro, cp, best, hit);
    }
    if (live) {
        t_hit[i] = best;
        if (obb) obb[i] = hit;
    }
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_motions_first_hit(const epp_world* world, const double* s1, const double* s2, int64_t n,
                                 int32_t can_pass_gate, double* t_hit, int32_t* obb, void* stream) {
    const int64_t groups = n > 0 ? (n + kHitBlock - 1) / kHitBlock : 0;
    if (!world || n < 0 || groups > INT_MAX || (can_pass_gate != 0 && can_pass_gate != 1) ||
        (n > 0 && (!s1 || !s2 || !t_hit))) {
        set_error("epp_motions_first_hit: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    IndexLease ix;  // (a stale index is rebuilt here, as by epp_check_motions)
    if (const epp_status st = ensure_index(world, &ix)) return st;
    const WorldView& v = ix.view;
    const double* recs = reinterpret_cast<const double*>(v.blob + v.off_aos);
    hipLaunchKernelGGL(k_motions_first_hit, dim3((unsigned)groups), dim3(kHitBlock), 0, (hipStream_t)stream, recs,
                       v.n_obb, v.r_gate, v.r_obst, s1, s2, n, (int)can_pass_gate, t_hit, obb);
    return launch_error("epp_motions_first_hit");
}

}  // extern "C"
