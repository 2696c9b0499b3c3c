// first_hit.h — the one definition of "first hit": where along a straight edge s -> e the
// world first blocks it and which OBB does, shared by k_motions_first_hit (first_hit.hip) and
// k_traj_first_hit (trajcheck.hip), so both compute the same bits.
//
// The candidates are the OBBs World::checkRayValid (src/World.cpp:130-162) would test:
//   - OBB i takes part iff its stored inflated AABB (the records' own doubles) overlaps the
//     edge's bounding box, closed on both sides (the rtree's intersects);
//   - a filling OBB is skipped when can_pass_gate is 1  (:150-153).
// For a candidate, rec_ray_parts (collision_common.h: the operations of rec_ray_hit, which is
// OBB::checkCollisionWithRay, src/OBB.cpp:10-61, with r = r_gate for a gate's OBB and r_obst
// otherwise) gives start_hit and end_hit (the endpoint tests, inflated iff the OBB is not
// filling), slab_hit (the final predicate on tMin and tMax after the three axes) and tMin.
// The entry parameter of OBB i is
//   t_i = 0.0    if start_hit
//         tMin   else if slab_hit
//         1.0    else if end_hit     (reachable through the |d| < 1e-6 parallel branch, which
//                                     tests the start against the faces and never the end)
//         none   otherwise: OBB i does not block the edge  (+inf here)
// and the edge's answer t_hit = min_i t_i with the lowest index i that attains it, +inf / -1
// when nothing blocks.  So obb >= 0 exactly when rec_ray_hit is true for some candidate: when
// epp_check_motions (mode 0) gives flag 0.  Every operation is one IEEE fp64 multiply, add,
// subtract or divide (-ffp-contract=off); a zero may carry either sign.  Non-finite endpoints
// go through the same operations (NaN compares false).
#pragma once
#include <hip/hip_runtime.h>

#include "collision_common.h"

namespace epp {
namespace {

// Records per LDS tile (136 B each: 34 KB).  Worlds with more OBBs take further tiles.
constexpr int kHitTile = 256;

// An edge with its bounding box (the rtree query of src/World.cpp:135-141).
struct HitEdge {
    double s[3], e[3], lo[3], hi[3];
    __device__ __forceinline__ void set(double sx, double sy, double sz, double ex, double ey, double ez) {
        s[0] = sx, s[1] = sy, s[2] = sz;
        e[0] = ex, e[1] = ey, e[2] = ez;
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // (ray_valid's selects)
            lo[k] = (e[k] < s[k]) ? e[k] : s[k];
            hi[k] = (s[k] < e[k]) ? e[k] : s[k];
        }
    }
};

// t_i of one record (kRecDoubles doubles, LDS or HBM), +inf when the OBB does not take part or
// does not block the edge.  Branch-free.
__device__ __forceinline__ double hit_entry(const double* rec, const HitEdge& g, double rg, double ro, bool can_pass) {
    const uint32_t m = (uint32_t)__double_as_longlong(rec[R_META]);
    const bool overlap = !((rec[F_HIX] < g.lo[0]) | (g.hi[0] < rec[F_LOX]) | (rec[F_HIY] < g.lo[1]) |
                           (g.hi[1] < rec[F_LOY]) | (rec[F_HIZ] < g.lo[2]) | (g.hi[2] < rec[F_LOZ]));
    const bool takes_part = overlap & !(((m & META_FILLING) != 0u) & can_pass);
    const RayParts p = rec_ray_parts(rec, g.s, g.e, (m & META_GATE) ? rg : ro);
    const double t = p.start_hit ? 0.0 : (p.slab_hit ? p.tMin : (p.end_hit ? 1.0 : HUGE_VAL));
    return takes_part ? t : HUGE_VAL;
}

// The running minimum of one edge over records i0, i0 + step, ... < i1 of `recs` (record 0 at
// recs[0]; the reported index is base + i), ascending, strict <: the lowest index wins a tie.
__device__ __forceinline__ void hit_min(const double* recs, int i0, int i1, int step, int base, const HitEdge& g,
                                        double rg, double ro, bool can_pass, double& best, int& obb) {
    for (int i = i0; i < i1; i += step) {
        const double t = hit_entry(recs + (size_t)i * kRecDoubles, g, rg, ro, can_pass);
        const bool lt = t < best;
        best = lt ? t : best;
        obb = lt ? base + i : obb;
    }
}

}  // namespace
}  // namespace epp
