// clearance.h — the one definition of "clearance": the squared Euclidean distance from a point
// to a collision (non-filling) OBB, shared by k_states_clearance (clearance.hip) and
// k_traj_clearance (trajcheck.hip), so both compute the same bits.
//
//   dx = px - cx;  dy = py - cy;  dz = pz - cz
//   lx = c*dx + s*dy;  ly = c*dy - s*dx            (the records' own cos / sin, as rec_hit)
//   ex = max(|lx| - hx, 0);  ey = max(|ly| - hy, 0);  ez = max(|dz| - hz, 0)   (not inflated)
//   d2 = (ex*ex + ey*ey) + ez*ez
//
// Every operation is one IEEE fp64 multiply, add or subtract in this association
// (-ffp-contract=off).  The max is a select that keeps a NaN (v_max_f64 would drop it): a
// non-finite point gives a NaN or +inf d2, which the strict < of the running minimum never
// takes.  There is no grid, no AABB prefilter and no inflate radius here: every OBB of the
// world is visited, in the world's order, and the lowest index that attains the minimum wins.
#pragma once
#include <hip/hip_runtime.h>

#include "epp_internal.h"

namespace epp {

// Entries per LDS tile (64 B each: 16 KB).  Worlds with more OBBs take further tiles.
constexpr int kClearTile = 256;
constexpr int kClearDoubles = 8;  // centre (3), cos, sin, half sizes (3)

// The compact entry of record i (epp_internal.h: kRecDoubles doubles, fields in the order of
// enum Field).  A filling OBB keeps its slot, so indices stay the world's; the select below
// makes it inert: with hz = -inf, ez = |dz| + inf = +inf and so d2 = +inf (NaN for a NaN
// point), which no strict < takes.
__device__ __forceinline__ void clear_entry(const double* __restrict__ rec, double (&e)[kClearDoubles]) {
    const uint32_t m = (uint32_t)__double_as_longlong(rec[R_META]);
    e[0] = rec[F_CX];
    e[1] = rec[F_CY];
    e[2] = rec[F_CZ];
    e[3] = rec[F_COS];
    e[4] = rec[F_SIN];
    e[5] = rec[F_HX];
    e[6] = rec[F_HY];
    e[7] = (m & META_FILLING) ? -HUGE_VAL : rec[F_HZ];
}

__device__ __forceinline__ double clear_pos(double a) { return a < 0.0 ? 0.0 : a; }  // max(a, 0), NaN kept

__device__ __forceinline__ double clear_d2(const double (&e)[kClearDoubles], double px, double py, double pz) {
    const double dx = px - e[0], dy = py - e[1], dz = pz - e[2];
    const double c = e[3], s = e[4];
    const double lx = c * dx + s * dy;
    const double ly = c * dy - s * dx;
    const double ex = clear_pos(fabs(lx) - e[5]);
    const double ey = clear_pos(fabs(ly) - e[6]);
    const double ez = clear_pos(fabs(dz) - e[7]);
    return (ex * ex + ey * ey) + ez * ez;
}

// The running minimum of one point over entries [i0, i0 + n) held at `tile` (LDS: every lane
// of a wave reads the same entry, a broadcast read), ascending, strict <.
__device__ __forceinline__ void clear_min_tile(const double* tile, int i0, int n, double px, double py, double pz,
                                               double& best, int& obb) {
    for (int i = 0; i < n; ++i) {
        double e[kClearDoubles];
#pragma unroll
        for (int k = 0; k < kClearDoubles; ++k) e[k] = tile[i * kClearDoubles + k];
        const double d2 = clear_d2(e, px, py, pz);
        const bool lt = d2 < best;
        best = lt ? d2 : best;
        obb = lt ? i0 + i : obb;
    }
}

// The same over records [i0, i1) read where they lie (through L2).
__device__ __forceinline__ void clear_min_recs(const double* __restrict__ recs, int i0, int i1, double px, double py,
                                               double pz, double& best, int& obb) {
    for (int i = i0; i < i1; ++i) {
        double e[kClearDoubles];
        clear_entry(recs + (size_t)i * kRecDoubles, e);
        const double d2 = clear_d2(e, px, py, pz);
        const bool lt = d2 < best;
        best = lt ? d2 : best;
        obb = lt ? i : obb;
    }
}

// Block-wide: entries [i0, i0 + n) of the records into `tile` (n <= kClearTile).  No barrier.
__device__ __forceinline__ void clear_stage(const double* __restrict__ recs, int i0, int n, double* tile, int nthreads) {
    for (int i = threadIdx.x; i < n; i += nthreads) {
        double e[kClearDoubles];
        clear_entry(recs + (size_t)(i0 + i) * kRecDoubles, e);
#pragma unroll
        for (int k = 0; k < kClearDoubles; ++k) tile[i * kClearDoubles + k] = e[k];
    }
}

}  // namespace epp
