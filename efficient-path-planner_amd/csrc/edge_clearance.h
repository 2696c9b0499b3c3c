// edge_clearance.h — the one definition of "edge clearance": the squared Euclidean distance
// between a straight edge s -> e and a collision (non-filling) OBB and where along the edge it
// is attained, shared by k_motions_clearance (edge_clearance.hip) and k_traj_chord_clearance
// (trajcheck.hip), so both compute the same bits.  The entry is clear_entry's (clearance.h:
// centre, cos, sin, half sizes h, not inflated).
//
// Both endpoints go into the box frame by clear_d2's operations (a from s, b from e):
//   dx = px - cx;  dy = py - cy;  dz = pz - cz;   lx = c*dx + s*dy;  ly = c*dy - s*dx;  lz = dz
// and d = b - a per axis.  Along the edge q(t) = a + t*d per axis, and for a local point q
//   F(q) = (ex*ex + ey*ey) + ez*ez,   e_k = max(|q_k| - h_k, 0)             (clear_d2's d2)
//   G(q) = (wx + wy) + wz,            w_k = e_k * (q_k < 0 ? -d_k : d_k)    (half of df/dt)
// f(t) = F(q(t)) is convex and piecewise quadratic, its pieces joined where an axis crosses a
// face plane, so its minimum over [0, 1] is at an end, at a face crossing, or at the zero of
// the piecewise linear, non-decreasing G inside one piece.  The candidates, in this order, the
// running minimum starting from +inf and taking a candidate on a strict <:
//   1. t = 0:  f = F(a), which is clear_d2(entry, s) itself
//   2. t = 1:  f = F(b), which is clear_d2(entry, e) itself
//   3. axes x, y, z, for each the face -h_k then +h_k:  t = (-+h_k - a_k) / d_k, kept iff
//      0 < t < 1 (d_k == 0 gives an infinity or a NaN, which is not kept):  f = F(q(t)).
//      The bracket of G's zero: (tl, gl) starts at (0, G(a)) and (tr, gr) at (1, G(b)); a kept
//      t with g = G(q(t)) < 0 and t > tl replaces (tl, gl), one with g >= 0 and t < tr
//      replaces (tr, gr): no face crossing is left between tl and tr, so G is linear there
//   4. iff G(a) < 0 < G(b):  t* = tl + (tr - tl) * ((-gl) / (gr - gl)),  f = F(q(t*))
// d2_i is the smallest f and t_i the candidate that gave it.  Every operation is one IEEE fp64
// multiply, add, subtract or divide in this association (-ffp-contract=off); the max and every
// other choice is a select on a compare, which keeps a NaN out of the minimum (a NaN compares
// false).  A filling OBB needs no case of its own: with hz = -inf every f is +inf (ez = +inf,
// never 0 * inf: ex, ey are finite) and no strict < takes it, so its d2_i is +inf whatever its
// G came to.  Over the world: every OBB in the world's order on a strict <, so the lowest
// index that attains the minimum wins; an edge with a coordinate that is not finite takes part
// in nothing (its s may well be finite, and F(a) with it).  One square root, after the minimum.
#pragma once
#include <hip/hip_runtime.h>

#include "clearance.h"

namespace epp {

struct ClearEdge {
    double s[3], e[3];
    bool finite;  // all six coordinates
    __device__ __forceinline__ void set(double sx, double sy, double sz, double ex, double ey, double ez) {
        s[0] = sx, s[1] = sy, s[2] = sz;
        e[0] = ex, e[1] = ey, e[2] = ez;
        finite = (fabs(sx) < HUGE_VAL) & (fabs(sy) < HUGE_VAL) & (fabs(sz) < HUGE_VAL) & (fabs(ex) < HUGE_VAL) &
                 (fabs(ey) < HUGE_VAL) & (fabs(ez) < HUGE_VAL);  // (NaN compares false)
    }
};

// clear_d2's frame change of one point.
__device__ __forceinline__ void edge_local(const double (&en)[kClearDoubles], const double (&p)[3], double (&l)[3]) {
    const double dx = p[0] - en[0], dy = p[1] - en[1], dz = p[2] - en[2];
    const double c = en[3], s = en[4];
    l[0] = c * dx + s * dy;
    l[1] = c * dy - s * dx;
    l[2] = dz;
}

// F(q) and G(q) of a local point.
__device__ __forceinline__ void edge_fg(const double (&en)[kClearDoubles], const double (&q)[3], const double (&d)[3],
                                        double& f, double& g) {
    const double ex = clear_pos(fabs(q[0]) - en[5]);
    const double ey = clear_pos(fabs(q[1]) - en[6]);
    const double ez = clear_pos(fabs(q[2]) - en[7]);
    f = (ex * ex + ey * ey) + ez * ez;
    const double wx = ex * (q[0] < 0.0 ? -d[0] : d[0]);
    const double wy = ey * (q[1] < 0.0 ? -d[1] : d[1]);
    const double wz = ez * (q[2] < 0.0 ? -d[2] : d[2]);
    g = (wx + wy) + wz;
}

// d2_i and t_i of one entry.  Branch-free.
__device__ __forceinline__ double edge_d2(const double (&en)[kClearDoubles], const ClearEdge& edge, double& t_at) {
    double a[3], b[3], d[3];
    edge_local(en, edge.s, a);
    edge_local(en, edge.e, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = b[k] - a[k];
    double f0, g0, f1, g1;
    edge_fg(en, a, d, f0, g0);
    edge_fg(en, b, d, f1, g1);
    double best = HUGE_VAL, tb = -1.0;
    bool lt = f0 < best;
    best = lt ? f0 : best;
    tb = lt ? 0.0 : tb;
    lt = f1 < best;
    best = lt ? f1 : best;
    tb = lt ? 1.0 : tb;
    double tl = 0.0, gl = g0, tr = 1.0, gr = g1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const double face = side ? en[5 + k] : -en[5 + k];
            const double t = (face - a[k]) / d[k];
            const bool ok = (0.0 < t) & (t < 1.0);
            const double q[3] = {a[0] + t * d[0], a[1] + t * d[1], a[2] + t * d[2]};
            double f, g;
            edge_fg(en, q, d, f, g);
            lt = ok & (f < best);
            best = lt ? f : best;
            tb = lt ? t : tb;
            const bool lo = ok & (g < 0.0) & (t > tl);
            const bool hi = ok & (g >= 0.0) & (t < tr);
            tl = lo ? t : tl;
            gl = lo ? g : gl;
            tr = hi ? t : tr;
            gr = hi ? g : gr;
        }
    }
    const double ts = tl + (tr - tl) * ((-gl) / (gr - gl));
    const double q[3] = {a[0] + ts * d[0], a[1] + ts * d[1], a[2] + ts * d[2]};
    double f, g;
    edge_fg(en, q, d, f, g);
    lt = (g0 < 0.0) & (0.0 < g1) & (f < best);
    best = lt ? f : best;
    tb = lt ? ts : tb;
    t_at = tb;
    return best;
}

// One entry into the running minimum of an edge (strict <: ascending callers keep the lowest index).
__device__ __forceinline__ void edge_take(const double (&en)[kClearDoubles], int index, const ClearEdge& edge,
                                          double& best, double& t_best, int& obb) {
    double t;
    const double d2 = edge_d2(en, edge, t);
    const bool lt = edge.finite & (d2 < best);
    best = lt ? d2 : best;
    t_best = lt ? t : t_best;
    obb = lt ? index : obb;
}

// The running minimum of one edge over entries [i0, i0 + n) held at `tile` (LDS: every lane
// of a wave reads the same entry, a broadcast read), ascending.
__device__ __forceinline__ void edge_min_tile(const double* tile, int i0, int n, const ClearEdge& edge, double& best,
                                              double& t_best, int& obb) {
    for (int i = 0; i < n; ++i) {
        double en[kClearDoubles];
#pragma unroll
        for (int k = 0; k < kClearDoubles; ++k) en[k] = tile[i * kClearDoubles + k];
        edge_take(en, i0 + i, edge, best, t_best, obb);
    }
}

// The same over records [i0, i1) read where they lie (through L2).
__device__ __forceinline__ void edge_min_recs(const double* __restrict__ recs, int i0, int i1, const ClearEdge& edge,
                                              double& best, double& t_best, int& obb) {
    for (int i = i0; i < i1; ++i) {
        double en[kClearDoubles];
        clear_entry(recs + (size_t)i * kRecDoubles, en);
        edge_take(en, i, edge, best, t_best, obb);
    }
}

}  // namespace epp
