// plan_geometry.h — the geometry of one problem of the batched planner: a pure function of
// its ends and the sampling box (standard library only).
//
// Row-restricted search: A* pops nodes in increasing f = g + h >= |x - start| + |x - goal|,
// so a search that reaches the goal with every popped f <= bound has expanded only
// nodes inside the ellipsoid |x - start| + |x - goal| <= bound, and pops exactly what the
// search over the whole table pops (a node outside has f > bound >= the path's length):
// the same path.  bound = ellipse * |start - goal| + 0.25 m; capacity 1.25 x the
// ellipsoid's expected rows (its volume, unclipped, over the sampling box's) + 1024, not
// past half the nodes.  Otherwise (a pop above the bound, rows past the capacity, no kept
// edge into the goal among the rows, more than 65,535 nodes) the whole table is built.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace epp {

struct PlanBox {          // what the problems of one batch share
    double lo[3], hi[3];  // the sampling box (the world's bounds)
    int64_t nmax;         // nodes of a problem at most: samples + 2
    double ellipse;       // the bound's factor
    bool restrict_ok;     // restricted rows can be built at all (else cap = 0)
};

// From q's ends s, g (PlanSeg's fields, epp_internal.h): bound, gbound, the grid's cell h and
// box glo / ghi (the gbound ellipsoid's box, foci s and g, padded, clipped to kbox), the row
// capacity cap (0: no restricted rows); kbox: the whole table's k-NN box, lo then hi.
template <class Seg>
void plan_geometry(Seg& q, double kbox[6], const PlanBox& b) {
    // the rows' k-NN grid: cells of ~1.5 nodes (the sampling density), over the nodes of the
    // ellipsoid bound + 7.5 cells (a query's search radius r stays below half the margin:
    // |x - s| + |x - g| is 2-Lipschitz, so every node within r of a row's node is in it)
    const double vbox = (b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]);
    q.h = std::cbrt(1.5 * std::max(vbox, 1e-12) / (double)b.nmax);
    const double dx = q.g[0] - q.s[0], dy = q.g[1] - q.s[1], dz = q.g[2] - q.s[2];
    const double d_sg = std::sqrt((dx * dx + dy * dy) + dz * dz);  // (Vec3::norm's order)
    q.bound = b.ellipse * d_sg + 0.25;
    q.gbound = q.bound + 7.5 * q.h;
    const double a = 0.5 * q.gbound, b2 = std::max(0.0, a * a - 0.25 * d_sg * d_sg);
    for (int d = 0; d < 3; ++d) {
        // the grid over the sampling box widened by start and goal (every node lies inside)
        kbox[d] = std::min({b.lo[d], q.s[d], q.g[d]});
        kbox[3 + d] = std::max({b.hi[d], q.s[d], q.g[d]});
        const double u = d_sg > 0 ? (q.g[d] - q.s[d]) / d_sg : 0.0;
        const double e = std::sqrt(a * a * u * u + b2 * (1.0 - u * u)) * (1.0 + 1e-6) + 1e-6;
        const double c = 0.5 * (q.s[d] + q.g[d]);
        q.glo[d] = std::max(kbox[d], c - e);
        q.ghi[d] = std::min(kbox[3 + d], c + e);
    }
    q.cap = 0;
    if (b.restrict_ok) {
        const double vell = M_PI * q.bound * (q.bound * q.bound - d_sg * d_sg) / 6.0;
        const double frac = vbox > 0 ? std::min(1.0, vell / vbox) : 1.0;
        const double want = 1.25 * frac * (double)b.nmax + 1024.0;
        if (want < 0.5 * (double)b.nmax) q.cap = (int32_t)want;
    }
}

}  // namespace epp
