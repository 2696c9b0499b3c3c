// gate_pass.h — the one definition of "the edge p1 -> p2 crosses gate g", shared by
// k_gates_crossed and k_traj_gates (gate_pass.hip) and by the host's resolution of a sampled
// trajectory (host_online.cpp: plannedGatePasses), so all compute the same bits.
//
//   OnlineTrajGenerator::checkGatePassed  src/OnlineTrajGenerator.cpp:228-256
//
// A gate frame is five doubles [cx, cy, cz, c, s]: the gate centre (position + (0, 0,
// height[type]), getGateCenterAndNormal) and cos / sin of its yaw, computed once on the host;
// nothing here calls a trigonometric function.
//
//   t1 = p1 - centre;  g1 = (c*t1.x - s*t1.y,  s*t1.x + c*t1.y,  t1.z)      (same for p2 -> g2)
//   crossed = g1.y < 0  &&  g2.y > 0  &&  |(g1.x + g2.x) / 2| <= half_edge
//                                     &&  |(g1.z + g2.z) / 2| <= half_edge
//
// Every operation is one IEEE fp64 multiply, add, subtract or divide in this association
// (-ffp-contract=off).  From negative to positive gate-frame y only, both inequalities strict:
// a point exactly on the gate plane crosses on neither side.  NaN compares false.  With a
// crossing go the plane parameter u = g1.y / (g1.y - g2.y) and the two midpoint offsets the
// predicate tested.  Plain C++ apart from the HIP qualifiers.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPP_GP_FN __host__ __device__ __forceinline__
#else
#define EPP_GP_FN inline
#endif
#include <cmath>

namespace epp {

constexpr int kGateDoubles = 5;  // cx, cy, cz, cos, sin
constexpr int kMaxGates = 64;    // one bit of a mask each

struct GateCross {
    double g1y, g2y;  // gate-frame y of the two ends
    double mx, mz;    // the midpoint offsets
    bool crossed;
    EPP_GP_FN double u() const { return g1y / (g1y - g2y); }  // (asked only of a crossing: g1y < 0 < g2y)
};

EPP_GP_FN GateCross gate_cross(const double* f, double half_edge, double p1x, double p1y, double p1z, double p2x,
                               double p2y, double p2z) {
    const double c = f[3], s = f[4];
    const double ax = p1x - f[0], ay = p1y - f[1], az = p1z - f[2];
    const double bx = p2x - f[0], by = p2y - f[1], bz = p2z - f[2];
    const double g1x = c * ax - s * ay, g2x = c * bx - s * by;
    GateCross r;
    r.g1y = s * ax + c * ay;
    r.g2y = s * bx + c * by;
    r.mx = (g1x + g2x) / 2.0;
    r.mz = (az + bz) / 2.0;
    r.crossed = (r.g1y < 0.0) & (r.g2y > 0.0) & (fabs(r.mx) <= half_edge) & (fabs(r.mz) <= half_edge);
    return r;
}

}  // namespace epp
