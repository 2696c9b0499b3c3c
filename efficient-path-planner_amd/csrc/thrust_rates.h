// thrust_rates.h — the one definition of the input-feasibility quantities of a differentially
// flat quadrotor track at one sample (Mueller, Hehn, D'Andrea 2015), shared by k_thrust_rates
// and k_traj_thrust_rates (thrust_rates.hip) and by tests/thrust_rates_host.cpp, so all compute
// the same bits.  No reference counterpart: the reference limits |v| and |a| only.
//
// For the acceleration a and the jerk j of a sample and the gravity g:
//
//   Fx = ax;  Fy = ay;  Fz = az + g                      (mass-normalised thrust vector)
//   f2 = (Fx*Fx + Fy*Fy) + Fz*Fz;       thrust   = sqrt(f2)
//   cx = Fy*jz - Fz*jy;  cy = Fz*jx - Fx*jz;  cz = Fx*jy - Fy*jx
//   w2 = (cx*cx + cy*cy) + cz*cz;       rate     = sqrt(w2) / f2    (= |F x j| / |F|^2: the rate
//                                                                    of the thrust direction,
//                                                                    the roll / pitch body rate)
//                                       cos_tilt = Fz / thrust
//
// Every operation is one IEEE fp64 multiply, add, subtract, divide or square root in this
// association (-ffp-contract=off); no trigonometric function.  At f2 == 0 (free fall) thrust is
// 0, cos_tilt NaN and rate NaN or +inf, as the operations give.  Plain C++ apart from the HIP
// qualifiers.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPP_TR_FN __host__ __device__ __forceinline__
#else
#define EPP_TR_FN inline
#endif
#include <cmath>

namespace epp {

struct ThrustRates {
    double thrust, rate, cos_tilt;
};

EPP_TR_FN ThrustRates thrust_rates(double ax, double ay, double az, double jx, double jy, double jz, double g) {
    const double Fx = ax, Fy = ay, Fz = az + g;
    const double f2 = (Fx * Fx + Fy * Fy) + Fz * Fz;
    const double cx = Fy * jz - Fz * jy, cy = Fz * jx - Fx * jz, cz = Fx * jy - Fy * jx;
    const double w2 = (cx * cx + cy * cy) + cz * cz;
    ThrustRates r;
    r.thrust = sqrt(f2);
    r.rate = sqrt(w2) / f2;
    r.cos_tilt = Fz / r.thrust;
    return r;
}

}  // namespace epp
