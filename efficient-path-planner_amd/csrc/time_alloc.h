// time_alloc.h — the one definition of a fitted track's snap cost and of the pieces of the
// segment-time descent that are plain arithmetic, shared by k_traj_snap_cost, k_time_grad and
// k_time_opt (time_alloc.hip) and by tests/host/time_alloc_main.cpp, so all compute the same
// bits.  Every operation is one IEEE fp64 operation (-ffp-contract=off).
//
// The cost is PolynomialOptimization::computeCost (external/poly_traj/include/
// mav_trajectory_generation/impl/polynomial_optimization_linear_impl.h:123-140):
//   J = 0.5 * sum_seg sum_dim c^T Q(T) c
// with Q of computeQuadraticCostJacobian (impl :567-583) for derivative 4:
//   Q[a][b] = B4[a] B4[b] T^(a+b-7) 2 / (a+b-7)  for a, b >= 4, else 0,  B4[j] = j! / (j-4)!
// (so J is the integral of the squared snap over the track).
//
// Order of the arithmetic (what "the same bits" means):
//   powers    tp[1] = T, tp[e] = tp[e-1] * T, e = 2..11
//   constant  kq(a, b) = (B4[a] * B4[b] * 2) / (a+b-7): the product is an exact integer
//             below 2^25, the quotient is rounded once
//   poly      s = 0; for a = 4..9, for b = 4..9: s = s + (c[a] * (kq(a, b) * tp[a+b-7])) * c[b]
//             (36 products per polynomial)
//   track     polynomial q = 3 * segment + axis.  part[l] (l = 0..63) = the costs of the
//             polynomials q = l, l + 64, ... added in that order from 0; then the 64 parts are
//             folded: for off = 32, 16, .., 1: part[i] = part[i] + part[i + off] (i < off);
//             J = 0.5 * part[0].  On the device a lane holds a part and the fold is the xor
//             butterfly (a + b is b + a bit for bit, so lane 0 holds the same value).
//
// A track is invalid (status -1, cost NaN) when it has no segment, a segment time that is not
// > 0 or not finite, or a non-finite coefficient: track_invalid's rule (feasibility.hip).
//
// The descent's arithmetic (the rule itself is in DESIGN.md section 4 and include/epp.h):
//   variant n of the Mellinger gradient: T_i + h for i = n, T_i - h / (M - 1) for i != n,
//   each clamped from below at t_min (getCostAndGradientMellinger, impl/
//   polynomial_optimization_nonlinear_impl.h:286-364; the reference's h and t_min are 0.1);
//   direction d_i = g_i - (sum_{n != i} g_n) / (M - 1), the sum taken in the order of n.
//
// Plain C++ apart from the HIP qualifiers.
#pragma once

#include <cmath>

#include "poly_deriv.h"

namespace epp {

constexpr int kCostLanes = 64;   // parts of a track's cost (one per lane of a wavefront)
constexpr int kCostPowers = 12;  // tp[0..11]; tp[0] is not used

// B4[a] * B4[b] * 2 / (a + b - 7)
EPP_PD_FN constexpr double snap_q_const(int a, int b) {
    return (falling<4>(a) * falling<4>(b) * 2.0) / (double)(a + b - 7);
}

EPP_PD_FN void snap_powers(double T, double (&tp)[kCostPowers]) {
    tp[0] = 1.0;
    tp[1] = T;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 2; e < kCostPowers; ++e) tp[e] = tp[e - 1] * T;
}

// c^T Q(T) c of one polynomial (c: 10 coefficients, increasing powers)
EPP_PD_FN double poly_snap_cost(const double* c, const double (&tp)[kCostPowers]) {
    double s = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 4; a < kDerivCoeffs; ++a)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int b = 4; b < kDerivCoeffs; ++b) s = s + (c[a] * (snap_q_const(a, b) * tp[a + b - 7])) * c[b];
    return s;
}

// part l of a track's cost: its polynomials l, l + 64, ... in order
EPP_PD_FN double snap_cost_part(const double* T, const double* C, int M, int l) {
    double part = 0.0;
    for (int q = l; q < 3 * M; q += kCostLanes) {
        double tp[kCostPowers];
        snap_powers(T[q / 3], tp);
        part = part + poly_snap_cost(C + (size_t)q * kDerivCoeffs, tp);
    }
    return part;
}

EPP_PD_FN bool snap_time_bad(double x) { return !(x > 0.0) || !std::isfinite(x); }

// the host's whole-track statement of what a wavefront does: J, or NaN for an invalid track
inline double snap_cost_track(const double* T, const double* C, int M, int* status = nullptr) {
    bool bad = M < 1;
    for (int i = 0; i < M && !bad; ++i) bad = snap_time_bad(T[i]);
    for (int i = 0; i < M * 3 * kDerivCoeffs && !bad; ++i) bad = !std::isfinite(C[i]);
    if (status) *status = bad ? -1 : 0;
    if (bad) return NAN;
    double part[kCostLanes];
    for (int l = 0; l < kCostLanes; ++l) part[l] = snap_cost_part(T, C, M, l);
    for (int off = kCostLanes / 2; off >= 1; off >>= 1)
        for (int i = 0; i < off; ++i) part[i] = part[i] + part[i + off];
    return 0.5 * part[0];
}

// entry i of variant n of the Mellinger gradient's segment times (M >= 2)
EPP_PD_FN double mellinger_time(double Ti, int i, int n, int M, double h, double t_min) {
    const double t = i == n ? Ti + h : Ti - h / ((double)M - 1.0);
    return t > t_min ? t : t_min;  // std::max(kOptimizationTimeLowerBound, t)
}

// entry i of the descent direction d = sum_n g_n u_n, u_n = e_n - (1 / (M - 1)) sum_{i != n} e_i
EPP_PD_FN double descent_direction(const double* g, int i, int M) {
    double s = 0.0;
    for (int n = 0; n < M; ++n)
        if (n != i) s = s + g[n];
    return g[i] - s / ((double)M - 1.0);
}

}  // namespace epp
