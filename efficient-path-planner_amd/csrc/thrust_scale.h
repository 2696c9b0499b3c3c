// thrust_scale.h — the one definition of the time scaling that brings a fitted track within
// thrust, body-rate and tilt limits, shared by k_traj_thrust_grid and k_traj_thrust_scale
// (thrust_scale.hip) and by tests/thrust_scale_host.cpp, so all compute the same bits.  It
// extends Trajectory::scaleSegmentTimesToMeetConstraints (external/poly_traj/src/
// trajectory.cpp:385-429), which stretches a track for |v| and |a| only; the quantities are
// thrust_rates.h's.  Every operation is one IEEE fp64 operation (-ffp-contract=off).
//
// Grid points (those k_traj_peaks looks at): segment m with time T_m contributes
// tau_i = T_m * (i * (1 / 64)) for i = 0..63 and tau = T_m itself: 65 points.  At each,
// a = p''(tau) and j = p'''(tau) of the INPUT track per axis, by deriv<2> and deriv<3>
// (poly_deriv.h).  A point's time from the track's start is the sum of the earlier segment
// times, accumulated in order, plus tau.
//
// The track at scale s, x_new(s t) = x_old(t):  s2 = s * s;  s3 = s2 * s;  a_s = a / s2 and
// j_s = j / s3 componentwise -- divisions, not reciprocals: for the dyadic s the search visits,
// s2 and s3 are exact, so a_s and j_s are the correctly rounded quotients -- then
// thrust_rates(a_s, j_s, g).
//
// A point violates when thrust < f_min (bit 0), thrust > f_max (bit 1), rate > rate_max
// (bit 2) or cos_tilt < cos_tilt_min (bit 3).  A NaN violates nothing: the rule by which the
// extremes of epp_traj_thrust_rates_batch ignore a NaN, so "some point violates" is "an extreme
// over the points lies outside its limit".  A track is feasible at s when no grid point violates.
//
// The limits must satisfy 0 <= f_min < g < f_max, rate_max > 0, cos_tilt_min < 1, g finite and
// > 0 (thrust_limits_ok).  Then every finite track is feasible for large enough s: thrust -> g,
// rate -> 0, cos_tilt -> 1.  f_max = +inf, rate_max = +inf and cos_tilt_min <= -1 switch a limit
// off; f_min = 0 switches the lower thrust bound off.
//
// The search (thrust_scale_search): feasible at 1: scale 1, status 0.  Otherwise hi = 2, doubled
// while the track is infeasible at hi, up to 2^kMaxDoublings; infeasible there: status 1, scale
// 1.  Then lo = hi / 2 and exactly kBisectRounds rounds of mid = 0.5 * (lo + hi), hi = mid when
// feasible at mid, else lo = mid; the answer is hi.  Every s visited is dyadic with at most 13
// significant bits, so this arithmetic is exact, and hi / lo <= 1 + 2^-12.
//
// Only f_max is monotone in s (|F|^2 is a convex quadratic in 1 / s^2 that holds at 0).  f_min,
// the rate and the tilt are not: a track can be feasible at a small s with its thrust axis
// pointing down and infeasible at a larger one.  So the answer is A feasible s >= 1 with an
// infeasible s within 2^-12 below it (or exactly 1), not a proven minimum, and a track that is
// feasible at 1 is taken as it is.  Like epp_traj_peaks the check looks at 65 points per
// segment: a bump narrower than T / 64 can be missed, and the rows every dt of the scaled track
// are other points than the grid (a caller who needs the rows' answer runs
// epp_traj_thrust_rates_batch on the result).  Scaling alters a non-zero start velocity.
//
// The apply is one round of k_traj_scale: T[i] = T[i] * s, every polynomial through
// scale_polynomial_in_time(1 / s) (poly_deriv.h).
//
// Plain C++ apart from the HIP qualifiers; the *_track functions are the host's whole-track
// statement of what the kernels do with one workgroup.
#pragma once

#include "poly_deriv.h"
#include "thrust_rates.h"

namespace epp {

constexpr int kGridPoints = 64;     // per segment, and tau = T besides
constexpr int kMaxDoublings = 10;   // hi = 2 .. 1024
constexpr int kBisectRounds = 12;

enum : int { kViolFmin = 1, kViolFmax = 2, kViolRate = 4, kViolTilt = 8 };

struct ThrustLimits {
    double g, f_min, f_max, rate_max, cos_tilt_min;
};

// (every comparison is false for a NaN, so a NaN limit fails)
EPP_TR_FN bool thrust_limits_ok(const ThrustLimits& L) {
    return L.g > 0.0 && L.g < HUGE_VAL && L.f_min >= 0.0 && L.f_min < L.g && L.g < L.f_max && L.rate_max > 0.0 &&
           L.cos_tilt_min < 1.0;
}

// grid point i of a segment of time T: i = 0..63, and i = 64 is T itself
EPP_TR_FN double grid_tau(double T, int i) { return i < kGridPoints ? T * ((double)i * (1.0 / kGridPoints)) : T; }

// a = p''(tau), j = p'''(tau) per axis; cs: the segment's 3 x 10 coefficients
EPP_TR_FN void grid_point(const double* cs, double tau, double (&a)[3], double (&j)[3]) {
    for (int d = 0; d < 3; ++d) {
        double c[kDerivCoeffs];
        for (int n = 0; n < kDerivCoeffs; ++n) c[n] = cs[d * kDerivCoeffs + n];
        a[d] = deriv<2>(c, tau);
        j[d] = deriv<3>(c, tau);
    }
}

// the quantities of a point at scale s, given s2 = s * s and s3 = s2 * s
EPP_TR_FN ThrustRates scaled_thrust_rates(const double (&a)[3], const double (&j)[3], double s2, double s3, double g) {
    return thrust_rates(a[0] / s2, a[1] / s2, a[2] / s2, j[0] / s3, j[1] / s3, j[2] / s3, g);
}

EPP_TR_FN int thrust_violation(const ThrustRates& r, const ThrustLimits& L) {
    return (r.thrust < L.f_min ? kViolFmin : 0) | (r.thrust > L.f_max ? kViolFmax : 0) |
           (r.rate > L.rate_max ? kViolRate : 0) | (r.cos_tilt < L.cos_tilt_min ? kViolTilt : 0);
}

struct ThrustScale {
    double scale;
    int status;    // 0: feasible at scale; 1: infeasible at 2^kMaxDoublings (scale 1)
    int violated;  // the limits violated at s = 1
};

// violated_at(s): the OR of the grid points' violation bits at scale s (non-zero: infeasible).
// On the device every thread of the workgroup runs the search; violated_at is uniform.
template <class V>
EPP_TR_FN ThrustScale thrust_scale_search(V&& violated_at) {
    ThrustScale r{1.0, 0, violated_at(1.0)};
    if (!r.violated) return r;
    double hi = 2.0;
    for (int d = 1; violated_at(hi); ++d) {
        if (d == kMaxDoublings) {
            r.status = 1;
            return r;
        }
        hi = hi * 2.0;
    }
    double lo = hi * 0.5;
    for (int it = 0; it < kBisectRounds; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (violated_at(mid)) lo = mid;
        else hi = mid;
    }
    r.scale = hi;
    return r;
}

// status -1: fewer than one segment, a segment time <= 0, or non-finite input (track_invalid)
EPP_TR_FN bool thrust_track_invalid(const double* T, const double* C, int M) {
    if (M < 1) return true;
    for (int i = 0; i < M; ++i)
        if (!(T[i] > 0.0) || !(T[i] < HUGE_VAL)) return true;
    for (int i = 0; i < M * 3 * kDerivCoeffs; ++i)
        if (!(C[i] - C[i] == 0.0)) return true;
    return false;
}

EPP_TR_FN int thrust_violation_track(const double* T, const double* C, int M, double s, const ThrustLimits& L) {
    const double s2 = s * s, s3 = s2 * s;
    int bits = 0;
    for (int m = 0; m < M; ++m)
        for (int i = 0; i <= kGridPoints; ++i) {
            double a[3], j[3];
            grid_point(C + (size_t)m * 3 * kDerivCoeffs, grid_tau(T[m], i), a, j);
            bits |= thrust_violation(scaled_thrust_rates(a, j, s2, s3, L.g), L);
        }
    return bits;
}

// epp_traj_scale_to_thrust_limits of one track, in place
EPP_TR_FN ThrustScale thrust_scale_track(double* T, double* C, int M, const ThrustLimits& L) {
    if (thrust_track_invalid(T, C, M)) return ThrustScale{1.0, -1, 0};
    const ThrustScale r = thrust_scale_search([&](double s) { return thrust_violation_track(T, C, M, s, L); });
    if (r.status == 0 && r.scale != 1.0) {
        const double inv = 1.0 / r.scale;
        for (int i = 0; i < M; ++i) T[i] = T[i] * r.scale;
        for (int q = 0; q < M * 3; ++q) scale_polynomial_in_time(C + (size_t)q * kDerivCoeffs, inv);
    }
    return r;
}

// one extreme: value and time; strict comparison, ties to the earlier time, a NaN never wins
struct GridBest {
    double v, t;
    template <bool MIN>
    EPP_TR_FN void take(double nv, double nt) {
        const bool better = (MIN ? nv < v : nv > v) || (nv == v && nt < t);
        v = better ? nv : v;
        t = better ? nt : t;
    }
};
struct GridExtremes {
    GridBest fmin, fmax, rmax, cmin;
    EPP_TR_FN void reset() {
        fmin = GridBest{HUGE_VAL, -1.0};
        fmax = GridBest{-HUGE_VAL, -1.0};
        rmax = GridBest{-HUGE_VAL, -1.0};
        cmin = GridBest{HUGE_VAL, -1.0};
    }
    EPP_TR_FN void take(const ThrustRates& r, double t) {
        fmin.take<true>(r.thrust, t);
        fmax.take<false>(r.thrust, t);
        rmax.take<false>(r.rate, t);
        cmin.take<true>(r.cos_tilt, t);
    }
    EPP_TR_FN void take(const GridExtremes& o) {
        fmin.take<true>(o.fmin.v, o.fmin.t);
        fmax.take<false>(o.fmax.v, o.fmax.t);
        rmax.take<false>(o.rmax.v, o.rmax.t);
        cmin.take<true>(o.cmin.v, o.cmin.t);
    }
    EPP_TR_FN void store(double* q) const {
        q[0] = fmin.v, q[1] = fmin.t, q[2] = fmax.v, q[3] = fmax.t;
        q[4] = rmax.v, q[5] = rmax.t, q[6] = cmin.v, q[7] = cmin.t;
    }
};

// epp_traj_thrust_grid_batch of one track: out[8] at scale s, times in the input track's time
EPP_TR_FN void thrust_grid_track(const double* T, const double* C, int M, double s, double g, double* out) {
    GridExtremes e;
    e.reset();
    if (!thrust_track_invalid(T, C, M)) {
        const double s2 = s * s, s3 = s2 * s;
        double start = 0.0;
        for (int m = 0; m < M; ++m) {
            for (int i = 0; i <= kGridPoints; ++i) {
                const double tau = grid_tau(T[m], i);
                double a[3], j[3];
                grid_point(C + (size_t)m * 3 * kDerivCoeffs, tau, a, j);
                e.take(scaled_thrust_rates(a, j, s2, s3, g), start + tau);
            }
            start += T[m];
        }
    }
    e.store(out);
}

}  // namespace epp
