// feasibility.hip — peak speed / acceleration of min-snap trajectories and the uniform
// time scaling that brings them within v_max / a_max, batched over tracks, for gfx950.
//
// Reference: Trajectory::computeMaxVelocityAndAcceleration
// (external/poly_traj/src/trajectory.cpp:344-361, :191-227) over the per-segment magnitude
// extrema of src/segment.cpp:83-185, Trajectory::scaleSegmentTimesToMeetConstraints
// (src/trajectory.cpp:385-429) and Polynomial::scalePolynomialInTime (src/polynomial.cpp:199-205).
//
// The extrema of |p^(k)(t)| (Euclidean norm over x, y, z) on a segment are its two ends and
// the roots of g_k(t) = sum_d p_d^(k)(t) p_d^(k+1)(t), half the derivative of the squared
// magnitude.  The reference convolves the two derivative polynomials into one of degree 15
// and takes its Jenkins-Traub roots; here g_k is never expanded: it is evaluated as three
// products of Horner evaluations, and its sign changes are bracketed on a grid and bisected.
//
// One workgroup (4 wavefronts) per track, the wavefronts striding over the track's
// segments; one wavefront per segment.  Lane i owns [T i/64, T (i+1)/64]: it evaluates
// g_1, g_2 and the two squared magnitudes at its left end, takes g at its right end from
// lane i+1 (lane 63: evaluated at T; T (63+1)/64 is T exactly), and holds a maximum
// bracket of g_k when g_k(left) > 0 and g_k(right) <= 0.  Bracketing lanes bisect (both
// derivatives in the same loop) until the bracket cannot be split any more, at most
// kMaxBisect rounds (a bracket T 2^-6 wide is then T 2^-58 wide); the loop ends on a wave
// vote.  The root taken is the bracket's right end (g <= 0), so a root that lies exactly
// on a grid point is that grid point.  A subinterval that holds two roots of g shows no
// sign change and is not searched: the error is the height of a bump narrower
// than T/64.  Candidates (left end, root, and T for lane 63) are reduced by (magnitude,
// time) with ties to the earlier time: over the wave by a butterfly, over a wave's segments
// in registers, over the waves through LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "epp_internal.h"
#include "launch_helpers.h"
#include "poly_deriv.h"

namespace epp {
namespace {

constexpr int N = kDerivCoeffs;  // (falling<K>, deriv<K>: poly_deriv.h)
constexpr int kWave = 64;
constexpr int kFeasWaves = 4;
constexpr int kFeasBlock = kFeasWaves * kWave;
constexpr int kMaxBisect = 52;
constexpr int kMaxScaleRounds = 20;   // kMaxCounter, trajectory.cpp:388
constexpr double kScaleTol = 1e-3;    // kTolerance, trajectory.cpp:389

struct Seg3 {
    double c[3][N];
};

__device__ __forceinline__ void load_seg(Seg3& s, const double* p) {
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int j = 0; j < N; ++j) s.c[d][j] = p[d * N + j];
}

// |v|^2, |a|^2, g_1 and g_2 at t (the p'' evaluations are shared)
__device__ __forceinline__ void eval_all(const Seg3& s, double t, double& v2, double& a2, double& g1, double& g2) {
    v2 = a2 = g1 = g2 = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double p1 = deriv<1>(s.c[d], t), p2 = deriv<2>(s.c[d], t), p3 = deriv<3>(s.c[d], t);
        v2 += p1 * p1;
        a2 += p2 * p2;
        g1 += p1 * p2;
        g2 += p2 * p3;
    }
}
template <int K>
__device__ __forceinline__ double eval_g(const Seg3& s, double t) {
    double g = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) g += deriv<K>(s.c[d], t) * deriv<K + 1>(s.c[d], t);
    return g;
}
template <int K>
__device__ __forceinline__ double eval_sq(const Seg3& s, double t) {
    double m = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double p = deriv<K>(s.c[d], t);
        m += p * p;
    }
    return m;
}

// a candidate maximum: squared magnitude and time; the larger value wins, ties go to the
// earlier time (a NaN never wins)
struct Cand {
    double m, t;
};
__device__ __forceinline__ void take(Cand& best, double m, double t) {
    if (m > best.m || (m == best.m && t < best.t)) {
        best.m = m;
        best.t = t;
    }
}
__device__ __forceinline__ void wave_max(Cand& c) {
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        const double m = __shfl_xor(c.m, off, kWave), t = __shfl_xor(c.t, off, kWave);
        take(c, m, t);
    }
}

struct Peaks {
    double v, tv, a, ta;
};

// The peaks of one track by the whole workgroup (every thread returns them).  T: the M
// segment times, C: M x 3 x 10 coefficients.  s_part: kFeasWaves x 4 doubles of LDS; the
// caller's next use of it must follow a barrier (the one that ends this function covers
// the reads).
__device__ __forceinline__ Peaks track_peaks(const double* T, const double* C, int M, double (*s_part)[4]) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    Cand bv{-1.0, 0.0}, ba{-1.0, 0.0};
    double start = 0.0;  // sum of the earlier segment times, in order (as Trajectory accumulates them)
    int summed = 0;
    for (int s = wave; s < M; s += kFeasWaves) {
        for (; summed < s; ++summed) start += T[summed];
        const double Ts = T[s];
        Seg3 sg;
        load_seg(sg, C + (size_t)s * 3 * N);
        const double tl = Ts * ((double)lane * (1.0 / kWave));
        const double tr = Ts * ((double)(lane + 1) * (1.0 / kWave));  // lane 63: Ts itself
        double v2, a2, g1, g2;
        eval_all(sg, tl, v2, a2, g1, g2);
        double g1r = __shfl_down(g1, 1, kWave), g2r = __shfl_down(g2, 1, kWave);
        Cand cv{v2, tl}, ca{a2, tl};
        if (lane == kWave - 1) {
            double v2e, a2e;
            eval_all(sg, Ts, v2e, a2e, g1r, g2r);
            take(cv, v2e, Ts);
            take(ca, a2e, Ts);
        }
        const bool br1 = g1 > 0.0 && g1r <= 0.0, br2 = g2 > 0.0 && g2r <= 0.0;
        double lo1 = tl, hi1 = tr, lo2 = tl, hi2 = tr;
        bool act1 = br1, act2 = br2;
        for (int it = 0; it < kMaxBisect; ++it) {
            if (!__any(act1 || act2)) break;  // wave-uniform exit
            if (act1) {
                const double mid = 0.5 * (lo1 + hi1);
                if (mid > lo1 && mid < hi1) {
                    if (eval_g<1>(sg, mid) > 0.0) lo1 = mid;
                    else hi1 = mid;
                } else {
                    act1 = false;
                }
            }
            if (act2) {
                const double mid = 0.5 * (lo2 + hi2);
                if (mid > lo2 && mid < hi2) {
                    if (eval_g<2>(sg, mid) > 0.0) lo2 = mid;
                    else hi2 = mid;
                } else {
                    act2 = false;
                }
            }
        }
        if (br1) take(cv, eval_sq<1>(sg, hi1), hi1);
        if (br2) take(ca, eval_sq<2>(sg, hi2), hi2);
        wave_max(cv);
        wave_max(ca);
        take(bv, cv.m, start + cv.t);
        take(ba, ca.m, start + ca.t);
    }
    if (lane == 0) {
        s_part[wave][0] = bv.m;
        s_part[wave][1] = bv.t;
        s_part[wave][2] = ba.m;
        s_part[wave][3] = ba.t;
    }
    __syncthreads();
    Cand rv{-1.0, 0.0}, ra{-1.0, 0.0};
#pragma unroll
    for (int w = 0; w < kFeasWaves; ++w) {
        take(rv, s_part[w][0], s_part[w][1]);
        take(ra, s_part[w][2], s_part[w][3]);
    }
    __syncthreads();
    return Peaks{sqrt(rv.m), rv.t, sqrt(ra.m), ra.t};
}

// status -1: fewer than one segment, a segment time <= 0, or non-finite input (workgroup-uniform)
__device__ __forceinline__ bool track_invalid(const double* T, const double* C, int M) {
    int bad = M < 1;
    if (!bad) {
        for (int i = threadIdx.x; i < M; i += kFeasBlock) {
            const double x = T[i];
            bad |= !(x > 0.0) || !isfinite(x);
        }
        for (int i = threadIdx.x; i < M * 3 * N; i += kFeasBlock) bad |= !isfinite(C[i]);
    }
    return __syncthreads_or(bad) != 0;
}

__global__ __launch_bounds__(kFeasBlock) void k_traj_peaks(const double* __restrict__ seg_times,
                                                           const double* __restrict__ coeffs,
                                                           const int32_t* __restrict__ wp_off, int n_tracks,
                                                           double* __restrict__ peaks, int32_t* __restrict__ status) {
    __shared__ double s_part[kFeasWaves][4];
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int seg0 = wp_off[t] - t;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    const double* T = seg_times + seg0;
    const double* C = coeffs + (size_t)seg0 * 3 * N;
    if (track_invalid(T, C, M)) {
        if (threadIdx.x < 4) peaks[(size_t)t * 4 + threadIdx.x] = NAN;
        if (threadIdx.x == 0 && status) status[t] = -1;
        return;
    }
    const Peaks p = track_peaks(T, C, M, s_part);
    if (threadIdx.x == 0) {
        double* o = peaks + (size_t)t * 4;
        o[0] = p.v;
        o[1] = p.tv;
        o[2] = p.a;
        o[3] = p.ta;
        if (status) status[t] = 0;
    }
}

// Trajectory::scaleSegmentTimesToMeetConstraints per track, in place, the whole loop in one
// launch.  (seg_times and coeffs are read and written by the workgroup: no __restrict__ /
// const, so every load of them is a vector load ordered by the barriers.)
__global__ __launch_bounds__(kFeasBlock) void k_traj_scale(double* seg_times, double* coeffs,
                                                           const int32_t* __restrict__ wp_off, int n_tracks,
                                                           double v_max, double a_max, double* __restrict__ scale,
                                                           int32_t* __restrict__ status) {
    __shared__ double s_part[kFeasWaves][4];
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int seg0 = wp_off[t] - t;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    double* T = seg_times + seg0;
    double* C = coeffs + (size_t)seg0 * 3 * N;
    if (track_invalid(T, C, M)) {
        if (threadIdx.x == 0) {
            scale[t] = 1.0;
            if (status) status[t] = -1;
        }
        return;
    }
    double product = 1.0;
    int st = 1;
    for (int round = 0; round < kMaxScaleRounds; ++round) {
        const Peaks p = track_peaks(T, C, M, s_part);
        const double vv = p.v / v_max, av = p.a / a_max;
        if (vv <= 1.0 + kScaleTol && av <= 1.0 + kScaleTol) {
            st = 0;
            break;
        }
        const double s = fmax(1.0, fmax(vv, sqrt(av)));
        const double inv = 1.0 / s;
        for (int i = threadIdx.x; i < M; i += kFeasBlock) T[i] = T[i] * s;
        for (int q = threadIdx.x; q < M * 3; q += kFeasBlock)  // scalePolynomialInTime(1 / s)
            scale_polynomial_in_time(C + (size_t)q * N, inv);
        product = product * s;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        scale[t] = product;
        if (status) status[t] = st;
    }
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_traj_peaks(const double* seg_times, const double* coeffs, const int32_t* wp_offsets, int32_t n_tracks,
                          double* peaks, int32_t* status, void* stream) {
    if (n_tracks < 0 || (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !peaks))) {
        set_error("epp_traj_peaks: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    hipLaunchKernelGGL(k_traj_peaks, dim3(n_tracks), dim3(kFeasBlock), 0, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, n_tracks, peaks, status);
    return launch_error("epp_traj_peaks");
}

epp_status epp_traj_scale_to_limits(double* seg_times, double* coeffs, const int32_t* wp_offsets, int32_t n_tracks,
                                    double v_max, double a_max, double* scale, int32_t* status, void* stream) {
    if (n_tracks < 0 || (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !scale))) {
        set_error("epp_traj_scale_to_limits: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (!(v_max > 0.0) || !(a_max > 0.0)) {
        set_error("epp_traj_scale_to_limits: v_max and a_max must be greater than zero");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    hipLaunchKernelGGL(k_traj_scale, dim3(n_tracks), dim3(kFeasBlock), 0, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, n_tracks, v_max, a_max, scale, status);
    return launch_error("epp_traj_scale_to_limits");
}

}  // extern "C"
