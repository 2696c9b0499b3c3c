// thrust_scale.hip — time scaling of fitted tracks to thrust, body-rate and tilt limits,
// batched over tracks, for gfx950: epp_traj_thrust_grid_batch (the four extremes over the grid
// points at a per-track scale) and epp_traj_scale_to_thrust_limits (the whole search and the
// apply in one launch).  It extends
//
//   Trajectory::scaleSegmentTimesToMeetConstraints   external/poly_traj/src/trajectory.cpp:385-429
//
// which stretches a track for |v| and |a| only (k_traj_scale, feasibility.hip).  The thrust
// |a / s^2 + g e_z| is no power of s, so there is no closed form: the scale is bracketed and
// bisected.  The grid points, the quantities at a scale, the violation rule, the search and
// the apply are thrust_scale.h's, one definition for the kernels and the host.
//
// Both kernels have the shape of k_traj_peaks: one workgroup (4 wavefronts) per track, the
// wavefronts striding over the track's segments, lane i owning grid point i = T i/64 and lane
// 63 also tau = T; an invalid track (fewer than one segment, a time <= 0, non-finite input)
// is found by the whole workgroup first.
//
// k_traj_thrust_grid reduces (value, time) with ties to the earlier time: over the wave by a
// butterfly, over a wave's segments in registers, over the waves through LDS.
//
// k_traj_thrust_scale: a feasibility evaluation is one OR of the lanes' violation bits over
// the workgroup (__syncthreads_or), at most 1 + 10 + 12 of them per track; the control flow of
// the search is workgroup-uniform, so every thread runs it.  A wave keeps (a, j) of the points
// of its first kHeld segments in registers (a track of up to kHeld * 4 segments never reads
// its coefficients again) and recomputes them from the coefficients for the segments beyond.
// After the last evaluation's barrier the workgroup applies the scale in place.
#include <cmath>

#include "epp_internal.h"
#include "launch_helpers.h"
#include "thrust_scale.h"

namespace epp {
namespace {

constexpr int N = kDerivCoeffs;
constexpr int kWave = 64;
constexpr int kTsWaves = 4;
constexpr int kTsBlock = kTsWaves * kWave;
constexpr int kHeld = 2;  // segments per wave whose points stay in registers: 24 doubles
static_assert(kGridPoints == kWave, "lane i owns grid point i");

// status -1: fewer than one segment, a segment time <= 0, or non-finite input (workgroup-
// uniform; k_traj_peaks' rule)
__device__ __forceinline__ bool track_invalid(const double* T, const double* C, int M) {
    int bad = M < 1;
    if (!bad) {
        for (int i = threadIdx.x; i < M; i += kTsBlock) {
            const double x = T[i];
            bad |= !(x > 0.0) || !isfinite(x);
        }
        for (int i = threadIdx.x; i < M * 3 * N; i += kTsBlock) bad |= !isfinite(C[i]);
    }
    return __syncthreads_or(bad) != 0;
}

// a lane's points of one segment: grid point `lane`, and for lane 63 tau = T
struct SegPoints {
    double a[3], j[3], ae[3], je[3];
};
__device__ __forceinline__ void seg_points(const double* cs, double Ts, int lane, SegPoints& p) {
    grid_point(cs, grid_tau(Ts, lane), p.a, p.j);
#pragma unroll
    for (int d = 0; d < 3; ++d) p.ae[d] = p.je[d] = 0.0;
    if (lane == kWave - 1) grid_point(cs, Ts, p.ae, p.je);
}
__device__ __forceinline__ int seg_violation(const SegPoints& p, int lane, double s2, double s3,
                                             const ThrustLimits& L) {
    int bits = thrust_violation(scaled_thrust_rates(p.a, p.j, s2, s3, L.g), L);
    if (lane == kWave - 1) bits |= thrust_violation(scaled_thrust_rates(p.ae, p.je, s2, s3, L.g), L);
    return bits;
}

__device__ __forceinline__ void wave_reduce(GridExtremes& e) {
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) {
        GridExtremes o;
        o.fmin = GridBest{__shfl_xor(e.fmin.v, off, kWave), __shfl_xor(e.fmin.t, off, kWave)};
        o.fmax = GridBest{__shfl_xor(e.fmax.v, off, kWave), __shfl_xor(e.fmax.t, off, kWave)};
        o.rmax = GridBest{__shfl_xor(e.rmax.v, off, kWave), __shfl_xor(e.rmax.t, off, kWave)};
        o.cmin = GridBest{__shfl_xor(e.cmin.v, off, kWave), __shfl_xor(e.cmin.t, off, kWave)};
        e.take(o);
    }
}

__global__ __launch_bounds__(kTsBlock) void k_traj_thrust_grid(const double* __restrict__ seg_times,
                                                               const double* __restrict__ coeffs,
                                                               const int32_t* __restrict__ wp_off, int n_tracks,
                                                               const double* __restrict__ scale_in, double g,
                                                               double* __restrict__ out) {
    __shared__ double s_part[kTsWaves][8];
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int seg0 = wp_off[t] - t;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    const double* T = seg_times + seg0;
    const double* C = coeffs + (size_t)seg0 * 3 * N;
    GridExtremes e;
    e.reset();
    if (track_invalid(T, C, M)) {
        if (threadIdx.x == 0) e.store(out + (size_t)t * 8);
        return;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const double s = scale_in ? scale_in[t] : 1.0;
    const double s2 = s * s, s3 = s2 * s;
    double start = 0.0;  // sum of the earlier segment times, in order
    int summed = 0;
    for (int m = wave; m < M; m += kTsWaves) {
        for (; summed < m; ++summed) start += T[summed];
        const double Ts = T[m];
        SegPoints p;
        seg_points(C + (size_t)m * 3 * N, Ts, lane, p);
        e.take(scaled_thrust_rates(p.a, p.j, s2, s3, g), start + grid_tau(Ts, lane));
        if (lane == kWave - 1) e.take(scaled_thrust_rates(p.ae, p.je, s2, s3, g), start + Ts);
    }
    wave_reduce(e);
    if (lane == 0) e.store(s_part[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        GridExtremes r;
        r.reset();
#pragma unroll
        for (int w = 0; w < kTsWaves; ++w) {
            GridExtremes o;
            o.fmin = GridBest{s_part[w][0], s_part[w][1]};
            o.fmax = GridBest{s_part[w][2], s_part[w][3]};
            o.rmax = GridBest{s_part[w][4], s_part[w][5]};
            o.cmin = GridBest{s_part[w][6], s_part[w][7]};
            r.take(o);
        }
        r.store(out + (size_t)t * 8);
    }
}

// (seg_times and coeffs are read and written by the workgroup: no __restrict__ / const, so
// every load of them is a vector load ordered by the barriers.)
__global__ __launch_bounds__(kTsBlock) void k_traj_thrust_scale(double* seg_times, double* coeffs,
                                                                const int32_t* __restrict__ wp_off, int n_tracks,
                                                                ThrustLimits L, double* __restrict__ scale,
                                                                int32_t* __restrict__ status,
                                                                int32_t* __restrict__ violated) {
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int seg0 = wp_off[t] - t;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    double* T = seg_times + seg0;
    double* C = coeffs + (size_t)seg0 * 3 * N;
    if (track_invalid(T, C, M)) {
        if (threadIdx.x == 0) {
            scale[t] = 1.0;
            status[t] = -1;
            if (violated) violated[t] = 0;
        }
        return;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    SegPoints held[kHeld];
#pragma unroll
    for (int h = 0; h < kHeld; ++h) {
        const int m = wave + h * kTsWaves;
        if (m < M) seg_points(C + (size_t)m * 3 * N, T[m], lane, held[h]);
    }
    const ThrustScale r = thrust_scale_search([&](double s) -> int {
        const double s2 = s * s, s3 = s2 * s;
        int bits = 0;
#pragma unroll
        for (int h = 0; h < kHeld; ++h)
            if (wave + h * kTsWaves < M) bits |= seg_violation(held[h], lane, s2, s3, L);
        for (int m = wave + kHeld * kTsWaves; m < M; m += kTsWaves) {
            SegPoints p;
            seg_points(C + (size_t)m * 3 * N, T[m], lane, p);
            bits |= seg_violation(p, lane, s2, s3, L);
        }
        if (s != 1.0) return __syncthreads_or(bits);
        int all = 0;  // the first evaluation: which limits, one OR per bit
#pragma unroll
        for (int b = 1; b <= kViolTilt; b <<= 1) all |= __syncthreads_or(bits & b) ? b : 0;
        return all;
    });
    // (the last evaluation ended in a barrier: every read of T and C above is done)
    if (r.status == 0 && r.scale != 1.0) {
        const double s = r.scale, inv = 1.0 / s;
        for (int i = threadIdx.x; i < M; i += kTsBlock) T[i] = T[i] * s;
        for (int q = threadIdx.x; q < M * 3; q += kTsBlock)  // scalePolynomialInTime(1 / s)
            scale_polynomial_in_time(C + (size_t)q * N, inv);
    }
    if (threadIdx.x == 0) {
        scale[t] = r.scale;
        status[t] = r.status;
        if (violated) violated[t] = r.violated;
    }
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_traj_thrust_grid_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                                      int32_t n_tracks, const double* scale_in, double g, double* out, void* stream) {
    if (n_tracks < 0 || !std::isfinite(g) || (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !out))) {
        set_error("epp_traj_thrust_grid_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    hipLaunchKernelGGL(k_traj_thrust_grid, dim3(n_tracks), dim3(kTsBlock), 0, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, (int)n_tracks, scale_in, g, out);
    return launch_error("epp_traj_thrust_grid_batch");
}

epp_status epp_traj_scale_to_thrust_limits(double* seg_times, double* coeffs, const int32_t* wp_offsets,
                                           int32_t n_tracks, double g, double f_min, double f_max, double rate_max,
                                           double cos_tilt_min, double* scale, int32_t* status, int32_t* violated,
                                           void* stream) {
    if (n_tracks < 0 || (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !scale || !status))) {
        set_error("epp_traj_scale_to_thrust_limits: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const ThrustLimits L{g, f_min, f_max, rate_max, cos_tilt_min};
    if (!thrust_limits_ok(L)) {
        set_error(
            "epp_traj_scale_to_thrust_limits: the limits must satisfy 0 <= f_min < g < f_max, rate_max > 0, "
            "cos_tilt_min < 1, g finite");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    hipLaunchKernelGGL(k_traj_thrust_scale, dim3(n_tracks), dim3(kTsBlock), 0, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, (int)n_tracks, L, scale, status, violated);
    return launch_error("epp_traj_scale_to_thrust_limits");
}

}  // extern "C"
