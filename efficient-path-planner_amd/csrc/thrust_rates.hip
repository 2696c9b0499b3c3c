// thrust_rates.hip — what a quadrotor must do to fly fitted tracks (gfx950): the thrust, the
// roll / pitch body rate and the tilt of samples (epp_thrust_rates), their extremes over the
// rows of fitted tracks straight from the coefficients (epp_traj_thrust_rates_batch), and the
// sampler of any derivative they rest on (epp_sample_derivative_batch):
//
//   Trajectory::evaluateRange(t_start, t_end, dt, derivative_order, ...)
//   external/poly_traj/src/trajectory.cpp:81-141
//
// The per-sample arithmetic is thrust_rates.h's; the rows, their times and the derivative
// values are traj_sample.h's (the recurrence, range_produce, poly_eval), so all three calls
// see the same bits.
//
// k_thrust_rates: one sample per lane, grid-stride.
//
// k_sample_deriv: the shape of k_sample_rows (minsnap.hip): one wave per track, lane 0 runs the
// time recurrence a chunk at a time, the wave evaluates the chunk with poly_eval and the
// falling-factorial table in LDS.  The table is filled from falling_factorial (exact small
// integers: the bits of the table k_sample_rows stages) and the segment times come from LDS up
// to kTcSegLds segments, through L2 beyond, so the launch needs nothing from the host: no
// track offsets read back, no constants uploaded.
//
// k_traj_thrust_rates: the walk of traj_walk.h with the check TcThrust, which never posts, so
// every chunk of every track is walked.
#include <algorithm>
#include <cmath>

#include "launch_helpers.h"
#include "thrust_rates.h"
#include "traj_walk.h"

namespace epp {
namespace {

constexpr int kTrBlock = 256;
constexpr int kMaxOrder = kPolyCoeffs - 1;

__global__ __launch_bounds__(kTrBlock) void k_thrust_rates(const double* __restrict__ acc,
                                                           const double* __restrict__ jerk, int64_t n, double g,
                                                           double* __restrict__ thrust, double* __restrict__ rate,
                                                           double* __restrict__ cos_tilt) {
    const int64_t stride = (int64_t)gridDim.x * kTrBlock;
    for (int64_t i = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; i < n; i += stride) {
        const ThrustRates r = thrust_rates(acc[3 * i], acc[3 * i + 1], acc[3 * i + 2], jerk[3 * i], jerk[3 * i + 1],
                                           jerk[3 * i + 2], g);
        thrust[i] = r.thrust;
        if (rate) rate[i] = r.rate;
        if (cos_tilt) cos_tilt[i] = r.cos_tilt;
    }
}

constexpr int kSdWave = 64;

__global__ __launch_bounds__(kSdWave) void k_sample_deriv(const double* __restrict__ seg_times,
                                                          const double* __restrict__ coeffs,
                                                          const int32_t* __restrict__ wp_off, int n_tracks, double dt,
                                                          int order, const int64_t* __restrict__ row_off,
                                                          double* __restrict__ values) {
    constexpr int N = kPolyCoeffs;
    __shared__ double sB[N * N], sT[kTcSegLds], s_tin[kRowChunk], s_tac[kRowChunk];
    __shared__ int s_seg[kRowChunk], s_cnt, s_done;
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int lane = threadIdx.x;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    if (M < 1) return;  // no segment, no row
    const int seg0 = wp_off[t] - t;
    const bool t_lds = M <= kTcSegLds;
    for (int e = lane; e < N * N; e += kSdWave) sB[e] = falling_factorial(e / N, e % N);
    if (t_lds)
        for (int i = lane; i < M; i += kSdWave) sT[i] = seg_times[seg0 + i];
    double* out = values + (row_off ? row_off[t] : 0) * 3;
    RangeIter it;
    __syncthreads();
    if (lane == 0) {
        it.init(t_lds ? sT : seg_times + seg0, M);
        s_done = 0;
    }
    int64_t base = 0;
    while (true) {
        if (lane == 0) s_cnt = range_produce(it, dt, kRowChunk, s_seg, s_tin, s_tac, s_done);
        __syncthreads();
        const int cnt = s_cnt, done = s_done;
        for (int j = lane; j < cnt; j += kSdWave) {
            const double* cs = coeffs + (size_t)(seg0 + s_seg[j]) * (3 * N);
            const double tin = s_tin[j];
            double* v = out + (base + j) * 3;
            for (int d = 0; d < 3; ++d) v[d] = poly_eval(sB, cs + d * N, tin, order);
        }
        base += cnt;
        __syncthreads();
        if (done) break;
    }
}

// The extremes of thrust, body rate and tilt over the rows.  A checking lane takes samples
// lane, + 64, ..., evaluates the acceleration and the jerk of each (six Horner evaluations,
// poly_eval_order: poly_eval's bits without the table) and keeps four bests (value, row, time)
// in registers across the chunks, updating on strict < or >: its rows ascend, so the earliest
// row wins within a lane, a NaN never updates and a +inf rate does.  At the track's end wave 1
// reduces each lexicographically by (value, row).
struct TtOut {
    double g;
    double* out;    // n_tracks x 8
    int64_t* rows;  // n_tracks x 4, may be NULL
};
struct TtBest {
    double v, time;
    long long row;
    __device__ __forceinline__ void reset(double identity) {
        v = identity;
        time = -1.0;
        row = -1;
    }
    __device__ __forceinline__ void take(bool better, double nv, long long nrow, double ntime) {
        v = better ? nv : v;
        row = better ? nrow : row;
        time = better ? ntime : time;
    }
    template <bool MIN>
    __device__ __forceinline__ void reduce() {
        for (int m = 32; m > 0; m >>= 1) {
            const double ov = __shfl_xor(v, m), otime = __shfl_xor(time, m);
            const long long orow = __shfl_xor(row, m);
            take((MIN ? ov < v : ov > v) || (ov == v && orow < row), ov, orow, otime);
        }
    }
};
struct TcThrust {
    TtOut o;
    TtBest fmin, fmax, rmax, cmin;  // wave 1: the lane's bests so far
    __device__ __forceinline__ void reset() {
        fmin.reset(HUGE_VAL);
        fmax.reset(-HUGE_VAL);
        rmax.reset(-HUGE_VAL);
        cmin.reset(HUGE_VAL);
    }
    __device__ __forceinline__ void begin() { reset(); }
    __device__ __forceinline__ void keep(const TcShared&, int) {}
    __device__ __forceinline__ void check(TcShared& s, int b, int cnt, int64_t base, int lane,
                                          const double* __restrict__ coeffs, int seg0) {
        for (int j = lane; j < cnt; j += kTcCheckers) {
            const double* cs = coeffs + (size_t)(seg0 + s.seg[b][j]) * (3 * kPolyCoeffs);
            const double tin = s.tin[b][j], tac = s.tac[b][j];
            double a[3], jk[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                a[d] = poly_eval_order<2>(cs + d * kPolyCoeffs, tin);
                jk[d] = poly_eval_order<3>(cs + d * kPolyCoeffs, tin);
            }
            const ThrustRates r = thrust_rates(a[0], a[1], a[2], jk[0], jk[1], jk[2], o.g);
            const long long row = base + j;
            fmin.take(r.thrust < fmin.v, r.thrust, row, tac);
            fmax.take(r.thrust > fmax.v, r.thrust, row, tac);
            rmax.take(r.rate > rmax.v, r.rate, row, tac);
            cmin.take(r.cos_tilt < cmin.v, r.cos_tilt, row, tac);
        }
    }
    __device__ __forceinline__ int row(int f) const { return f; }                           // (never posted:
    __device__ __forceinline__ double time(const TcShared&, int, int) const { return 0.0; }  //  never asked)
    __device__ __forceinline__ void posted(const TcShared&, int, int, const double* __restrict__, int) {}
    __device__ __forceinline__ void end(int t, int tid, bool walked, int64_t, double, int64_t* __restrict__,
                                        double* __restrict__) {
        if (tid < 64) return;  // (wave-uniform: wave 1 holds the bests)
        if (!walked) reset();  // no segment, no row
        fmin.reduce<true>();
        fmax.reduce<false>();
        rmax.reduce<false>();
        cmin.reduce<true>();
        if (tid == 64) {
            double* q = o.out + (size_t)t * 8;
            // the rows' time columns as epp_sample_batch writes them with t0 == NULL
            q[0] = fmin.v;
            q[1] = fmin.time + 0.0;
            q[2] = fmax.v;
            q[3] = fmax.time + 0.0;
            q[4] = rmax.v;
            q[5] = rmax.time + 0.0;
            q[6] = cmin.v;
            q[7] = cmin.time + 0.0;
            if (o.rows) {
                int64_t* r = o.rows + (size_t)t * 4;
                r[0] = fmin.row;
                r[1] = fmax.row;
                r[2] = rmax.row;
                r[3] = cmin.row;
            }
        }
    }
};

__global__ __launch_bounds__(kTcBlock) void k_traj_thrust_rates(const double* __restrict__ seg_times,
                                                                const double* __restrict__ coeffs,
                                                                const int32_t* __restrict__ wp_off, int n_tracks,
                                                                double dt, TtOut out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    TcThrust chk{out};
    chk.reset();
    tc_walk(*reinterpret_cast<TcShared*>(lds), seg_times, coeffs, wp_off, n_tracks, dt, nullptr, nullptr, chk);
}

bool tracks_ok(const double* seg_times, const double* coeffs, const int32_t* wp_offsets, int32_t n_tracks, double dt) {
    return n_tracks >= 0 && dt > 0 && std::isfinite(dt) && (n_tracks == 0 || (seg_times && coeffs && wp_offsets));
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_sample_derivative_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                                       int32_t n_tracks, double dt, int32_t order, const int64_t* row_offsets,
                                       double* values, void* stream) {
    if (!tracks_ok(seg_times, coeffs, wp_offsets, n_tracks, dt) || order < 0 || order > kMaxOrder ||
        (n_tracks > 0 && !values)) {
        set_error("epp_sample_derivative_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    hipLaunchKernelGGL(k_sample_deriv, dim3(n_tracks), dim3(kSdWave), 0, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, (int)n_tracks, dt, (int)order, row_offsets, values);
    return launch_error("epp_sample_derivative_batch");
}

epp_status epp_thrust_rates(const double* acc, const double* jerk, int64_t n, double g, double* thrust, double* rate,
                            double* cos_tilt, void* stream) {
    if (n < 0 || !std::isfinite(g) || (n > 0 && (!acc || !jerk || !thrust))) {
        set_error("epp_thrust_rates: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return EPP_OK;
    const int64_t groups = (n + kTrBlock - 1) / kTrBlock;
    const int grid = (int)std::min<int64_t>(groups, (int64_t)cu_count() * 8);
    hipLaunchKernelGGL(k_thrust_rates, dim3(grid), dim3(kTrBlock), 0, (hipStream_t)stream, acc, jerk, n, g, thrust,
                       rate, cos_tilt);
    return launch_error("epp_thrust_rates");
}

epp_status epp_traj_thrust_rates_batch(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                                       int32_t n_tracks, double dt, double g, double* out, int64_t* rows,
                                       void* stream) {
    if (!tracks_ok(seg_times, coeffs, wp_offsets, n_tracks, dt) || !std::isfinite(g) || (n_tracks > 0 && !out)) {
        set_error("epp_traj_thrust_rates_batch: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    const uint32_t shm = kTcSharedBytes;
    // persistent grid: as many workgroups as stay resident (trajcheck.hip: 8 per CU by registers, fewer by LDS)
    const int per_cu = std::max(1, std::min<int>(8, (int)((160u * 1024u) / shm)));
    const int grid = (int)std::min<int64_t>(n_tracks, (int64_t)cu_count() * per_cu);
    hipLaunchKernelGGL(k_traj_thrust_rates, dim3(grid), dim3(kTcBlock), shm, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, (int)n_tracks, dt, TtOut{g, out, rows});
    return launch_error("epp_traj_thrust_rates_batch");
}

}  // extern "C"
