// time_alloc.hip — the segment-time allocation of fitted tracks for gfx950: the snap cost from
// coefficients (k_traj_snap_cost), the cost and Mellinger gradient of a time allocation
// (k_time_grad, k_time_quot) and the descent over the segment times at constant total time
// (k_time_opt), batched over tracks.
//
// Reference: PolynomialOptimization::computeCost (external/poly_traj/include/
// mav_trajectory_generation/impl/polynomial_optimization_linear_impl.h:123-140) and
// getCostAndGradientMellinger (impl/polynomial_optimization_nonlinear_impl.h:286-364); the
// iteration itself the reference leaves to NLopt (and ships commented out), so the descent
// rule is this library's (include/epp.h).
//
// Every cost J(T) is solve_track (minsnap_solve.h) at the times T with the refinement step on,
// then the cost of time_alloc.h over the coefficients that solve wrote.  One wavefront per
// workgroup, as k_minsnap: the solve's block elimination is one wavefront's work, and the cost
// is one butterfly over its lanes.
//   k_time_grad   one workgroup per (track, variant), variant 0 the unperturbed times: the
//                 sum (M + 1) solves of a launch are independent
//   k_time_opt    one workgroup per track, the whole loop in one launch: the solves of one
//                 track run one after another; the batch is the parallelism
// A variant's / trial's coefficients go to a global workspace and are read back by the same
// workgroup behind a barrier: that pointer carries no __restrict__ or const, so every load of
// it is a vector load ordered by the barrier (see k_traj_scale, feasibility.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "cached_ws.h"
#include "collision_common.h"
#include "epp.h"
#include "launch_helpers.h"
#include "minsnap_kernels.h"
#include "minsnap_solve.h"
#include "time_alloc.h"

namespace epp {
namespace {

constexpr int kB = kWave;  // threads per workgroup, all kernels here

// J of one track by the wavefront (every lane returns it): time_alloc.h's parts, one per lane,
// folded by the xor butterfly
__device__ __forceinline__ double wave_snap_cost(const double* T, const double* C, int M) {
    double part = snap_cost_part(T, C, M, (int)threadIdx.x);
#pragma unroll
    for (int off = kCostLanes / 2; off >= 1; off >>= 1) part = part + __shfl_xor(part, off, kWave);
    return 0.5 * part;
}

__global__ __launch_bounds__(kB) void k_traj_snap_cost(const double* __restrict__ seg_times,
                                                       const double* __restrict__ coeffs,
                                                       const int32_t* __restrict__ wp_off, int n_tracks,
                                                       double* __restrict__ cost, int32_t* __restrict__ status) {
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int seg0 = wp_off[t] - t;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    const double* T = seg_times + seg0;
    const double* C = coeffs + (size_t)seg0 * 3 * N;
    // track_invalid's rule (feasibility.hip): workgroup-uniform
    int bad = M < 1;
    if (!bad) {
        for (int i = threadIdx.x; i < M; i += kB) bad |= snap_time_bad(T[i]);
        for (int i = threadIdx.x; i < M * 3 * N; i += kB) bad |= !isfinite(C[i]);
    }
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0) {
            cost[t] = NAN;
            if (status) status[t] = -1;
        }
        return;
    }
    const double J = wave_snap_cost(T, C, M);
    if (threadIdx.x == 0) {
        cost[t] = J;
        if (status) status[t] = 0;
    }
}

// The LDS of a solving workgroup: [error flag (16 bytes) | constants | segment scratch (LDS) |
// vertex values (vertex_doubles) | `extra` doubles of the kernel's own]
struct SolveLds {
    int* s_err;
    double *kc, *scr, *dv, *rhs, *Tm, *xch, *extra;
};
template <bool LDS>
__device__ __forceinline__ SolveLds solve_lds(double* smem, int M, double* gscr) {
    SolveLds L;
    L.s_err = reinterpret_cast<int*>(smem);
    L.kc = smem + 2;
    double* sm = L.kc + kNC;
    L.scr = LDS ? sm : gscr;
    L.dv = LDS ? sm + (size_t)M * Seg::kSize : sm;
    L.rhs = L.dv + (size_t)(M + 1) * 15;
    L.Tm = L.rhs + (size_t)(M + 1) * 12;
    L.xch = L.Tm + M;
    L.extra = L.dv + vertex_doubles(M);
    return L;
}
size_t solve_lds_bytes(bool lds, int max_m, int extra) {
    return ((lds ? (size_t)max_m * Seg::kSize : 0) + vertex_doubles(max_m) + 2 + kNC + (size_t)extra) * sizeof(double);
}

// Workgroup (track, variant) = (blockIdx.x, blockIdx.y); stride = the batch's largest M + 1.
// Variant v of track k owns segments [seg0 * stride + v * M, + M) of ws_c (x 30 doubles) and of
// gscratch (x Seg::kSize, long tracks), and slot k * stride + v of Jv / stv.
template <bool LDS>
__global__ __launch_bounds__(kB) void k_time_grad(const double* __restrict__ wp, const int32_t* __restrict__ wp_off,
                                                  int n_tracks, const double* __restrict__ v0,
                                                  const double* __restrict__ a0, const double* __restrict__ seg_times,
                                                  double h, double t_min, int stride, double* ws_c, double* gscratch,
                                                  double* __restrict__ Jv, int32_t* __restrict__ stv) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int track = blockIdx.x, variant = blockIdx.y;
    if (track >= n_tracks) return;
    const int w0 = wp_off[track];
    const int M = wp_off[track + 1] - w0 - 1;
    const int seg0 = w0 - track;
    if (variant > M || M < 1 || (M == 1 && variant > 0)) return;  // (k_time_quot answers for M < 1)
    const size_t base = (size_t)seg0 * stride + (size_t)variant * M;
    const SolveLds L = solve_lds<LDS>(smem, M, gscratch + base * Seg::kSize);
    stage_consts<kB>(L.kc);
    if (threadIdx.x == 0) *L.s_err = 0;
    double* Tt = L.extra;  // M
    for (int i = threadIdx.x; i < M; i += kB) {
        const double Ti = seg_times[seg0 + i];
        Tt[i] = variant == 0 ? Ti : mellinger_time(Ti, i, variant - 1, M, h, t_min);
    }
    __syncthreads();
    double* Cw = ws_c + base * 30;
    const int st = solve_track<kB, LDS>(L.kc, wp + (size_t)w0 * 3, M, 0.0, 0.0, v0 ? v0 + 3 * track : nullptr,
                                        a0 ? a0 + 3 * track : nullptr, Tt, L.scr, L.dv, L.rhs, L.Tm, L.xch, L.s_err,
                                        nullptr, Cw, true);
    double J = NAN;
    if (st == 0) {  // (workgroup-uniform)
        __syncthreads();
        J = wave_snap_cost(Tt, Cw, M);
    }
    if (threadIdx.x == 0) {
        Jv[(size_t)track * stride + variant] = J;
        stv[(size_t)track * stride + variant] = st;
    }
}

// The quotients of one track from its variants' costs
__global__ __launch_bounds__(kB) void k_time_quot(const int32_t* __restrict__ wp_off, int n_tracks, double h,
                                                  int stride, const double* __restrict__ Jv,
                                                  const int32_t* __restrict__ stv, double* __restrict__ cost,
                                                  double* __restrict__ grad, int32_t* __restrict__ status) {
    const int t = blockIdx.x;
    if (t >= n_tracks) return;
    const int seg0 = wp_off[t] - t;
    const int M = wp_off[t + 1] - wp_off[t] - 1;
    if (M < 1) {
        if (threadIdx.x == 0) {
            cost[t] = NAN;
            if (status) status[t] = -1;
        }
        return;
    }
    const size_t s0 = (size_t)t * stride;
    const int st0 = stv[s0];
    const double J0 = Jv[s0];
    int failed = 0;
    for (int n = threadIdx.x; n < M; n += kB) {
        double g = 0.0;  // M == 1: no gradient
        if (M > 1) {
            const int sn = stv[s0 + 1 + n];
            failed |= sn != 0;
            g = (st0 == 0 && sn == 0) ? (Jv[s0 + 1 + n] - J0) / h : NAN;
        } else if (st0 != 0) {
            g = NAN;
        }
        grad[seg0 + n] = g;
    }
    failed = __syncthreads_or(failed);
    if (threadIdx.x == 0) {
        cost[t] = st0 == 0 ? J0 : NAN;
        if (status) status[t] = st0 != 0 ? st0 : failed ? -3 : 0;
    }
}

// The descent of one track (include/epp.h, epp_minsnap_optimize_times).  LDS extras: the
// current times Tc, the trial times Tt, the gradient g and the direction d (M each).  All
// control flow around solve_track is workgroup-uniform: a solve's status is read behind its
// barrier, a cost is the same in every lane, and g / d / Tc are read from LDS by every lane.
template <bool LDS>
__global__ __launch_bounds__(kB) void k_time_opt(const double* __restrict__ wp, const int32_t* __restrict__ wp_off,
                                                 int n_tracks, const double* __restrict__ v0,
                                                 const double* __restrict__ a0, double* seg_times, double* coeffs,
                                                 epp_timeopt_params prm, double* ws_c, double* gscratch,
                                                 double* __restrict__ cost0, double* __restrict__ cost1,
                                                 int32_t* __restrict__ iters, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int track = blockIdx.x;
    if (track >= n_tracks) return;
    const int tid = threadIdx.x;
    const int w0 = wp_off[track];
    const int M = wp_off[track + 1] - w0 - 1;
    const int seg0 = w0 - track;
    auto finish = [&](double j0, double j1, int it, int st) {
        if (tid == 0) {
            cost0[track] = j0;
            cost1[track] = j1;
            iters[track] = it;
            if (status) status[track] = st;
        }
    };
    if (M < 1) {
        finish(NAN, NAN, 0, -1);
        return;
    }
    const SolveLds L = solve_lds<LDS>(smem, M, gscratch + (size_t)seg0 * Seg::kSize);
    stage_consts<kB>(L.kc);
    double* Tc = L.extra;
    double* Tt = Tc + M;
    double* g = Tt + M;
    double* d = g + M;
    double* Cw = ws_c + (size_t)seg0 * 30;      // a trial's coefficients
    double* Cout = coeffs + (size_t)seg0 * 30;  // the result's
    const double* P = wp + (size_t)w0 * 3;
    const double* v0p = v0 ? v0 + 3 * track : nullptr;
    const double* a0p = a0 ? a0 + 3 * track : nullptr;
    // J at `times` (LDS), the coefficients to Cdst; st: the solve's status (J NaN unless 0)
    auto eval = [&](const double* times, double* Cdst, double* Tout, int& st) -> double {
        __syncthreads();  // the writers of `times` and the previous solve's readers
        if (tid == 0) *L.s_err = 0;
        __syncthreads();
        st = solve_track<kB, LDS>(L.kc, P, M, 0.0, 0.0, v0p, a0p, times, L.scr, L.dv, L.rhs, L.Tm, L.xch, L.s_err, Tout,
                                  Cdst, true);
        if (st != 0) return NAN;
        __syncthreads();
        return wave_snap_cost(times, Cdst, M);
    };
    for (int i = tid; i < M; i += kB) Tc[i] = seg_times[seg0 + i];
    int st;
    double J = eval(Tc, Cout, nullptr, st);
    const double J0 = J;
    if (st != 0 || M == 1 || prm.max_iter <= 0 || !isfinite(J)) {  // the plain fit at the given times
        finish(J0, J0, 0, st);
        return;
    }
    double sum0 = 0.0;
    for (int i = 0; i < M; ++i) sum0 = sum0 + Tc[i];
    int done = 0, result = 2;
    for (int it = 0; it < prm.max_iter; ++it) {
        for (int n = 0; n < M; ++n) {
            __syncthreads();
            for (int i = tid; i < M; i += kB) Tt[i] = mellinger_time(Tc[i], i, n, M, prm.h, prm.t_min);
            int sn;
            const double Jn = eval(Tt, Cw, nullptr, sn);
            if (tid == 0) g[n] = (Jn - J) / prm.h;  // (NaN when the variant's solve broke down)
        }
        __syncthreads();
        for (int i = tid; i < M; i += kB) d[i] = descent_direction(g, i, M);
        __syncthreads();
        double dmax = 0.0, tmin = INFINITY;
        bool finite = true;
        for (int i = 0; i < M; ++i) {
            const double a = fabs(d[i]);
            finite = finite && isfinite(a);
            dmax = a > dmax ? a : dmax;
            tmin = Tc[i] < tmin ? Tc[i] : tmin;
        }
        if (!finite) {
            result = 1;
            break;
        }
        if (dmax == 0.0) {
            result = 0;
            break;
        }
        double alpha = prm.step0 * tmin / dmax;
        double Jt = NAN;
        bool accepted = false;
        for (int k = 0; k <= prm.max_halvings; ++k) {
            __syncthreads();
            int below = 0;
            for (int i = tid; i < M; i += kB) {
                const double t = Tc[i] - alpha * d[i];
                Tt[i] = t;
                below |= !(t >= prm.t_min);
            }
            if (!__syncthreads_or(below)) {
                int sk;
                Jt = eval(Tt, Cw, nullptr, sk);
                if (Jt < J) {
                    accepted = true;
                    break;
                }
            }
            alpha = 0.5 * alpha;
        }
        if (!accepted) {
            result = 1;
            break;
        }
        __syncthreads();
        for (int i = tid; i < M; i += kB) Tc[i] = Tt[i];
        __syncthreads();
        ++done;
        const double dec = J - Jt, Jold = J;
        J = Jt;
        if (dec <= prm.ftol * Jold) {
            result = 0;
            break;
        }
    }
    // one factor brings the running sum back to the start's; then the result's own fit
    __syncthreads();
    double sum = 0.0;
    for (int i = 0; i < M; ++i) sum = sum + Tc[i];
    const double f = sum0 / sum;
    __syncthreads();
    for (int i = tid; i < M; i += kB) Tc[i] = Tc[i] * f;
    const double J1 = eval(Tc, Cout, seg_times + seg0, st);
    finish(J0, J1, done, st != 0 ? st : result);
}

CachedWs g_timealloc_ws[64];

bool bad_positive(double x) { return !(x > 0.0) || !std::isfinite(x); }

// offsets into the workspace, 256-byte aligned parts
size_t after(size_t o, size_t bytes) { return (o + bytes + 255) & ~(size_t)255; }

struct WsUse {  // the device's workspace held for one call (released on every way out)
    CachedWs& ws;
    std::unique_lock<std::mutex> lk;
    hipStream_t s;
    bool held = false;
    WsUse(hipStream_t st) : ws(g_timealloc_ws[device() & 63]), lk(ws.mu), s(st) {}
    static int device() {
        int dev = 0;
        (void)hipGetDevice(&dev);
        return dev;
    }
    hipError_t acquire(size_t bytes) {
        const hipError_t e = ws.acquire(s, std::max<size_t>(bytes, 256));
        held = e == hipSuccess;
        return e;
    }
    ~WsUse() {
        if (held) ws.release(s);
    }
};

epp_status time_opt(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, const double* v0, const double* a0,
                    double* seg_times, double* coeffs, epp_timeopt_params p, double* cost0, double* cost1,
                    int32_t* iters, int32_t* status, hipStream_t s, const char* what, int known_m = -1) {
    if (n_tracks < 0 || (n_tracks > 0 && (!wp || !wp_offsets || !seg_times || !coeffs || !cost0 || !cost1 || !iters))) {
        set_error(std::string(what) + ": invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (bad_positive(p.h) || bad_positive(p.t_min) || bad_positive(p.step0) || p.step0 > 1.0 || !(p.ftol >= 0.0) ||
        !std::isfinite(p.ftol) || p.max_halvings < 0 || p.max_iter < 0) {
        set_error(std::string(what) +
                  ": the parameters must satisfy h > 0, t_min > 0, 0 < step0 <= 1, ftol >= 0, max_halvings >= 0, "
                  "max_iter >= 0");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    epp_status st = ensure_consts();
    if (st) return st;
    int max_m = 0;
    int64_t total_m = 0;
    if (known_m >= 0) {  // (one track whose segment count the host caller knows)
        max_m = std::max(1, known_m);
        total_m = known_m;
    } else if ((st = read_offsets(wp_offsets, n_tracks, s, what, &max_m, &total_m))) {
        return st;
    }
    const bool lds = max_m <= kMaxLdsSeg;
    const size_t shm = solve_lds_bytes(lds, max_m, 4 * max_m);
    if (shm > kLdsBudget) {
        set_error(std::string(what) + ": a track has too many waypoints for one workgroup's LDS (" +
                  std::to_string(max_m + 1) + ")");
        return EPP_ERR_UNSUPPORTED;
    }
    const size_t segs = (size_t)std::max<int64_t>(total_m, 1);
    const size_t o_C = 0, o_scr = after(o_C, segs * 240), bytes = lds ? o_scr : after(o_scr, segs * Seg::kSize * 8);
    WsUse use(s);
    const hipError_t e = use.acquire(bytes);
    if (e != hipSuccess) {
        set_error(std::string(what) + ": workspace: " + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    char* base = static_cast<char*>(use.ws.buf);
    double* d_C = reinterpret_cast<double*>(base + o_C);
    double* d_scr = lds ? nullptr : reinterpret_cast<double*>(base + o_scr);
    if (lds) {
        allow_lds(k_time_opt<true>);
        hipLaunchKernelGGL((k_time_opt<true>), dim3(n_tracks), dim3(kB), shm, s, wp, wp_offsets, n_tracks, v0, a0,
                           seg_times, coeffs, p, d_C, d_scr, cost0, cost1, iters, status);
    } else {
        allow_lds(k_time_opt<false>);
        hipLaunchKernelGGL((k_time_opt<false>), dim3(n_tracks), dim3(kB), shm, s, wp, wp_offsets, n_tracks, v0, a0,
                           seg_times, coeffs, p, d_C, d_scr, cost0, cost1, iters, status);
    }
    return launch_error(what);
}

}  // namespace

epp_status launch_time_opt_track(const double* wp, const int32_t* wp_off, int M, const double* v0, const double* a0,
                                 double* seg_times, double* coeffs, const epp_timeopt_params& p, double* cost0,
                                 double* cost1, int32_t* iters, int32_t* status, hipStream_t st, const char* what) {
    return time_opt(wp, wp_off, 1, v0, a0, seg_times, coeffs, p, cost0, cost1, iters, status, st, what, M);
}

}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_traj_snap_cost(const double* seg_times, const double* coeffs, const int32_t* wp_offsets,
                              int32_t n_tracks, double* cost, int32_t* status, void* stream) {
    if (n_tracks < 0 || (n_tracks > 0 && (!seg_times || !coeffs || !wp_offsets || !cost))) {
        set_error("epp_traj_snap_cost: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    hipLaunchKernelGGL(k_traj_snap_cost, dim3(n_tracks), dim3(kB), 0, (hipStream_t)stream, seg_times, coeffs,
                       wp_offsets, n_tracks, cost, status);
    return launch_error("epp_traj_snap_cost");
}

epp_status epp_minsnap_time_gradient(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, const double* v0,
                                     const double* a0, const double* seg_times, double h, double t_min, double* cost,
                                     double* grad, int32_t* status, void* stream) {
    const char* what = "epp_minsnap_time_gradient";
    if (n_tracks < 0 || (n_tracks > 0 && (!wp || !wp_offsets || !seg_times || !cost || !grad))) {
        set_error(std::string(what) + ": invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (bad_positive(h) || bad_positive(t_min)) {
        set_error(std::string(what) + ": h and t_min must be greater than zero");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (n_tracks == 0) return EPP_OK;
    epp_status st = ensure_consts();
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    int max_m = 0;
    int64_t total_m = 0;
    if ((st = read_offsets(wp_offsets, n_tracks, s, what, &max_m, &total_m))) return st;
    if (max_m + 1 > 65535) {
        set_error(std::string(what) + ": a track has too many waypoints (" + std::to_string(max_m + 1) + ")");
        return EPP_ERR_UNSUPPORTED;
    }
    const bool lds = max_m <= kMaxLdsSeg;
    const size_t shm = solve_lds_bytes(lds, max_m, max_m);
    if (shm > kLdsBudget) {
        set_error(std::string(what) + ": a track has too many waypoints for one workgroup's LDS (" +
                  std::to_string(max_m + 1) + ")");
        return EPP_ERR_UNSUPPORTED;
    }
    const int stride = max_m + 1;
    const size_t slots = (size_t)n_tracks * stride, vsegs = (size_t)std::max<int64_t>(total_m, 1) * stride;
    const size_t o_J = 0, o_st = after(o_J, slots * 8), o_C = after(o_st, slots * 4), o_scr = after(o_C, vsegs * 240),
                 bytes = lds ? o_scr : after(o_scr, vsegs * Seg::kSize * 8);
    WsUse use(s);
    const hipError_t e = use.acquire(bytes);
    if (e != hipSuccess) {
        set_error(std::string(what) + ": workspace: " + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    char* base = static_cast<char*>(use.ws.buf);
    double* d_J = reinterpret_cast<double*>(base + o_J);
    int32_t* d_st = reinterpret_cast<int32_t*>(base + o_st);
    double* d_C = reinterpret_cast<double*>(base + o_C);
    double* d_scr = lds ? nullptr : reinterpret_cast<double*>(base + o_scr);
    const dim3 grid(n_tracks, stride);
    if (lds) {
        allow_lds(k_time_grad<true>);
        hipLaunchKernelGGL((k_time_grad<true>), grid, dim3(kB), shm, s, wp, wp_offsets, n_tracks, v0, a0, seg_times, h,
                           t_min, stride, d_C, d_scr, d_J, d_st);
    } else {
        allow_lds(k_time_grad<false>);
        hipLaunchKernelGGL((k_time_grad<false>), grid, dim3(kB), shm, s, wp, wp_offsets, n_tracks, v0, a0, seg_times,
                           h, t_min, stride, d_C, d_scr, d_J, d_st);
    }
    if ((st = launch_error(what))) return st;
    hipLaunchKernelGGL(k_time_quot, dim3(n_tracks), dim3(kB), 0, s, wp_offsets, n_tracks, h, stride, d_J, d_st, cost,
                       grad, status);
    return launch_error(what);
}

epp_status epp_minsnap_optimize_times(const double* wp, const int32_t* wp_offsets, int32_t n_tracks, const double* v0,
                                      const double* a0, double* seg_times, double* coeffs, epp_timeopt_params p,
                                      double* cost0, double* cost1, int32_t* iters, int32_t* status, void* stream) {
    return time_opt(wp, wp_offsets, n_tracks, v0, a0, seg_times, coeffs, p, cost0, cost1, iters, status,
                    (hipStream_t)stream, "epp_minsnap_optimize_times");
}

}  // extern "C"
