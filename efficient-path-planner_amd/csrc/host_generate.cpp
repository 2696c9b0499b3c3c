// host_generate.cpp — the C entry points of the single-track host calls: generateTrajectory
// (and its variants with caller times and with the fused check) over the refit
// (minsnap_refit.hip), the fits scaled to limits before the sampling (generate_scaled) and the
// fit under the caller's constraints (generate_constrained), which end in one row-sampling
// tail (sample_fitted_rows).
// Host code only: the kernels are enqueued through minsnap_kernels.h and the C ABI.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "epp.h"
#include "epp_internal.h"
#include "minsnap_kernels.h"
#include "stream_bufs.h"
#include "traj_sample.h"

namespace epp {
namespace {

double* malloc_rows(void* ctx, int64_t R) {
    double* p = (double*)std::malloc((size_t)std::max<int64_t>(R, 1) * 80);
    *static_cast<double**>(ctx) = p;
    return p;
}
// a failed call hands out no rows: frees what malloc_rows allocated
epp_status free_rows_on_failure(epp_status rc, double** rows_out) {
    if (rc != EPP_OK && *rows_out) {
        std::free(*rows_out);
        *rows_out = nullptr;
    }
    return rc;
}
epp_status generate_trajectory(const double* wp, int32_t n_wp, const double* times, double v_max, double a_max,
                               double dt, double t0, const double v0[3], const double a0[3], double** rows_out,
                               int64_t* n_rows) {
    if (!rows_out || !n_rows) {
        set_error("generateTrajectory: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    *rows_out = nullptr;
    return free_rows_on_failure(
        generate_trajectory_into(wp, n_wp, times, v_max, a_max, dt, t0, v0, a0, malloc_rows, rows_out, n_rows),
        rows_out);
}

// The end of generate_scaled and generate_constrained, once the fit's statuses have passed:
// the host runs Trajectory::evaluateRange's sample recurrence on the fitted (scaled) times in
// the pinned block (the exact row count), then the row sampler on c's stream into h_out, one
// synchronisation, and the rows copied into a malloc'ed buffer the caller owns.
epp_status sample_fitted_rows(StreamBufs& c, const double* h_T, const double* h_C, const int32_t* h_off, int M,
                              double dt, const double* h_t0, double** rows_out, int64_t* n_rows) {
    int64_t R = 0;
    if (dt > 0) {
        RangeIter it;
        it.init(h_T, M);
        R = range_count(it, dt);
    }
    if (!malloc_rows(rows_out, R)) {
        set_error("generateTrajectory: out of host memory");
        return EPP_ERR_RUNTIME;
    }
    if (R) {
        epp_status rc = EPP_OK;
        hipError_t e;
        if ((e = c.ensure(0, (size_t)R * 80, 0)) != hipSuccess) rc = buffers_error(e);
        if (!rc)
            rc = launch_sample_rows_track(h_T, h_C, h_off, M, dt, h_t0, c.h_out.as<double>(), R, c.s,
                                          "generateTrajectory");
        if (!rc && (e = hipStreamSynchronize(c.s)) != hipSuccess) {
            set_error(std::string("generateTrajectory: ") + hipGetErrorString(e));
            rc = EPP_ERR_HIP;
        }
        if (rc) return free_rows_on_failure(rc, rows_out);
        std::memcpy(*rows_out, c.h_out.p, (size_t)R * 80);
    }
    *n_rows = R;
    return EPP_OK;
}

// generateTrajectory followed by Trajectory::scaleSegmentTimesToMeetConstraints
// (src/trajectory.cpp:385-429) before the sampling: three launches on the calling thread's
// stream over pinned host buffers (StreamBufs: h_in the track's inputs, times, coefficients
// and flags, h_out the rows; the kernels read and write them directly) -- the batch fit
// (k_minsnap, one track), k_traj_scale, then, after the host has run evaluateRange's sample
// recurrence on the SCALED times to size the row buffer, the row sampler.
// (enforce_va: k_traj_scale; tl != NULL: k_traj_thrust_scale under tl = [g, f_min, f_max,
// rate_max, cos_tilt_min] after it -- epp_generate_trajectory_flyable_host; the limited call
// is enforce_va with tl == NULL)
// (opt != NULL: k_time_opt under *opt between the fit and the scalings --
// epp_generate_trajectory_timeopt_host: uniform scaling keeps the optimised ratios of the
// segment times, so the order is optimise, then scale; opt_out: [cost0, cost1, iters])
struct TimeoptOut {
    double cost0 = 0.0, cost1 = 0.0;
    int32_t iters = 0;
};
epp_status generate_scaled(const double* wp, int32_t n_wp, double v_max, double a_max, double dt, double t0,
                           const double v0[3], const double a0[3], bool enforce_va, const double* tl,
                           double** rows_out, int64_t* n_rows, double* scale_out, double* scale_thrust,
                           const epp_timeopt_params* opt = nullptr, TimeoptOut* opt_out = nullptr) {
    if (!rows_out || !n_rows || (n_wp > 0 && !wp)) {
        set_error("generateTrajectory: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    *rows_out = nullptr;
    *n_rows = 0;
    if (n_wp < 2) {
        set_error("At least two waypoints are required");  // trajectory_generator.cpp:24
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (enforce_va && (!(v_max > 0.0) || !(a_max > 0.0))) {
        set_error("generateTrajectory: v_max and a_max must be greater than zero to enforce them");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (tl) {  // the limits' conditions, before any device work (an empty batch launches nothing)
        const epp_status bad = epp_traj_scale_to_thrust_limits(nullptr, nullptr, nullptr, 0, tl[0], tl[1], tl[2], tl[3],
                                                               tl[4], nullptr, nullptr, nullptr, nullptr);
        if (bad) return bad;
    }
    if (opt) {  // likewise the descent's parameters
        const epp_status bad = epp_minsnap_optimize_times(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, *opt,
                                                          nullptr, nullptr, nullptr, nullptr, nullptr);
        if (bad) return bad;
    }
    const int M = n_wp - 1;
    for (int i = 0; i < M; ++i)
        if (!(nfabian(wp + 3 * i, wp + 3 * (i + 1), v_max, a_max) > 0)) {  // CHECK_GT(segment_time, 0)  impl :297
            set_error(fit_status_message(-2));
            return EPP_ERR_RUNTIME;
        }
    static thread_local StreamBufs c;
    if (c.bind() != hipSuccess) {
        set_error("generateTrajectory: stream");
        return EPP_ERR_HIP;
    }
    epp_status rc;
    const size_t nd = (size_t)3 * n_wp + 6 + (size_t)M * 31 + 5;  // doubles before the int32 words
    hipError_t e = c.ensure(nd * 8 + 32, 0, 0);
    if (e != hipSuccess) return buffers_error(e);
    double* h_wp = c.h_in.as<double>();
    double* h_v0 = h_wp + 3 * n_wp;
    double* h_a0 = h_v0 + 3;
    double* h_T = h_a0 + 3;
    double* h_C = h_T + M;
    double* h_scale = h_C + (size_t)M * 30;
    double* h_t0 = h_scale + 2;  // (h_scale: [v / a, thrust])
    double* h_cost = h_t0 + 1;   // [cost0, cost1] of the descent
    int32_t* h_off = reinterpret_cast<int32_t*>(h_cost + 2);
    int32_t* h_st = h_off + 2;  // [fit, scale, thrust scale, descent, its iterations]
    std::memcpy(h_wp, wp, (size_t)n_wp * 24);
    for (int k = 0; k < 3; ++k) {
        h_v0[k] = v0 ? v0[k] : 0.0;
        h_a0[k] = a0 ? a0[k] : 0.0;
    }
    h_scale[0] = h_scale[1] = 1.0;
    *h_t0 = t0;
    h_off[0] = 0;
    h_off[1] = n_wp;
    h_st[0] = -100;
    h_st[1] = enforce_va ? -100 : 0;
    h_st[2] = tl ? -100 : 0;
    h_st[3] = opt ? -100 : 0;
    h_st[4] = 0;
    h_cost[0] = h_cost[1] = 0.0;
    if ((rc = launch_minsnap_track(h_wp, h_off, M, v_max, a_max, h_v0, h_a0, h_T, h_C, h_st, c.s, "generateTrajectory")))
        return rc;
    if (opt && (rc = launch_time_opt_track(h_wp, h_off, M, h_v0, h_a0, h_T, h_C, *opt, h_cost, h_cost + 1, h_st + 4,
                                           h_st + 3, c.s, "generateTrajectory")))
        return rc;
    if (enforce_va && (rc = epp_traj_scale_to_limits(h_T, h_C, h_off, 1, v_max, a_max, h_scale, h_st + 1, c.s)))
        return rc;
    if (tl && (rc = epp_traj_scale_to_thrust_limits(h_T, h_C, h_off, 1, tl[0], tl[1], tl[2], tl[3], tl[4], h_scale + 1,
                                                    h_st + 2, nullptr, c.s)))
        return rc;
    e = hipStreamSynchronize(c.s);
    if (e != hipSuccess) {
        set_error(std::string("generateTrajectory: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    // (the descent's 1 -- no step accepted -- and 2 -- max_iter steps taken -- are answers)
    if (h_st[0] != 0 || h_st[3] < 0 || h_st[1] != 0 || h_st[2] != 0) {
        set_error(fit_status_message(h_st[0] != 0 ? h_st[0] : h_st[3] < 0 ? h_st[3] : 0, h_st[1], h_st[2]));
        return EPP_ERR_RUNTIME;
    }
    if (opt_out) *opt_out = TimeoptOut{h_cost[0], h_cost[1], h_st[4]};
    if ((rc = sample_fitted_rows(c, h_T, h_C, h_off, M, dt, h_t0, rows_out, n_rows))) return rc;
    if (scale_out) *scale_out = h_scale[0];
    if (scale_thrust) *scale_thrust = h_scale[1];
    return EPP_OK;
}

// generateTrajectory under the caller's constraints: the constrained batch fit
// (k_minsnap_constrained, one track) and, after the host has run evaluateRange's sample
// recurrence on the fit's times to size the row buffer, the row sampler -- two launches on
// the calling thread's stream over pinned host buffers, as generate_scaled.  times: the
// caller's segment times (NULL: Nfabian).
epp_status generate_constrained(const double* wp, int32_t n_wp, double v_max, double a_max, const double* times,
                                double dt, double t0, const uint8_t* fixed_mask, const double* fixed_val,
                                double** rows_out, int64_t* n_rows) {
    if (!rows_out || !n_rows || (n_wp > 0 && (!wp || !fixed_mask || !fixed_val))) {
        set_error("generateTrajectory: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    *rows_out = nullptr;
    *n_rows = 0;
    if (n_wp < 2) {
        set_error("At least two waypoints are required");  // trajectory_generator.cpp:24
        return EPP_ERR_INVALID_ARGUMENT;
    }
    const int M = n_wp - 1;
    static thread_local StreamBufs c;
    if (c.bind() != hipSuccess) {
        set_error("generateTrajectory: stream");
        return EPP_ERR_HIP;
    }
    epp_status rc;
    // doubles [wp (3 W) | values (12 W) | T in (M) | T (M) | coeffs (30 M) | t0], then the int32
    // words [offsets (2) | fit status], then the mask bytes
    const size_t nd = (size_t)15 * n_wp + (size_t)M * 32 + 1;
    hipError_t e = c.ensure(nd * 8 + 16 + (size_t)n_wp, 0, 0);
    if (e != hipSuccess) return buffers_error(e);
    double* h_wp = c.h_in.as<double>();
    double* h_val = h_wp + 3 * n_wp;
    double* h_Tin = h_val + (size_t)12 * n_wp;
    double* h_T = h_Tin + M;
    double* h_C = h_T + M;
    double* h_t0 = h_C + (size_t)M * 30;
    int32_t* h_off = reinterpret_cast<int32_t*>(h_t0 + 1);
    int32_t* h_st = h_off + 2;
    uint8_t* h_mask = reinterpret_cast<uint8_t*>(h_off + 4);
    std::memcpy(h_wp, wp, (size_t)n_wp * 24);
    std::memcpy(h_val, fixed_val, (size_t)n_wp * 96);
    std::memcpy(h_mask, fixed_mask, (size_t)n_wp);
    if (times) std::memcpy(h_Tin, times, (size_t)M * 8);
    *h_t0 = t0;
    h_off[0] = 0;
    h_off[1] = n_wp;
    h_st[0] = -100;
    if ((rc = launch_minsnap_constrained_track(h_wp, h_off, M, v_max, a_max, times ? h_Tin : nullptr, h_mask, h_val,
                                               h_T, h_C, h_st, c.s, "generateTrajectory")))
        return rc;
    e = hipStreamSynchronize(c.s);
    if (e != hipSuccess) {
        set_error(std::string("generateTrajectory: ") + hipGetErrorString(e));
        return EPP_ERR_HIP;
    }
    if (h_st[0] == -4) {
        set_error("generateTrajectory: a constraint mask has a bit above bit 3, or a fixed value is not finite");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    if (h_st[0] != 0) {
        set_error(fit_status_message(h_st[0]));
        return EPP_ERR_RUNTIME;
    }
    return sample_fitted_rows(c, h_T, h_C, h_off, M, dt, h_t0, rows_out, n_rows);
}

}  // namespace
}  // namespace epp

using namespace epp;

extern "C" {

epp_status epp_generate_trajectory_host(const double* wp, int32_t n_wp, double v_max, double a_max, double dt,
                                        double t0, const double v0[3], const double a0[3], double** rows_out,
                                        int64_t* n_rows) {
    return generate_trajectory(wp, n_wp, nullptr, v_max, a_max, dt, t0, v0, a0, rows_out, n_rows);
}

epp_status epp_check_and_generate_trajectory_host(const epp_world* world, const double* check_xyz, int64_t n_check,
                                                  double min_distance, uint8_t* check_valid, const double* wp,
                                                  int32_t n_wp, double v_max, double a_max, double dt, double t0,
                                                  const double v0[3], const double a0[3], double** rows_out,
                                                  int64_t* n_rows) {
    if (!rows_out || !n_rows || !world || n_check < 0 || (n_check > 0 && (!check_xyz || !check_valid))) {
        set_error("epp_check_and_generate_trajectory_host: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    *rows_out = nullptr;
    const FusedCheck chk{world, check_xyz, n_check, min_distance, check_valid};
    return free_rows_on_failure(
        check_and_generate_into(&chk, wp, n_wp, nullptr, v_max, a_max, dt, t0, v0, a0, malloc_rows, rows_out, n_rows),
        rows_out);
}

epp_status epp_generate_trajectory_times_host(const double* wp, int32_t n_wp, const double* seg_times, double dt,
                                              double t0, const double v0[3], const double a0[3], double** rows_out,
                                              int64_t* n_rows) {
    if (n_wp >= 2 && !seg_times) {
        set_error("generateTrajectory: invalid argument");
        return EPP_ERR_INVALID_ARGUMENT;
    }
    return generate_trajectory(wp, n_wp, seg_times, 0.0, 0.0, dt, t0, v0, a0, rows_out, n_rows);
}

epp_status epp_generate_trajectory_constrained_host(const double* wp, int32_t n_wp, double v_max, double a_max,
                                                    const double* seg_times, double dt, double t0,
                                                    const uint8_t* fixed_mask, const double* fixed_val,
                                                    double** rows_out, int64_t* n_rows) {
    return generate_constrained(wp, n_wp, v_max, a_max, seg_times, dt, t0, fixed_mask, fixed_val, rows_out, n_rows);
}

epp_status epp_generate_trajectory_limited_host(const double* wp, int32_t n_wp, double v_max, double a_max, double dt,
                                                double t0, const double v0[3], const double a0[3], double** rows_out,
                                                int64_t* n_rows, double* scale_out) {
    return generate_scaled(wp, n_wp, v_max, a_max, dt, t0, v0, a0, true, nullptr, rows_out, n_rows, scale_out,
                           nullptr);
}

// The same with epp_traj_scale_to_thrust_limits (thrust_scale.hip) after the v / a scaling,
// which enforce_va switches: one launch more on the same stream, before the one synchronisation.
epp_status epp_generate_trajectory_flyable_host(const double* wp, int32_t n_wp, double v_max, double a_max, double dt,
                                                double t0, const double v0[3], const double a0[3], int32_t enforce_va,
                                                double g, double f_min, double f_max, double rate_max,
                                                double cos_tilt_min, double** rows_out, int64_t* n_rows,
                                                double* scale_va, double* scale_thrust) {
    const double tl[5] = {g, f_min, f_max, rate_max, cos_tilt_min};
    return generate_scaled(wp, n_wp, v_max, a_max, dt, t0, v0, a0, enforce_va != 0, tl, rows_out, n_rows, scale_va,
                           scale_thrust);
}

// The fit, the descent over its segment times (time_alloc.hip), the scalings asked for, the
// sampler: one stream, one synchronisation before the row count.
epp_status epp_generate_trajectory_timeopt_host(const double* wp, int32_t n_wp, double v_max, double a_max, double dt,
                                                double t0, const double v0[3], const double a0[3],
                                                epp_timeopt_params params, int32_t enforce_va,
                                                const double* thrust_limits, double** rows_out, int64_t* n_rows,
                                                double* cost0, double* cost1, int32_t* iters) {
    TimeoptOut out;
    const epp_status rc = generate_scaled(wp, n_wp, v_max, a_max, dt, t0, v0, a0, enforce_va != 0, thrust_limits,
                                          rows_out, n_rows, nullptr, nullptr, &params, &out);
    if (rc == EPP_OK) {
        if (cost0) *cost0 = out.cost0;
        if (cost1) *cost1 = out.cost1;
        if (iters) *iters = out.iters;
    }
    return rc;
}

}  // extern "C"
