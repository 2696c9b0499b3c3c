// minsnap_kernels.h — minimum-snap fitting and sampling of tracks for gfx950 (MI355X).
//
//   poly_traj::generateTrajectory   external/poly_traj/src/trajectory_generator.cpp:12-100
//   Trajectory::evaluateRange       src/trajectory.cpp:81-141
//
// Files:
//   minsnap_solve.h     the solve of one track by one workgroup (solve_track) and its constants
//   minsnap.hip         the batch stage: k_minsnap, k_sample_count, k_sample_rows behind
//                       epp_minsnap_batch[_times], epp_sample_count, epp_sample_batch
//   minsnap_constrained.hip  the batch fit with the caller's constraints: k_minsnap_constrained
//                       behind epp_minsnap_batch_constrained
//   minsnap_refit.hip   the 50 Hz latency path: one track fitted and sampled in one launch
//                       (k_refit, k_check_refit) behind generate_trajectory_into /
//                       check_and_generate_into (epp_internal.h)
//   time_alloc.hip      snap cost, Mellinger gradient and descent over the segment times
//                       (time_alloc.h: the arithmetic they share with the host)
//   host_generate.cpp   the C entry points of the single-track host calls, and the fits
//                       scaled to limits (fit, scale kernels, sampler on one stream)
//
// The kernels sit in anonymous namespaces, so minsnap.hip offers the two single-track
// launchers host_generate.cpp needs.  A launcher enqueues on st and returns the launch
// status (launch_error(what)).
#pragma once
#include <hip/hip_runtime_api.h>

#include "epp.h"
#include "epp_internal.h"

namespace epp {

// (minsnap.hip) k_minsnap over one track of M segments (wp_off = {0, M + 1}; the host caller
// knows M, so the offsets are not read back), Nfabian times; as epp_minsnap_batch otherwise
epp_status launch_minsnap_track(const double* wp, const int32_t* wp_off, int M, double v_max, double a_max,
                                const double* v0, const double* a0, double* seg_times, double* coeffs,
                                int32_t* status, hipStream_t st, const char* what);

// (minsnap_constrained.hip) k_minsnap_constrained over one track of M segments: as
// epp_minsnap_batch_constrained (times_in NULL: Nfabian times; fixed_mask M + 1 bytes, fixed_val
// (M + 1) x 12)
epp_status launch_minsnap_constrained_track(const double* wp, const int32_t* wp_off, int M, double v_max, double a_max,
                                            const double* times_in, const uint8_t* fixed_mask,
                                            const double* fixed_val, double* seg_times, double* coeffs,
                                            int32_t* status, hipStream_t st, const char* what);

// (minsnap.hip) the per-device workspace that holds the segment scratch of long tracks for
// both batch fits (k_minsnap, k_minsnap_constrained)
struct CachedWs;
CachedWs& minsnap_workspace(int dev);

// (minsnap.hip) k_sample_rows over the same track: at most cap_rows rows (the host's count of
// the recurrence) to rows, the time column offset by *t0
epp_status launch_sample_rows_track(const double* seg_times, const double* coeffs, const int32_t* wp_off, int M,
                                    double dt, const double* t0, double* rows, int64_t cap_rows, hipStream_t st,
                                    const char* what);

// (minsnap.hip) the track offsets of a batch read back from the device on s: the largest
// segment count (at least 1) and, total_m != NULL, the total
epp_status read_offsets(const int32_t* d_off, int n_tracks, hipStream_t s, const char* what, int* max_m,
                        int64_t* total_m);

// (time_alloc.hip) k_time_opt over one track of M segments in place on seg_times / coeffs (the
// host caller knows M); as epp_minsnap_optimize_times otherwise, its argument checks included
epp_status launch_time_opt_track(const double* wp, const int32_t* wp_off, int M, const double* v0, const double* a0,
                                 double* seg_times, double* coeffs, const epp_timeopt_params& p, double* cost0,
                                 double* cost1, int32_t* iters, int32_t* status, hipStream_t st, const char* what);

// The error text of a single-track call from its kernels' statuses: the fit's (-2: a segment
// time <= 0, the reference's CHECK_GT(segment_time, 0), impl :297; else the solve), then the
// v / a scaling's and the thrust scaling's (0 where the call runs neither).
inline const char* fit_status_message(int fit, int scale = 0, int thrust = 0) {
    return fit == -2                   ? "Segment times need to be greater than zero"
           : fit != 0                  ? "min-snap solve failed"
           : scale == 1                ? "generateTrajectory: v_max / a_max not met after 20 rounds of time scaling"
           : scale == 0 && thrust == 1 ? "generateTrajectory: the thrust limits are not met at 1024 times the duration"
                                       : "generateTrajectory: the fit is not finite";
}

}  // namespace epp
