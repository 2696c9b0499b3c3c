// epp/trajectory_generator.h — drop-in for poly_traj::generateTrajectory
// (external/poly_traj/include/poly_traj/trajectory_generator.h:20,
// external/poly_traj/src/trajectory_generator.cpp:12-100), computed by the batched
// min-snap kernels (include/epp.h epp_minsnap_batch / epp_sample_batch).
#pragma once
#include <vector>

#include "epp/types.h"

namespace poly_traj {

// result: rows x 10 [x, vx, ax, y, vy, ay, z, vz, az, t + startTimeOffset].
// Throws std::invalid_argument("At least two waypoints are required") for < 2 waypoints
// and std::runtime_error for a non-positive segment time (the reference CHECK-aborts).
bool generateTrajectory(const std::vector<epp::Vec3>& waypoints, double v_max, double a_max,
                        double sampling_intervall, double startTimeOffset, const epp::Vec3& initialVel,
                        const epp::Vec3& initialAcc, epp::Matrix& result);

// generateTrajectory with v_max and a_max enforced on the fitted trajectory (the reference
// library's Trajectory::scaleSegmentTimesToMeetConstraints,
// external/poly_traj/src/trajectory.cpp:385-429, which its generateTrajectory never calls):
// every segment time is stretched by one factor s >= 1 until the peak speed and acceleration
// are within the limits (to 1e-3 relative), so the path keeps its shape and the rows cover
// the longer duration (include/epp.h epp_generate_trajectory_limited_host).  *scale (may be
// null): s.  Time scaling divides the start velocity by s and the start acceleration by
// s^2: only initialVel = initialAcc = 0 survive it unchanged.  Throws as generateTrajectory,
// and std::invalid_argument for v_max <= 0 or a_max <= 0.
bool generateTrajectoryWithinLimits(const std::vector<epp::Vec3>& waypoints, double v_max, double a_max,
                                    double sampling_intervall, double startTimeOffset, const epp::Vec3& initialVel,
                                    const epp::Vec3& initialAcc, epp::Matrix& result, double* scale = nullptr);

}  // namespace poly_traj
