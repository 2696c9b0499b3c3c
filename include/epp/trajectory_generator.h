// epp/trajectory_generator.h — drop-in for poly_traj::generateTrajectory
// (external/poly_traj/include/poly_traj/trajectory_generator.h:20,
// external/poly_traj/src/trajectory_generator.cpp:12-100), computed by the batched
// min-snap kernels (include/epp.h epp_minsnap_batch / epp_sample_batch).
#pragma once
#include <cstdint>
#include <vector>

#include "epp/types.h"

namespace epp {

// The constraints of generateTrajectoryConstrained: mask has one byte per waypoint, values
// 12 doubles per waypoint.  pin() sizes both for n waypoints on first use.
struct WaypointPins {
    std::vector<uint8_t> mask;
    std::vector<double> values;
    // fixes derivative k (1..4) at waypoint w of n to val
    void pin(size_t n, size_t w, int k, const Vec3& val) {
        mask.resize(n, 0);
        values.resize(n * 12, 0.0);
        mask[w] |= (uint8_t)(1u << (k - 1));
        double* p = &values[(w * 4 + (size_t)(k - 1)) * 3];
        p[0] = val.x;
        p[1] = val.y;
        p[2] = val.z;
    }
};

}  // namespace epp

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

// generateTrajectory under the caller's constraints (what the reference's library takes
// through Vertex::addConstraint, external/poly_traj/src/vertex.cpp:30-60, and its
// generateTrajectory never uses; include/epp.h epp_generate_trajectory_constrained_host).
// pins: per waypoint one mask byte (bit k-1: derivative k = 1..4 is fixed there) and 12 values
// ((k-1) * 3 + d).  At the first and the last waypoint all four derivatives are fixed: the
// mask there is ignored and the values are the start state (v, a, jerk, snap) and the end
// state; generateTrajectory is values {initialVel, initialAcc, 0, 0} at the start, zeros at
// the end and mask 0 inside.  Values whose bit is clear at an inner waypoint are not read.
// Segment times are Nfabian's (they ignore the pins).  Throws as generateTrajectory, and
// std::invalid_argument for pins of the wrong size, a mask bit above bit 3 or a non-finite
// value that is used.
bool generateTrajectoryConstrained(const std::vector<epp::Vec3>& waypoints, double v_max, double a_max,
                                   double sampling_intervall, double startTimeOffset, const epp::WaypointPins& pins,
                                   epp::Matrix& result);

}  // namespace poly_traj
