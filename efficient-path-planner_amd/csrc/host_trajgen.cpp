// host_trajgen.cpp — poly_traj::generateTrajectory and its limited and constrained variants
// over the HIP min-snap path (the C entry points of host_generate.cpp).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "epp.h"
#include "epp_internal.h"
#include "epp/trajectory_generator.h"
#include "host_waypoints.h"

namespace poly_traj {

namespace {
std::vector<double> checked_flat(const std::vector<epp::Vec3>& waypoints) {
    if (waypoints.size() < 2) throw std::invalid_argument("At least two waypoints are required");
    std::vector<double> wp;
    epp::flatten(waypoints, wp);
    return wp;
}
void throw_unless_ok(epp_status rc) {
    if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
    if (rc != EPP_OK) throw std::runtime_error(std::string("generateTrajectory: ") + epp_last_error());
}
// The n rows a *_host call handed out (none when it failed) into result, freed.
void take_rows(epp_status rc, double* rows, int64_t n, epp::Matrix& result) {
    throw_unless_ok(rc);
    result.rows = (size_t)n;
    result.cols = 10;
    result.data.assign(rows, rows + (size_t)n * 10);
    epp_host_free(rows);
}
}  // namespace

bool generateTrajectory(const std::vector<epp::Vec3>& waypoints, double v_max, double a_max,
                        double sampling_intervall, double startTimeOffset, const epp::Vec3& v0,
                        const epp::Vec3& a0, epp::Matrix& result) {
    const std::vector<double> wp = checked_flat(waypoints);
    const double v[3] = {v0.x, v0.y, v0.z}, a[3] = {a0.x, a0.y, a0.z};
    // the rows go straight from the kernel's pinned output into `result` (its storage is
    // reused when the caller passes the previous trajectory back, as a 50 Hz loop does)
    epp::Matrix tmp;
    std::swap(tmp, result);  // (result keeps its old value if the call throws)
    int64_t n = 0;
    const epp_status rc =
        epp::generate_trajectory_into(wp.data(), (int32_t)waypoints.size(), nullptr, v_max, a_max, sampling_intervall,
                                      startTimeOffset, v, a, epp::matrix_rows, &tmp, &n);
    if (rc != EPP_OK) {
        std::swap(tmp, result);
        throw_unless_ok(rc);
    }
    tmp.data.resize((size_t)n * 10);
    std::swap(tmp, result);
    return true;
}

bool generateTrajectoryWithinLimits(const std::vector<epp::Vec3>& waypoints, double v_max, double a_max,
                                    double sampling_intervall, double startTimeOffset, const epp::Vec3& v0,
                                    const epp::Vec3& a0, epp::Matrix& result, double* scale) {
    const std::vector<double> wp = checked_flat(waypoints);
    const double v[3] = {v0.x, v0.y, v0.z}, a[3] = {a0.x, a0.y, a0.z};
    double* rows = nullptr;
    int64_t n = 0;
    const epp_status rc =
        epp_generate_trajectory_limited_host(wp.data(), (int32_t)waypoints.size(), v_max, a_max, sampling_intervall,
                                             startTimeOffset, v, a, &rows, &n, scale);
    take_rows(rc, rows, n, result);
    return true;
}

bool generateTrajectoryConstrained(const std::vector<epp::Vec3>& waypoints, double v_max, double a_max,
                                   double sampling_intervall, double startTimeOffset, const epp::WaypointPins& pins,
                                   epp::Matrix& result) {
    const std::vector<double> wp = checked_flat(waypoints);
    if (pins.mask.size() != waypoints.size() || pins.values.size() != waypoints.size() * 12)
        throw std::invalid_argument("generateTrajectoryConstrained: pins need one mask byte and 12 values per waypoint");
    double* rows = nullptr;
    int64_t n = 0;
    const epp_status rc = epp_generate_trajectory_constrained_host(
        wp.data(), (int32_t)waypoints.size(), v_max, a_max, nullptr, sampling_intervall, startTimeOffset,
        pins.mask.data(), pins.values.data(), &rows, &n);
    take_rows(rc, rows, n, result);
    return true;
}

}  // namespace poly_traj
