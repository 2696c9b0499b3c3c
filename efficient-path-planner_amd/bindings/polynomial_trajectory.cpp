// polynomial_trajectory — the documented Python surface of the reference's min-snap
// wrapper (external/poly_traj/README.md:79, `polynomial_trajectory.generate_trajectory`;
// the reference ships no binding source for it).  Backed by the HIP kernels through
// the C ABI; returns the real 10-column layout of poly_traj::generateTrajectory
// ([x, vx, ax, y, vy, ay, z, vz, az, t], src/trajectory_generator.cpp:81-96).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "epp.h"

namespace py = pybind11;

static void read3(py::object o, double* out) {
    if (o.is_none()) return;
    auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(o);
    if (!a || a.size() != 3) throw std::invalid_argument("initial velocity/acceleration must have 3 entries");
    for (int i = 0; i < 3; ++i) out[i] = a.data()[i];
}

// waypointVel / waypointAcc: a list as long as the waypoints, None = free there; derivative k of
// the inner waypoints it names goes into mask / values (epp_minsnap_batch_constrained's layout)
static void read_waypoint_pins(py::object o, int k, py::ssize_t n, std::vector<uint8_t>& mask,
                               std::vector<double>& values, const char* name) {
    if (o.is_none()) return;
    if (!py::isinstance<py::sequence>(o) || (py::ssize_t)py::len(o) != n)
        throw py::value_error(std::string(name) + " needs one entry (a 3-vector or None) per waypoint");
    py::sequence seq = py::reinterpret_borrow<py::sequence>(o);
    for (py::ssize_t w = 0; w < n; ++w) {
        py::object e = seq[w];
        if (e.is_none()) continue;
        if (w == 0 || w == n - 1)
            throw py::value_error(std::string(name) + ": the first and the last waypoint take initialVel / "
                                  "initialAcc and finalVel / finalAcc");
        mask[w] |= (uint8_t)(1u << (k - 1));
        read3(e, &values[((size_t)w * 4 + (k - 1)) * 3]);
    }
}

// The n rows a *_host call handed out (none when it failed: it raises) as an (n, 10) array, freed.
static py::array_t<double> take_rows(epp_status rc, double* rows, int64_t n) {
    if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
    if (rc != EPP_OK) throw std::runtime_error(epp_last_error());
    py::array_t<double> out({(py::ssize_t)n, (py::ssize_t)10});
    if (n) std::memcpy(out.mutable_data(), rows, (size_t)n * 10 * sizeof(double));
    epp_host_free(rows);
    return out;
}

static py::array_t<double> generate_trajectory(py::array_t<double, py::array::c_style | py::array::forcecast> waypoints,
                                               double v_max, double a_max, double sampling_intervall,
                                               double start_time_offset, py::object initial_vel,
                                               py::object initial_acc, bool enforce_limits,
                                               py::object thrust_limits, py::object optimize_times,
                                               py::object final_vel, py::object final_acc, py::object initial_jerk,
                                               py::object initial_snap, py::object waypoint_vel,
                                               py::object waypoint_acc) {
    if (waypoints.ndim() != 2 || waypoints.shape(1) != 3)
        throw std::invalid_argument("waypoints must be an (n, 3) array");
    double v0[3] = {0, 0, 0}, a0[3] = {0, 0, 0};
    read3(initial_vel, v0);
    read3(initial_acc, a0);
    // finalVel / finalAcc, initialJerk / initialSnap, waypointVel / waypointAcc: the fit under
    // these constraints (epp_generate_trajectory_constrained_host); none given: the calls
    // below, as before.  The time scalings and the time descent do not keep them (scaling
    // divides a pinned velocity by s, the descent refits without the pins), so the
    // combinations are refused.
    if (!(final_vel.is_none() && final_acc.is_none() && initial_jerk.is_none() && initial_snap.is_none() &&
          waypoint_vel.is_none() && waypoint_acc.is_none())) {
        const bool timeopt_asked = !optimize_times.is_none() &&
                                   !(py::isinstance<py::bool_>(optimize_times) && !optimize_times.cast<bool>());
        if (enforce_limits || !thrust_limits.is_none() || timeopt_asked)
            throw py::value_error("generate_trajectory: finalVel, finalAcc, initialJerk, initialSnap, waypointVel and "
                                  "waypointAcc do not combine with enforceLimits, thrustLimits or optimizeTimes");
        const py::ssize_t n = waypoints.shape(0);
        if (n < 2) throw std::invalid_argument("At least two waypoints are required");
        std::vector<uint8_t> mask((size_t)n, 0);
        std::vector<double> values((size_t)n * 12, 0.0);
        std::memcpy(&values[0], v0, sizeof(v0));
        std::memcpy(&values[3], a0, sizeof(a0));
        read3(initial_jerk, &values[6]);
        read3(initial_snap, &values[9]);
        read3(final_vel, &values[(size_t)(n - 1) * 12]);
        read3(final_acc, &values[(size_t)(n - 1) * 12 + 3]);
        read_waypoint_pins(waypoint_vel, 1, n, mask, values, "waypointVel");
        read_waypoint_pins(waypoint_acc, 2, n, mask, values, "waypointAcc");
        double* rows = nullptr;
        int64_t nr = 0;
        epp_status rc;
        {
            py::gil_scoped_release release;
            rc = epp_generate_trajectory_constrained_host(waypoints.data(), (int32_t)n, v_max, a_max, nullptr,
                                                          sampling_intervall, start_time_offset, mask.data(),
                                                          values.data(), &rows, &nr);
        }
        return take_rows(rc, rows, nr);
    }
    // thrustLimits = (g, f_min, f_max, rate_max, cos_tilt_min): the fit also time-scaled until
    // its thrust, body rate and tilt are within them (epp_traj_scale_to_thrust_limits),
    // independently of enforceLimits; None: the calls below, as before
    double tl[5] = {0, 0, 0, 0, 0};
    const bool flyable = !thrust_limits.is_none();
    if (flyable) {
        auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(thrust_limits);
        if (!a || a.size() != 5)
            throw std::invalid_argument("thrustLimits must be (g, f_min, f_max, rate_max, cos_tilt_min)");
        for (int i = 0; i < 5; ++i) tl[i] = a.data()[i];
    }
    // optimizeTimes = True | (max_iter, h, t_min): the segment times redistributed at constant
    // duration to lower the snap cost (epp_minsnap_optimize_times) before any scaling;
    // None / False: the calls below, as before
    epp_timeopt_params opt = EPP_TIMEOPT_DEFAULTS;
    bool timeopt = false;
    if (!optimize_times.is_none()) {
        if (py::isinstance<py::bool_>(optimize_times)) {
            timeopt = optimize_times.cast<bool>();
        } else {
            auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(optimize_times);
            if (!a || a.size() != 3) throw std::invalid_argument("optimizeTimes must be True or (max_iter, h, t_min)");
            if (!(a.data()[0] >= 0.0 && a.data()[0] <= 1e9)) throw std::invalid_argument("optimizeTimes: max_iter");
            opt.max_iter = (int32_t)a.data()[0];
            opt.h = a.data()[1];
            opt.t_min = a.data()[2];
            timeopt = true;
        }
    }
    double* rows = nullptr;
    int64_t n = 0;
    epp_status rc;
    if (timeopt) {
        py::gil_scoped_release release;
        rc = epp_generate_trajectory_timeopt_host(waypoints.data(), (int32_t)waypoints.shape(0), v_max, a_max,
                                                  sampling_intervall, start_time_offset, v0, a0, opt,
                                                  enforce_limits ? 1 : 0, flyable ? tl : nullptr, &rows, &n, nullptr,
                                                  nullptr, nullptr);
    } else if (flyable) {
        py::gil_scoped_release release;
        rc = epp_generate_trajectory_flyable_host(waypoints.data(), (int32_t)waypoints.shape(0), v_max, a_max,
                                                  sampling_intervall, start_time_offset, v0, a0, enforce_limits ? 1 : 0,
                                                  tl[0], tl[1], tl[2], tl[3], tl[4], &rows, &n, nullptr, nullptr);
    } else {
        py::gil_scoped_release release;
        // enforceLimits: the fit time-scaled until its peak speed and acceleration are within
        // v_max / a_max (Trajectory::scaleSegmentTimesToMeetConstraints, src/trajectory.cpp:385-429)
        rc = enforce_limits
                 ? epp_generate_trajectory_limited_host(waypoints.data(), (int32_t)waypoints.shape(0), v_max, a_max,
                                                        sampling_intervall, start_time_offset, v0, a0, &rows, &n,
                                                        nullptr)
                 : epp_generate_trajectory_host(waypoints.data(), (int32_t)waypoints.shape(0), v_max, a_max,
                                                sampling_intervall, start_time_offset, v0, a0, &rows, &n);
    }
    return take_rows(rc, rows, n);
}

// Trajectory::computeMaxVelocityAndAcceleration (src/trajectory.cpp:344-361) of the fit
// generate_trajectory samples: (v_peak, a_peak).
static py::tuple max_velocity_and_acceleration(py::array_t<double, py::array::c_style | py::array::forcecast> waypoints,
                                               double v_max, double a_max, py::object initial_vel,
                                               py::object initial_acc) {
    if (waypoints.ndim() != 2 || waypoints.shape(1) != 3)
        throw std::invalid_argument("waypoints must be an (n, 3) array");
    const int32_t W = (int32_t)waypoints.shape(0);
    if (W < 2) throw std::invalid_argument("At least two waypoints are required");
    double va[6] = {0, 0, 0, 0, 0, 0};
    read3(initial_vel, va);
    read3(initial_acc, va + 3);
    const int32_t M = W - 1, off[2] = {0, W};
    // one device block: [wp (3 W) | v0 a0 (6) | T (M) | coeffs (30 M) | peaks (4) | offsets, statuses (int32 x 4)]
    const size_t nd = (size_t)3 * W + 6 + (size_t)M * 31 + 4;
    double peaks[4] = {0, 0, 0, 0};
    int32_t st[2] = {0, 0};
    void* buf = nullptr;
    epp_status rc;
    {
        py::gil_scoped_release release;
        rc = epp_malloc(&buf, nd * 8 + 16);
        if (rc == EPP_OK) {
            double* d_wp = static_cast<double*>(buf);
            double* d_va = d_wp + 3 * W;
            double* d_T = d_va + 6;
            double* d_C = d_T + M;
            double* d_pk = d_C + (size_t)M * 30;
            int32_t* d_off = reinterpret_cast<int32_t*>(d_pk + 4);
            int32_t* d_st = d_off + 2;
            rc = epp_memcpy_h2d(d_wp, waypoints.data(), (size_t)W * 24, nullptr);
            if (rc == EPP_OK) rc = epp_memcpy_h2d(d_va, va, sizeof(va), nullptr);
            if (rc == EPP_OK) rc = epp_memcpy_h2d(d_off, off, sizeof(off), nullptr);
            if (rc == EPP_OK)
                rc = epp_minsnap_batch(d_wp, d_off, 1, v_max, a_max, d_va, d_va + 3, d_T, d_C, d_st, nullptr);
            if (rc == EPP_OK) rc = epp_traj_peaks(d_T, d_C, d_off, 1, d_pk, d_st + 1, nullptr);
            if (rc == EPP_OK) rc = epp_memcpy_d2h(peaks, d_pk, sizeof(peaks), nullptr);
            if (rc == EPP_OK) rc = epp_memcpy_d2h(st, d_st, sizeof(st), nullptr);
            epp_free(buf);
        }
    }
    if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
    if (rc != EPP_OK) throw std::runtime_error(epp_last_error());
    if (st[0] == -2) throw std::runtime_error("Segment times need to be greater than zero");
    if (st[0] != 0 || st[1] != 0) throw std::runtime_error("min-snap solve failed");
    return py::make_tuple(peaks[0], peaks[2]);
}

PYBIND11_MODULE(polynomial_trajectory, m) {
    m.doc() = "MI355X min-snap trajectory generation (drop-in for poly_traj::generateTrajectory)";
    m.def("generate_trajectory", &generate_trajectory, py::arg("waypoints"), py::arg("v_max"), py::arg("a_max"),
          py::arg("sampling_intervall"), py::arg("startTimeOffset") = 0.0, py::arg("initialVel") = py::none(),
          py::arg("initialAcc") = py::none(), py::arg("enforceLimits") = false,
          py::arg("thrustLimits") = py::none(), py::arg("optimizeTimes") = py::none(), py::kw_only(),
          py::arg("finalVel") = py::none(), py::arg("finalAcc") = py::none(), py::arg("initialJerk") = py::none(),
          py::arg("initialSnap") = py::none(), py::arg("waypointVel") = py::none(),
          py::arg("waypointAcc") = py::none());
    m.def("max_velocity_and_acceleration", &max_velocity_and_acceleration, py::arg("waypoints"), py::arg("v_max"),
          py::arg("a_max"), py::arg("initialVel") = py::none(), py::arg("initialAcc") = py::none());
}
