// host_candidates.cpp — epp::PathPlanner's checks of trajectories against the world: a
// sampled trajectory's rows (checkTrajectoryValidity*) and candidate waypoint sets, fitted
// and queried on the device in one batch (the *Candidate* / candidate* calls, each over one
// CandidateBatch: the fit, the call's own kernel or kernels, one synchronisation).
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>

#include "candidate_batch.h"
#include "epp/PathPlanner.h"
#include "epp/trajectory_generator.h"
#include "epp_internal.h"
#include "host_waypoints.h"

namespace epp {

namespace {
// The positions (columns 0, 3, 6) of a trajectory's rows as x, y, z.
void traj_xyz(const Matrix& traj, std::vector<double>& xyz) {
    xyz.resize(traj.rows * 3);
    for (size_t i = 0; i < traj.rows; ++i) {
        xyz[3 * i] = traj(i, 0);
        xyz[3 * i + 1] = traj(i, 3);
        xyz[3 * i + 2] = traj(i, 6);
    }
}
bool all_set(const std::vector<uint8_t>& ok) {
    return std::find(ok.begin(), ok.end(), uint8_t(0)) == ok.end();
}
}  // namespace

// PathPlanner::checkTrajectoryValidity — src/PathPlanner.cpp:267-280 (one batched launch)
bool PathPlanner::checkTrajectoryValidity(const Matrix& traj, double minDistance) const {
    return checkTrajectoryValidityOn(*worldPtr, traj, minDistance);
}

bool PathPlanner::checkTrajectoryValidityOn(const World& world, const Matrix& traj, double minDistance) {
    if (traj.rows == 0) return true;
    std::vector<double> xyz;
    traj_xyz(traj, xyz);
    std::vector<uint8_t> ok(traj.rows);
    world.checkPointsMinDistance(xyz.data(), (int64_t)traj.rows, minDistance, ok.data());
    return all_set(ok);
}

bool PathPlanner::checkTrajectoryValidityAndGenerate(const Matrix& traj, double minDistance,
                                                     const std::vector<Vec3>& waypoints, double vMax, double aMax,
                                                     double samplingInterval, double startTimeOffset, const Vec3& v0,
                                                     const Vec3& a0, Matrix& result) const {
    if (waypoints.size() < 2) throw std::invalid_argument("At least two waypoints are required");
    thread_local std::vector<double> xyz, wp;
    thread_local std::vector<uint8_t> ok;
    traj_xyz(traj, xyz);
    wp.clear();
    flatten(waypoints, wp);
    ok.assign(traj.rows, 0);
    const double v[3] = {v0.x, v0.y, v0.z}, a[3] = {a0.x, a0.y, a0.z};
    const FusedCheck chk{worldPtr->device(), xyz.data(), (int64_t)traj.rows, minDistance, ok.data()};
    Matrix tmp;
    std::swap(tmp, result);  // (result keeps its old value if the call throws)
    int64_t n = 0;
    const epp_status rc = check_and_generate_into(traj.rows ? &chk : nullptr, wp.data(), (int32_t)waypoints.size(),
                                                  nullptr, vMax, aMax, samplingInterval, startTimeOffset, v, a,
                                                  matrix_rows, &tmp, &n);
    if (rc == EPP_ERR_UNSUPPORTED) {  // (a large check: the two calls)
        std::swap(tmp, result);
        const bool valid = checkTrajectoryValidity(traj, minDistance);
        poly_traj::generateTrajectory(waypoints, vMax, aMax, samplingInterval, startTimeOffset, v0, a0, result);
        return valid;
    }
    if (rc != EPP_OK) {
        std::swap(tmp, result);
        if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
        throw std::runtime_error(std::string("generateTrajectory: ") + epp_last_error());
    }
    tmp.data.resize((size_t)n * 10);
    std::swap(tmp, result);
    return all_set(ok);
}

namespace {
// What every candidate call shares: the sets' host image and block layout (CandidateLayout;
// a short set throws before any device work), then -- after the call has reserved its own
// parts -- fit(): the one allocation, the stream, the uploads and the fit of every set
// (epp_minsnap_batch).  The call enqueues its kernels on stream() over the parts' device
// pointers, queues its downloads with fetch() and ends with finish(): the one synchronisation
// and the check of the fit's status.  A call copies what it fetched into the caller's vectors
// only after finish() has passed: after a throw they hold their defaults.  `what` names the
// call in the errors.  The stream and the block are released on every way out.
class CandidateBatch : public CandidateLayout {
public:
    CandidateBatch(const char* what, const std::vector<std::vector<Vec3>>& sets) : CandidateLayout(sets), what_(what) {}

    void need(epp_status rc) const {
        if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
        if (rc != EPP_OK) throw std::runtime_error(std::string(what_) + ": " + epp_last_error());
    }
    // An upload of the call's own (the gate frames), sent by fit() after the waypoints' two.
    template <class T>
    void upload(const Part<T>& p, const T* host) {
        uploads_.push_back({p.off, host, p.bytes()});
    }
    void fit(double v_max, double a_max) {
        need(epp_malloc(&d_.buf, bytes));
        need(epp_stream_create(&d_.st));
        need(epp_memcpy_h2d_async(dev(p_wp), wp.data(), p_wp.bytes(), d_.st));
        need(epp_memcpy_h2d_async(dev(p_off), off.data(), p_off.bytes(), d_.st));
        for (const Upload& u : uploads_)
            if (u.bytes) need(epp_memcpy_h2d_async(static_cast<char*>(d_.buf) + u.off, u.host, u.bytes, d_.st));
        need(epp_minsnap_batch(d_wp(), d_off(), count(), v_max, a_max, nullptr, nullptr, d_T(), d_C(), dev(p_fit),
                               d_.st));
    }
    template <class T>
    T* dev(const Part<T>& p) const {
        return reinterpret_cast<T*>(static_cast<char*>(d_.buf) + p.off);
    }
    const double* d_wp() const { return dev(p_wp); }
    const int32_t* d_off() const { return dev(p_off); }
    double* d_T() const { return dev(p_T); }
    double* d_C() const { return dev(p_C); }
    void* stream() const { return d_.st; }
    int32_t count() const { return (int32_t)n; }

    template <class T>
    void fetch(const Part<T>& p, T* host) {
        if (p.count) need(epp_memcpy_d2h_async(host, dev(p), p.bytes(), d_.st));
    }
    // stage: the status per set of the call's own kernel, fetched by the call (negative: failed).
    void finish(const int32_t* stage = nullptr) {
        std::vector<int32_t> fit_status(n);
        fetch(p_fit, fit_status.data());
        need(epp_stream_sync(d_.st));
        for (size_t k = 0; k < n; ++k)
            if (fit_status[k] != 0 || (stage && stage[k] < 0))
                throw std::runtime_error("generateTrajectory: the fit of waypoint set " + std::to_string(k) +
                                         " failed (status " +
                                         std::to_string(fit_status[k] != 0 ? fit_status[k] : stage[k]) + ")");
    }

private:
    struct Upload {
        size_t off;
        const void* host;
        size_t bytes;
    };
    struct Dev {  // released on every way out
        void* buf = nullptr;
        void* st = nullptr;
        ~Dev() {
            if (st) (void)epp_stream_destroy(st);
            if (buf) (void)epp_free(buf);
        }
    } d_;
    const char* what_;
    std::vector<Upload> uploads_;
};
}  // namespace

bool PathPlanner::checkCandidateTrajectories(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                             double dt, double minDistance, std::vector<long>& firstInvalidRow,
                                             std::vector<double>* firstInvalidTime) const {
    CandidateBatch b("checkCandidateTrajectories", sets);
    firstInvalidRow.assign(b.n, -1);
    if (firstInvalidTime) firstInvalidTime->assign(b.n, -1.0);
    if (b.n == 0) return true;
    const Part<int64_t> p_row = b.part<int64_t>(b.n);
    const Part<double> p_time = b.part<double>(b.n);
    b.fit(v_max, a_max);
    b.need(epp_traj_check_batch(worldPtr->device(), b.d_T(), b.d_C(), b.d_off(), b.count(), dt, minDistance,
                                b.dev(p_row), b.dev(p_time), b.stream()));
    std::vector<int64_t> rows(b.n);
    std::vector<double> times(b.n);
    b.fetch(p_row, rows.data());
    b.fetch(p_time, times.data());
    b.finish();
    firstInvalidRow.assign(rows.begin(), rows.end());
    if (firstInvalidTime) *firstInvalidTime = times;
    return std::all_of(rows.begin(), rows.end(), [](int64_t r) { return r < 0; });
}

// The first failing row (epp_traj_check_batch) and the first failing chord
// (epp_traj_sweep_batch) of every fitted track, on the one fit.
bool PathPlanner::sweepCandidateTrajectories(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                             double dt, double minDistance, bool canPassGate,
                                             std::vector<long>& firstInvalidRow, std::vector<long>& firstInvalidChord,
                                             std::vector<double>* firstInvalidTime) const {
    CandidateBatch b("sweepCandidateTrajectories", sets);
    firstInvalidRow.assign(b.n, -1);
    firstInvalidChord.assign(b.n, -1);
    if (firstInvalidTime) firstInvalidTime->assign(b.n, -1.0);
    if (b.n == 0) return true;
    const Part<int64_t> p_row = b.part<int64_t>(b.n), p_chord = b.part<int64_t>(b.n);
    const Part<double> p_row_time = b.part<double>(b.n), p_chord_time = b.part<double>(b.n);
    b.fit(v_max, a_max);
    const epp_world* world = worldPtr->device();
    b.need(epp_traj_check_batch(world, b.d_T(), b.d_C(), b.d_off(), b.count(), dt, minDistance, b.dev(p_row),
                                b.dev(p_row_time), b.stream()));
    b.need(epp_traj_sweep_batch(world, b.d_T(), b.d_C(), b.d_off(), b.count(), dt, canPassGate ? 1 : 0,
                                b.dev(p_chord), b.dev(p_chord_time), b.stream()));
    std::vector<int64_t> rows(b.n), chords(b.n);
    std::vector<double> rowTimes(b.n), chordTimes(b.n);
    b.fetch(p_row, rows.data());
    b.fetch(p_row_time, rowTimes.data());
    b.fetch(p_chord, chords.data());
    b.fetch(p_chord_time, chordTimes.data());
    b.finish();
    firstInvalidRow.assign(rows.begin(), rows.end());
    firstInvalidChord.assign(chords.begin(), chords.end());
    bool all = true;
    for (size_t k = 0; k < b.n; ++k) {
        const int64_t r = rows[k], c = chords[k];
        all = all && r < 0 && c < 0;
        // the earlier of the two findings (a failing row j and a failing chord j start at the same time)
        if (firstInvalidTime && (r >= 0 || c >= 0))
            (*firstInvalidTime)[k] = (c < 0 || (r >= 0 && r <= c)) ? rowTimes[k] : chordTimes[k];
    }
    return all;
}

// The first hit of every fitted track (epp_traj_first_hit_batch): the first failing chord, the
// entry parameter along it, the hit's time and the OBB.
void PathPlanner::candidateFirstHits(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max, double dt,
                                     bool canPassGate, std::vector<long>& chord, std::vector<double>& t,
                                     std::vector<double>* time, std::vector<int>* obb) const {
    CandidateBatch b("candidateFirstHits", sets);
    chord.assign(b.n, -1);
    t.assign(b.n, HUGE_VAL);
    if (time) time->assign(b.n, -1.0);
    if (obb) obb->assign(b.n, -1);
    if (b.n == 0) return;
    const Part<int64_t> p_chord = b.part<int64_t>(b.n);
    const Part<double> p_t = b.part<double>(b.n), p_time = b.part<double>(b.n);
    const Part<int32_t> p_obb = b.part<int32_t>(b.n);
    b.fit(v_max, a_max);
    b.need(epp_traj_first_hit_batch(worldPtr->device(), b.d_T(), b.d_C(), b.d_off(), b.count(), dt,
                                    canPassGate ? 1 : 0, b.dev(p_chord), b.dev(p_t), b.dev(p_time), b.dev(p_obb),
                                    b.stream()));
    std::vector<int64_t> chords(b.n);
    std::vector<double> ts(b.n), times(b.n);
    std::vector<int32_t> obbs(b.n);
    b.fetch(p_chord, chords.data());
    b.fetch(p_time, times.data());
    b.fetch(p_t, ts.data());
    b.fetch(p_obb, obbs.data());
    b.finish();
    chord.assign(chords.begin(), chords.end());
    t = ts;
    if (time) *time = times;
    if (obb) obb->assign(obbs.begin(), obbs.end());
}

// The closest approach of every fitted track's rows (epp_traj_clearance_batch): the distance,
// the row, its time and the nearest OBB.
void PathPlanner::candidateClearances(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max, double dt,
                                      std::vector<double>& clearance, std::vector<long>* row,
                                      std::vector<double>* time, std::vector<int>* nearest) const {
    CandidateBatch b("candidateClearances", sets);
    clearance.assign(b.n, HUGE_VAL);
    if (row) row->assign(b.n, -1);
    if (time) time->assign(b.n, -1.0);
    if (nearest) nearest->assign(b.n, -1);
    if (b.n == 0) return;
    const Part<double> p_clr = b.part<double>(b.n), p_time = b.part<double>(b.n);
    const Part<int64_t> p_row = b.part<int64_t>(b.n);
    const Part<int32_t> p_near = b.part<int32_t>(b.n);
    b.fit(v_max, a_max);
    b.need(epp_traj_clearance_batch(worldPtr->device(), b.d_T(), b.d_C(), b.d_off(), b.count(), dt, b.dev(p_clr),
                                    b.dev(p_row), b.dev(p_time), b.dev(p_near), b.stream()));
    std::vector<double> clr(b.n), times(b.n);
    std::vector<int64_t> rows(b.n);
    std::vector<int32_t> near(b.n);
    b.fetch(p_row, rows.data());
    b.fetch(p_time, times.data());
    b.fetch(p_clr, clr.data());
    b.fetch(p_near, near.data());
    b.finish();
    clearance = clr;
    if (row) row->assign(rows.begin(), rows.end());
    if (time) *time = times;
    if (nearest) nearest->assign(near.begin(), near.end());
}

// The closest approach of every fitted track's chords (epp_traj_chord_clearance_batch): the
// distance, the chord, the parameter along it, the time of that point and the nearest OBB.
void PathPlanner::candidateSweptClearances(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                           double dt, std::vector<double>& clearance, std::vector<long>* chord,
                                           std::vector<double>* t, std::vector<double>* time,
                                           std::vector<int>* nearest) const {
    CandidateBatch b("candidateSweptClearances", sets);
    clearance.assign(b.n, HUGE_VAL);
    if (chord) chord->assign(b.n, -1);
    if (t) t->assign(b.n, -1.0);
    if (time) time->assign(b.n, -1.0);
    if (nearest) nearest->assign(b.n, -1);
    if (b.n == 0) return;
    const Part<double> p_clr = b.part<double>(b.n), p_t = b.part<double>(b.n), p_time = b.part<double>(b.n);
    const Part<int64_t> p_chord = b.part<int64_t>(b.n);
    const Part<int32_t> p_near = b.part<int32_t>(b.n);
    b.fit(v_max, a_max);
    b.need(epp_traj_chord_clearance_batch(worldPtr->device(), b.d_T(), b.d_C(), b.d_off(), b.count(), dt, b.dev(p_clr),
                                          b.dev(p_chord), b.dev(p_t), b.dev(p_time), b.dev(p_near), b.stream()));
    std::vector<double> clr(b.n), ts(b.n), times(b.n);
    std::vector<int64_t> chords(b.n);
    std::vector<int32_t> near(b.n);
    b.fetch(p_chord, chords.data());
    b.fetch(p_t, ts.data());
    b.fetch(p_time, times.data());
    b.fetch(p_clr, clr.data());
    b.fetch(p_near, near.data());
    b.finish();
    clearance = clr;
    if (chord) chord->assign(chords.begin(), chords.end());
    if (t) *t = ts;
    if (time) *time = times;
    if (nearest) nearest->assign(near.begin(), near.end());
}

// The room a waypoint polyline leaves: the minimum of World::edgeClearances over its edges, the
// earliest edge among equals.
double PathPlanner::pathClearance(const std::vector<Vec3>& path, long* edge, double* t, int* nearest) const {
    if (path.size() < 2) throw std::invalid_argument("pathClearance: a path has at least two points");
    std::vector<double> xyz;
    flatten(path, xyz);
    const int64_t n = (int64_t)path.size() - 1;
    std::vector<double> dist(n), ts(n);
    std::vector<int32_t> near(n);
    worldPtr->edgeClearances(xyz.data(), xyz.data() + 3, n, dist.data(), ts.data(), near.data());
    int64_t j = -1;
    double best = HUGE_VAL;
    for (int64_t i = 0; i < n; ++i)
        if (dist[i] < best) {
            best = dist[i];
            j = i;
        }
    if (edge) *edge = (long)j;
    if (t) *t = j < 0 ? -1.0 : ts[j];
    if (nearest) *nearest = j < 0 ? -1 : near[j];
    return best;
}

// The gate centre and cos / sin of the yaw per gate row: getGateCenterAndNormal's centre
// (src/OnlineTrajGenerator.cpp:50-70) and checkGatePassed's c, s (:236).
Matrix PathPlanner::gateFrames(const Matrix& gates) const {
    if (gates.rows && gates.cols < 7) throw std::invalid_argument("gateFrames: gate rows have 7 columns");
    Matrix f(gates.rows, 5);
    for (size_t g = 0; g < gates.rows; ++g) {
        const double* r = gates.row(g);
        if (r[3] != 0 || r[4] != 0)
            throw std::invalid_argument("gateFrames: Only simple rotation around z axis is supported");
        f(g, 0) = r[0];
        f(g, 1) = r[1];
        f(g, 2) = r[2] + configParser->getObjectPropertiesByTypeId((int)r[6]).height;
        f(g, 3) = std::cos(r[5]);
        f(g, 4) = std::sin(r[5]);
    }
    return f;
}

// The ordered gate passage of every fitted track (epp_traj_gate_pass_batch) against the frame
// table, uploaded with the waypoints.  Gates are no OBBs: no world takes part.
void PathPlanner::candidateGatePasses(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max, double dt,
                                      const Matrix& frames, double halfEdge, std::vector<long>& chord,
                                      std::vector<double>& time, std::vector<int>& nPassed,
                                      std::vector<double>* offsets) const {
    if (frames.cols != 5 || frames.rows > 64)
        throw std::invalid_argument("candidateGatePasses: the gate frame table must be (G <= 64) x 5");
    CandidateBatch b("candidateGatePasses", sets);
    const size_t G = frames.rows, nG = b.n * G;
    chord.assign(nG, -1);
    time.assign(nG, -1.0);
    nPassed.assign(b.n, 0);
    if (offsets) offsets->assign(nG * 2, NAN);
    if (b.n == 0) return;
    const Part<double> p_frames = b.part<double>(G * 5);
    const Part<int64_t> p_chord = b.part<int64_t>(nG);
    const Part<double> p_time = b.part<double>(nG), p_offsets = b.part<double>(offsets ? nG * 2 : 0);
    const Part<int32_t> p_passed = b.part<int32_t>(b.n);
    b.upload(p_frames, frames.data.data());
    b.fit(v_max, a_max);
    b.need(epp_traj_gate_pass_batch(b.dev(p_frames), (int32_t)G, halfEdge, b.d_T(), b.d_C(), b.d_off(), b.count(), dt,
                                    b.dev(p_chord), b.dev(p_time), offsets ? b.dev(p_offsets) : nullptr,
                                    b.dev(p_passed), b.stream()));
    std::vector<int64_t> chords(nG);
    std::vector<double> times(nG), offs(p_offsets.count);
    std::vector<int32_t> passed(b.n);
    b.fetch(p_passed, passed.data());
    b.fetch(p_chord, chords.data());
    b.fetch(p_time, times.data());
    b.fetch(p_offsets, offs.data());
    b.finish();
    chord.assign(chords.begin(), chords.end());
    time = times;
    nPassed.assign(passed.begin(), passed.end());
    if (offsets) *offsets = offs;
}

// The extremes of thrust, body rate and tilt of every fitted track's rows
// (epp_traj_thrust_rates_batch): n x 8 values and the n x 4 rows that attain them; no world
// takes part.
void PathPlanner::candidateThrustRates(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                       double dt, double g, std::vector<double>& out, std::vector<long>* rows) const {
    CandidateBatch b("candidateThrustRates", sets);
    out.resize(b.n * 8);
    for (size_t k = 0; k < b.n; ++k) {
        const double identity[8] = {HUGE_VAL, -1.0, -HUGE_VAL, -1.0, -HUGE_VAL, -1.0, HUGE_VAL, -1.0};
        std::copy(identity, identity + 8, out.begin() + 8 * k);
    }
    if (rows) rows->assign(b.n * 4, -1);
    if (b.n == 0) return;
    const Part<double> p_out = b.part<double>(b.n * 8);
    const Part<int64_t> p_rows = b.part<int64_t>(rows ? b.n * 4 : 0);
    b.fit(v_max, a_max);
    b.need(epp_traj_thrust_rates_batch(b.d_T(), b.d_C(), b.d_off(), b.count(), dt, g, b.dev(p_out),
                                       rows ? b.dev(p_rows) : nullptr, b.stream()));
    std::vector<double> vals(p_out.count);
    std::vector<int64_t> at(p_rows.count);
    b.fetch(p_out, vals.data());
    b.fetch(p_rows, at.data());
    b.finish();
    out = vals;
    if (rows) rows->assign(at.begin(), at.end());
}

// The thrust-limit search (epp_traj_scale_to_thrust_limits) on every fitted track: the scale,
// the scaled duration, the search's status and the limits violated.
void PathPlanner::candidateFlyableScales(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                         const FlightLimits& lim, std::vector<double>& scale,
                                         std::vector<double>& duration, std::vector<int>& status,
                                         std::vector<int>* violated) const {
    CandidateBatch b("candidateFlyableScales", sets);
    scale.assign(b.n, 1.0);
    duration.assign(b.n, 0.0);
    status.assign(b.n, 0);
    if (violated) violated->assign(b.n, 0);
    if (b.n == 0) {  // (the limits are checked all the same)
        b.need(epp_traj_scale_to_thrust_limits(nullptr, nullptr, nullptr, 0, lim.g, lim.fMin, lim.fMax, lim.rateMax,
                                               lim.cosTiltMin, nullptr, nullptr, nullptr, nullptr));
        return;
    }
    const Part<double> p_scale = b.part<double>(b.n);
    const Part<int32_t> p_status = b.part<int32_t>(b.n), p_violated = b.part<int32_t>(b.n);
    b.fit(v_max, a_max);
    b.need(epp_traj_scale_to_thrust_limits(b.d_T(), b.d_C(), b.d_off(), b.count(), lim.g, lim.fMin, lim.fMax,
                                           lim.rateMax, lim.cosTiltMin, b.dev(p_scale), b.dev(p_status),
                                           b.dev(p_violated), b.stream()));
    std::vector<int32_t> st(b.n), vi(b.n);
    std::vector<double> sc(b.n), T(b.nseg);
    b.fetch(p_status, st.data());
    b.fetch(p_violated, vi.data());
    b.fetch(p_scale, sc.data());
    b.fetch(b.p_T, T.data());
    b.finish(st.data());
    for (size_t k = 0; k < b.n; ++k) {
        double sum = 0.0;  // in order, as Trajectory accumulates the segment times
        for (size_t i = b.seg_begin(k); i < b.seg_begin(k + 1); ++i) sum += T[i];
        duration[k] = sum;
    }
    scale = sc;
    status.assign(st.begin(), st.end());
    if (violated) violated->assign(vi.begin(), vi.end());
}

// The snap cost of every fitted track (epp_traj_snap_cost), or the descent over its segment
// times (epp_minsnap_optimize_times) and the result's cost; and the segment times.
void PathPlanner::candidateSnapCosts(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                     bool optimize, std::vector<double>& costs,
                                     std::vector<std::vector<double>>* times) const {
    CandidateBatch b("candidateSnapCosts", sets);
    costs.assign(b.n, 0.0);
    if (times) times->assign(b.n, {});
    if (b.n == 0) return;
    const Part<double> p_cost0 = b.part<double>(optimize ? b.n : 0), p_cost = b.part<double>(b.n);
    const Part<int32_t> p_iters = b.part<int32_t>(optimize ? b.n : 0), p_status = b.part<int32_t>(b.n);
    b.fit(v_max, a_max);
    if (optimize) {
        const epp_timeopt_params prm = EPP_TIMEOPT_DEFAULTS;
        b.need(epp_minsnap_optimize_times(b.d_wp(), b.d_off(), b.count(), nullptr, nullptr, b.d_T(), b.d_C(), prm,
                                          b.dev(p_cost0), b.dev(p_cost), b.dev(p_iters), b.dev(p_status),
                                          b.stream()));
    } else {
        b.need(epp_traj_snap_cost(b.d_T(), b.d_C(), b.d_off(), b.count(), b.dev(p_cost), b.dev(p_status),
                                  b.stream()));
    }
    std::vector<int32_t> st(b.n);
    std::vector<double> J(b.n), T(b.nseg);
    b.fetch(p_status, st.data());
    b.fetch(p_cost, J.data());
    b.fetch(b.p_T, T.data());
    b.finish(st.data());
    costs = J;
    if (times)
        for (size_t k = 0; k < b.n; ++k) (*times)[k].assign(T.begin() + b.seg_begin(k), T.begin() + b.seg_begin(k + 1));
}

}  // namespace epp
