// host_candidates.cpp — epp::PathPlanner's checks of trajectories against the world: a
// sampled trajectory's rows (checkTrajectoryValidity*) and candidate waypoint sets, fitted
// and checked on the device in one batch (the three *Candidate* calls).
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "epp/PathPlanner.h"
#include "epp/trajectory_generator.h"
#include "epp_internal.h"

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
    wp.resize(waypoints.size() * 3);
    for (size_t i = 0; i < waypoints.size(); ++i) {
        wp[3 * i] = waypoints[i].x;
        wp[3 * i + 1] = waypoints[i].y;
        wp[3 * i + 2] = waypoints[i].z;
    }
    ok.assign(traj.rows, 0);
    const double v[3] = {v0.x, v0.y, v0.z}, a[3] = {a0.x, a0.y, a0.z};
    const FusedCheck chk{worldPtr->device(), xyz.data(), (int64_t)traj.rows, minDistance, ok.data()};
    Matrix tmp;
    std::swap(tmp, result);  // (result keeps its old value if the call throws)
    auto into = [](void* ctx, int64_t R) -> double* {
        Matrix& m = *static_cast<Matrix*>(ctx);
        m.rows = (size_t)R;
        m.cols = 10;
        m.data.resize((size_t)std::max<int64_t>(R, 1) * 10);
        return m.data.data();
    };
    int64_t n = 0;
    const epp_status rc = check_and_generate_into(traj.rows ? &chk : nullptr, wp.data(), (int32_t)waypoints.size(),
                                                  nullptr, vMax, aMax, samplingInterval, startTimeOffset, v, a, into,
                                                  &tmp, &n);
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
// The fit of every waypoint set (epp_minsnap_batch) and, on the same device buffers and
// stream, the first failing row (epp_traj_check_batch) and -- chords != nullptr -- the first
// failing chord (epp_traj_sweep_batch) of every fitted track; one synchronisation, at the end.
// `what` names the caller in the errors.  clr != nullptr: instead of the two checks, the
// closest approach of every fitted track's rows (epp_traj_clearance_batch) into *clr, the row
// into firstInvalidRow and its time into rowTimes -- the same upload, fit, stream and single
// synchronisation.  hit != nullptr: likewise the first hit of every fitted track
// (epp_traj_first_hit_batch): the entry parameter into *hit, the chord into firstInvalidRow
// and the hit's time into rowTimes.  gp != nullptr: instead of the checks, the ordered gate
// passage of every fitted track (epp_traj_gate_pass_batch) against gp's frame table, uploaded
// with the waypoints; its n x G outputs take a part of the device block of their own.  Gates
// are no OBBs: no world takes part.  tr != nullptr: instead of the checks, the extremes of thrust,
// body rate and tilt of every fitted track's rows (epp_traj_thrust_rates_batch) into tr's n x 8
// and n x 4 outputs, which take a part of the device block of their own; no world takes part.
struct CandidateClear {
    std::vector<double>& clearance;
    std::vector<int>* nearest;
};
struct CandidateHit {
    std::vector<double>& t;
    std::vector<int>* obb;
};
struct CandidateGates {
    const Matrix& frames;  // G x 5
    double halfEdge;
    std::vector<long>& chord;   // n x G
    std::vector<double>& time;  // n x G
    std::vector<int>& nPassed;  // n
    std::vector<double>* offsets;  // n x G x 2
};
struct CandidateThrust {
    double g;
    std::vector<double>& out;  // n x 8
    std::vector<long>* rows;   // n x 4
};
void fit_and_check_candidates(const char* what, const epp_world* world, const std::vector<std::vector<Vec3>>& sets,
                              double v_max, double a_max, double dt, double minDistance, int32_t canPassGate,
                              std::vector<long>& firstInvalidRow, std::vector<double>* rowTimes,
                              std::vector<long>* chords, std::vector<double>* chordTimes,
                              const CandidateClear* clr = nullptr, const CandidateHit* hit = nullptr,
                              const CandidateGates* gp = nullptr, const CandidateThrust* tr = nullptr) {
    if (gp && (gp->frames.cols != 5 || gp->frames.rows > 64))
        throw std::invalid_argument(std::string(what) + ": the gate frame table must be (G <= 64) x 5");
    for (const auto& s : sets)
        if (s.size() < 2) throw std::invalid_argument("At least two waypoints are required");
    const size_t n = sets.size();
    firstInvalidRow.assign(n, -1);
    if (rowTimes) rowTimes->assign(n, -1.0);
    if (chords) chords->assign(n, -1);
    if (chordTimes) chordTimes->assign(n, -1.0);
    if (clr) {
        clr->clearance.assign(n, HUGE_VAL);
        if (clr->nearest) clr->nearest->assign(n, -1);
    }
    if (hit) {
        hit->t.assign(n, HUGE_VAL);
        if (hit->obb) hit->obb->assign(n, -1);
    }
    const size_t G = gp ? gp->frames.rows : 0;
    if (gp) {
        gp->chord.assign(n * G, -1);
        gp->time.assign(n * G, -1.0);
        gp->nPassed.assign(n, 0);
        if (gp->offsets) gp->offsets->assign(n * G * 2, NAN);
    }
    if (tr) {
        tr->out.resize(n * 8);
        for (size_t k = 0; k < n; ++k) {
            const double identity[8] = {HUGE_VAL, -1.0, -HUGE_VAL, -1.0, -HUGE_VAL, -1.0, HUGE_VAL, -1.0};
            std::copy(identity, identity + 8, tr->out.begin() + 8 * k);
        }
        if (tr->rows) tr->rows->assign(n * 4, -1);
    }
    if (n == 0) return;
    // host image of the upload: [waypoints | offsets]; device block: [wp | T | coeffs |
    // first_time | first_invalid | chord_time | chord | offsets | status | gate parts | thrust parts]
    size_t total = 0;
    for (const auto& s : sets) total += s.size();
    const size_t nseg = total - n;
    std::vector<double> wp(total * 3);
    std::vector<int32_t> off(n + 1, 0);
    size_t w = 0;
    for (size_t k = 0; k < n; ++k) {
        for (const Vec3& p : sets[k]) {
            wp[3 * w] = p.x;
            wp[3 * w + 1] = p.y;
            wp[3 * w + 2] = p.z;
            ++w;
        }
        off[k + 1] = (int32_t)w;
    }
    struct Dev {  // released on every way out
        void* buf = nullptr;
        void* st = nullptr;
        ~Dev() {
            if (st) (void)epp_stream_destroy(st);
            if (buf) (void)epp_free(buf);
        }
    } d;
    auto need = [what](epp_status rc) {
        if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
        if (rc != EPP_OK) throw std::runtime_error(std::string(what) + ": " + epp_last_error());
    };
    auto after = [](size_t o, size_t b) { return (o + b + 255) & ~(size_t)255; };  // 256-B aligned parts
    const size_t o_wp = 0, o_T = after(o_wp, total * 24), o_C = after(o_T, nseg * 8), o_ft = after(o_C, nseg * 240),
                 o_fi = after(o_ft, n * 8), o_ct = after(o_fi, n * 8), o_ci = after(o_ct, n * 8),
                 o_off = after(o_ci, n * 8), o_st = after(o_off, (n + 1) * 4), o_gf = after(o_st, n * 4),
                 o_gc = after(o_gf, G * 40), o_gt = after(o_gc, n * G * 8), o_go = after(o_gt, n * G * 8),
                 o_gn = after(o_go, n * G * 16), o_to = after(o_gn, gp ? n * 4 : 0),
                 o_tr = after(o_to, tr ? n * 64 : 0), bytes = after(o_tr, tr ? n * 32 : 0);
    need(epp_malloc(&d.buf, bytes));
    need(epp_stream_create(&d.st));
    char* base = static_cast<char*>(d.buf);
    need(epp_memcpy_h2d_async(base + o_wp, wp.data(), total * 24, d.st));
    need(epp_memcpy_h2d_async(base + o_off, off.data(), (n + 1) * 4, d.st));
    if (G) need(epp_memcpy_h2d_async(base + o_gf, gp->frames.data.data(), G * 40, d.st));
    double* d_T = reinterpret_cast<double*>(base + o_T);
    double* d_C = reinterpret_cast<double*>(base + o_C);
    const int32_t* d_off = reinterpret_cast<const int32_t*>(base + o_off);
    need(epp_minsnap_batch(reinterpret_cast<const double*>(base + o_wp), d_off, (int32_t)n, v_max, a_max, nullptr,
                           nullptr, d_T, d_C, reinterpret_cast<int32_t*>(base + o_st), d.st));
    if (gp)
        need(epp_traj_gate_pass_batch(reinterpret_cast<const double*>(base + o_gf), (int32_t)G, gp->halfEdge, d_T, d_C,
                                      d_off, (int32_t)n, dt, reinterpret_cast<int64_t*>(base + o_gc),
                                      reinterpret_cast<double*>(base + o_gt),
                                      gp->offsets ? reinterpret_cast<double*>(base + o_go) : nullptr,
                                      reinterpret_cast<int32_t*>(base + o_gn), d.st));
    else if (tr)
        need(epp_traj_thrust_rates_batch(d_T, d_C, d_off, (int32_t)n, dt, tr->g, reinterpret_cast<double*>(base + o_to),
                                         tr->rows ? reinterpret_cast<int64_t*>(base + o_tr) : nullptr, d.st));
    else if (clr)  // (the chord slots hold the clearance and the nearest OBB)
        need(epp_traj_clearance_batch(world, d_T, d_C, d_off, (int32_t)n, dt, reinterpret_cast<double*>(base + o_ct),
                                      reinterpret_cast<int64_t*>(base + o_fi), reinterpret_cast<double*>(base + o_ft),
                                      reinterpret_cast<int32_t*>(base + o_ci), d.st));
    else if (hit)  // (the chord slots hold the entry parameter and the OBB)
        need(epp_traj_first_hit_batch(world, d_T, d_C, d_off, (int32_t)n, dt, canPassGate,
                                      reinterpret_cast<int64_t*>(base + o_fi), reinterpret_cast<double*>(base + o_ct),
                                      reinterpret_cast<double*>(base + o_ft), reinterpret_cast<int32_t*>(base + o_ci),
                                      d.st));
    else
        need(epp_traj_check_batch(world, d_T, d_C, d_off, (int32_t)n, dt, minDistance,
                                  reinterpret_cast<int64_t*>(base + o_fi), reinterpret_cast<double*>(base + o_ft),
                                  d.st));
    if (chords)
        need(epp_traj_sweep_batch(world, d_T, d_C, d_off, (int32_t)n, dt, canPassGate,
                                  reinterpret_cast<int64_t*>(base + o_ci), reinterpret_cast<double*>(base + o_ct),
                                  d.st));
    std::vector<int32_t> status(n);
    std::vector<int64_t> rows(n), crows(n);
    std::vector<double> times(n), ctimes(n);
    need(epp_memcpy_d2h_async(status.data(), base + o_st, n * 4, d.st));
    if (!gp && !tr) {
        need(epp_memcpy_d2h_async(rows.data(), base + o_fi, n * 8, d.st));
        need(epp_memcpy_d2h_async(times.data(), base + o_ft, n * 8, d.st));
    }
    std::vector<int64_t> gchord(n * G);
    std::vector<int32_t> gpassed(gp ? n : 0);
    if (gp) {
        need(epp_memcpy_d2h_async(gpassed.data(), base + o_gn, n * 4, d.st));
        if (G) {
            need(epp_memcpy_d2h_async(gchord.data(), base + o_gc, n * G * 8, d.st));
            need(epp_memcpy_d2h_async(gp->time.data(), base + o_gt, n * G * 8, d.st));
            if (gp->offsets) need(epp_memcpy_d2h_async(gp->offsets->data(), base + o_go, n * G * 16, d.st));
        }
    }
    std::vector<int64_t> trows(tr && tr->rows ? n * 4 : 0);
    std::vector<double> tout(tr ? n * 8 : 0);  // (tr->out keeps the identities if the call throws)
    if (tr) {
        need(epp_memcpy_d2h_async(tout.data(), base + o_to, n * 64, d.st));
        if (tr->rows) need(epp_memcpy_d2h_async(trows.data(), base + o_tr, n * 32, d.st));
    }
    if (chords) {
        need(epp_memcpy_d2h_async(crows.data(), base + o_ci, n * 8, d.st));
        need(epp_memcpy_d2h_async(ctimes.data(), base + o_ct, n * 8, d.st));
    }
    std::vector<int32_t> near(clr || hit ? n : 0);
    if (clr || hit) {
        need(epp_memcpy_d2h_async((clr ? clr->clearance : hit->t).data(), base + o_ct, n * 8, d.st));
        need(epp_memcpy_d2h_async(near.data(), base + o_ci, n * 4, d.st));
    }
    need(epp_stream_sync(d.st));
    for (size_t k = 0; k < n; ++k)
        if (status[k] != 0)
            throw std::runtime_error("generateTrajectory: the fit of waypoint set " + std::to_string(k) +
                                     " failed (status " + std::to_string(status[k]) + ")");
    for (size_t k = 0; k < n; ++k) {
        firstInvalidRow[k] = (long)rows[k];
        if (chords) (*chords)[k] = (long)crows[k];
    }
    if (rowTimes) *rowTimes = times;
    if (chords && chordTimes) *chordTimes = ctimes;
    if (clr && clr->nearest) clr->nearest->assign(near.begin(), near.end());
    if (hit && hit->obb) hit->obb->assign(near.begin(), near.end());
    if (gp) {
        gp->chord.assign(gchord.begin(), gchord.end());
        gp->nPassed.assign(gpassed.begin(), gpassed.end());
    }
    if (tr) tr->out = tout;
    if (tr && tr->rows) tr->rows->assign(trows.begin(), trows.end());
}
}  // namespace

void PathPlanner::candidateFirstHits(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max, double dt,
                                     bool canPassGate, std::vector<long>& chord, std::vector<double>& t,
                                     std::vector<double>* time, std::vector<int>* obb) const {
    const CandidateHit hit{t, obb};
    fit_and_check_candidates("candidateFirstHits", sets.empty() ? nullptr : worldPtr->device(), sets, v_max, a_max, dt,
                             0.0, canPassGate ? 1 : 0, chord, time, nullptr, nullptr, nullptr, &hit);
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

void PathPlanner::candidateGatePasses(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max, double dt,
                                      const Matrix& frames, double halfEdge, std::vector<long>& chord,
                                      std::vector<double>& time, std::vector<int>& nPassed,
                                      std::vector<double>* offsets) const {
    std::vector<long> rows;
    const CandidateGates gp{frames, halfEdge, chord, time, nPassed, offsets};
    fit_and_check_candidates("candidateGatePasses", nullptr, sets, v_max, a_max, dt, 0.0, 0, rows, nullptr, nullptr,
                             nullptr, nullptr, nullptr, &gp);
}

void PathPlanner::candidateThrustRates(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                       double dt, double g, std::vector<double>& out, std::vector<long>* rows) const {
    std::vector<long> none;
    const CandidateThrust tr{g, out, rows};
    fit_and_check_candidates("candidateThrustRates", nullptr, sets, v_max, a_max, dt, 0.0, 0, none, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, &tr);
}

// The fit of every set and the thrust-limit search (epp_traj_scale_to_thrust_limits) on one
// stream, one synchronisation; device block: [wp | T | offsets | fit status | scale | status |
// violated | coeffs].
void PathPlanner::candidateFlyableScales(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                         const FlightLimits& lim, std::vector<double>& scale,
                                         std::vector<double>& duration, std::vector<int>& status,
                                         std::vector<int>* violated) const {
    const char* what = "candidateFlyableScales";
    for (const auto& s : sets)
        if (s.size() < 2) throw std::invalid_argument("At least two waypoints are required");
    const size_t n = sets.size();
    scale.assign(n, 1.0);
    duration.assign(n, 0.0);
    status.assign(n, 0);
    if (violated) violated->assign(n, 0);
    auto need = [what](epp_status rc) {
        if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
        if (rc != EPP_OK) throw std::runtime_error(std::string(what) + ": " + epp_last_error());
    };
    if (n == 0) {  // (the limits are checked all the same)
        need(epp_traj_scale_to_thrust_limits(nullptr, nullptr, nullptr, 0, lim.g, lim.fMin, lim.fMax, lim.rateMax,
                                             lim.cosTiltMin, nullptr, nullptr, nullptr, nullptr));
        return;
    }
    size_t total = 0;
    for (const auto& s : sets) total += s.size();
    const size_t nseg = total - n;
    std::vector<double> wp(total * 3);
    std::vector<int32_t> off(n + 1, 0);
    size_t w = 0;
    for (size_t k = 0; k < n; ++k) {
        for (const Vec3& p : sets[k]) {
            wp[3 * w] = p.x;
            wp[3 * w + 1] = p.y;
            wp[3 * w + 2] = p.z;
            ++w;
        }
        off[k + 1] = (int32_t)w;
    }
    struct Dev {  // released on every way out
        void* buf = nullptr;
        void* st = nullptr;
        ~Dev() {
            if (st) (void)epp_stream_destroy(st);
            if (buf) (void)epp_free(buf);
        }
    } d;
    auto after = [](size_t o, size_t b) { return (o + b + 255) & ~(size_t)255; };  // 256-B aligned parts
    const size_t o_wp = 0, o_T = after(o_wp, total * 24), o_off = after(o_T, nseg * 8),
                 o_fs = after(o_off, (n + 1) * 4), o_sc = after(o_fs, n * 4), o_st = after(o_sc, n * 8),
                 o_vi = after(o_st, n * 4), o_C = after(o_vi, n * 4), bytes = after(o_C, nseg * 240);
    need(epp_malloc(&d.buf, bytes));
    need(epp_stream_create(&d.st));
    char* base = static_cast<char*>(d.buf);
    need(epp_memcpy_h2d_async(base + o_wp, wp.data(), total * 24, d.st));
    need(epp_memcpy_h2d_async(base + o_off, off.data(), (n + 1) * 4, d.st));
    double* d_T = reinterpret_cast<double*>(base + o_T);
    double* d_C = reinterpret_cast<double*>(base + o_C);
    const int32_t* d_off = reinterpret_cast<const int32_t*>(base + o_off);
    need(epp_minsnap_batch(reinterpret_cast<const double*>(base + o_wp), d_off, (int32_t)n, v_max, a_max, nullptr,
                           nullptr, d_T, d_C, reinterpret_cast<int32_t*>(base + o_fs), d.st));
    need(epp_traj_scale_to_thrust_limits(d_T, d_C, d_off, (int32_t)n, lim.g, lim.fMin, lim.fMax, lim.rateMax,
                                         lim.cosTiltMin, reinterpret_cast<double*>(base + o_sc),
                                         reinterpret_cast<int32_t*>(base + o_st),
                                         reinterpret_cast<int32_t*>(base + o_vi), d.st));
    std::vector<int32_t> fit(n), st(n), vi(n);
    std::vector<double> sc(n), T(nseg);
    need(epp_memcpy_d2h_async(fit.data(), base + o_fs, n * 4, d.st));
    need(epp_memcpy_d2h_async(st.data(), base + o_st, n * 4, d.st));
    need(epp_memcpy_d2h_async(vi.data(), base + o_vi, n * 4, d.st));
    need(epp_memcpy_d2h_async(sc.data(), base + o_sc, n * 8, d.st));
    need(epp_memcpy_d2h_async(T.data(), base + o_T, nseg * 8, d.st));
    need(epp_stream_sync(d.st));
    for (size_t k = 0; k < n; ++k)
        if (fit[k] != 0 || st[k] < 0)
            throw std::runtime_error("generateTrajectory: the fit of waypoint set " + std::to_string(k) +
                                     " failed (status " + std::to_string(fit[k] != 0 ? fit[k] : st[k]) + ")");
    for (size_t k = 0; k < n; ++k) {
        double sum = 0.0;  // in order, as Trajectory accumulates the segment times
        for (size_t i = (size_t)off[k] - k; i < (size_t)off[k + 1] - k - 1; ++i) sum += T[i];
        duration[k] = sum;
    }
    scale = sc;
    status.assign(st.begin(), st.end());
    if (violated) violated->assign(vi.begin(), vi.end());
}

// The fit of every set and its snap cost (epp_traj_snap_cost), or the descent over its segment
// times (epp_minsnap_optimize_times) and the result's cost, on one stream, one synchronisation;
// device block: [wp | T | offsets | fit status | cost0 | cost | iters | status | coeffs].
void PathPlanner::candidateSnapCosts(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                     bool optimize, std::vector<double>& costs,
                                     std::vector<std::vector<double>>* times) const {
    const char* what = "candidateSnapCosts";
    for (const auto& s : sets)
        if (s.size() < 2) throw std::invalid_argument("At least two waypoints are required");
    const size_t n = sets.size();
    costs.assign(n, 0.0);
    if (times) times->assign(n, {});
    if (n == 0) return;
    auto need = [what](epp_status rc) {
        if (rc == EPP_ERR_INVALID_ARGUMENT) throw std::invalid_argument(epp_last_error());
        if (rc != EPP_OK) throw std::runtime_error(std::string(what) + ": " + epp_last_error());
    };
    size_t total = 0;
    for (const auto& s : sets) total += s.size();
    const size_t nseg = total - n;
    std::vector<double> wp(total * 3);
    std::vector<int32_t> off(n + 1, 0);
    size_t w = 0;
    for (size_t k = 0; k < n; ++k) {
        for (const Vec3& p : sets[k]) {
            wp[3 * w] = p.x;
            wp[3 * w + 1] = p.y;
            wp[3 * w + 2] = p.z;
            ++w;
        }
        off[k + 1] = (int32_t)w;
    }
    struct Dev {  // released on every way out
        void* buf = nullptr;
        void* st = nullptr;
        ~Dev() {
            if (st) (void)epp_stream_destroy(st);
            if (buf) (void)epp_free(buf);
        }
    } d;
    auto after = [](size_t o, size_t b) { return (o + b + 255) & ~(size_t)255; };  // 256-B aligned parts
    const size_t o_wp = 0, o_T = after(o_wp, total * 24), o_off = after(o_T, nseg * 8),
                 o_fs = after(o_off, (n + 1) * 4), o_j0 = after(o_fs, n * 4), o_j = after(o_j0, n * 8),
                 o_it = after(o_j, n * 8), o_st = after(o_it, n * 4), o_C = after(o_st, n * 4),
                 bytes = after(o_C, nseg * 240);
    need(epp_malloc(&d.buf, bytes));
    need(epp_stream_create(&d.st));
    char* base = static_cast<char*>(d.buf);
    need(epp_memcpy_h2d_async(base + o_wp, wp.data(), total * 24, d.st));
    need(epp_memcpy_h2d_async(base + o_off, off.data(), (n + 1) * 4, d.st));
    const double* d_wp = reinterpret_cast<const double*>(base + o_wp);
    double* d_T = reinterpret_cast<double*>(base + o_T);
    double* d_C = reinterpret_cast<double*>(base + o_C);
    const int32_t* d_off = reinterpret_cast<const int32_t*>(base + o_off);
    int32_t* d_st = reinterpret_cast<int32_t*>(base + o_st);
    need(epp_minsnap_batch(d_wp, d_off, (int32_t)n, v_max, a_max, nullptr, nullptr, d_T, d_C,
                           reinterpret_cast<int32_t*>(base + o_fs), d.st));
    if (optimize) {
        const epp_timeopt_params prm = EPP_TIMEOPT_DEFAULTS;
        need(epp_minsnap_optimize_times(d_wp, d_off, (int32_t)n, nullptr, nullptr, d_T, d_C, prm,
                                        reinterpret_cast<double*>(base + o_j0), reinterpret_cast<double*>(base + o_j),
                                        reinterpret_cast<int32_t*>(base + o_it), d_st, d.st));
    } else {
        need(epp_traj_snap_cost(d_T, d_C, d_off, (int32_t)n, reinterpret_cast<double*>(base + o_j), d_st, d.st));
    }
    std::vector<int32_t> fit(n), st(n);
    std::vector<double> T(nseg);
    need(epp_memcpy_d2h_async(fit.data(), base + o_fs, n * 4, d.st));
    need(epp_memcpy_d2h_async(st.data(), base + o_st, n * 4, d.st));
    need(epp_memcpy_d2h_async(costs.data(), base + o_j, n * 8, d.st));
    need(epp_memcpy_d2h_async(T.data(), base + o_T, nseg * 8, d.st));
    need(epp_stream_sync(d.st));
    for (size_t k = 0; k < n; ++k)
        if (fit[k] != 0 || st[k] < 0)
            throw std::runtime_error("generateTrajectory: the fit of waypoint set " + std::to_string(k) +
                                     " failed (status " + std::to_string(fit[k] != 0 ? fit[k] : st[k]) + ")");
    if (times)
        for (size_t k = 0; k < n; ++k)
            (*times)[k].assign(T.begin() + (off[k] - (long)k), T.begin() + (off[k + 1] - (long)k - 1));
}

void PathPlanner::candidateClearances(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max, double dt,
                                      std::vector<double>& clearance, std::vector<long>* row,
                                      std::vector<double>* time, std::vector<int>* nearest) const {
    std::vector<long> rows;
    const CandidateClear clr{clearance, nearest};
    fit_and_check_candidates("candidateClearances", sets.empty() ? nullptr : worldPtr->device(), sets, v_max, a_max,
                             dt, 0.0, 0, rows, time, nullptr, nullptr, &clr);
    if (row) *row = rows;
}

bool PathPlanner::checkCandidateTrajectories(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                             double dt, double minDistance, std::vector<long>& firstInvalidRow,
                                             std::vector<double>* firstInvalidTime) const {
    fit_and_check_candidates("checkCandidateTrajectories", sets.empty() ? nullptr : worldPtr->device(), sets, v_max,
                             a_max, dt, minDistance, 0, firstInvalidRow, firstInvalidTime, nullptr, nullptr);
    for (long r : firstInvalidRow)
        if (r >= 0) return false;
    return true;
}

bool PathPlanner::sweepCandidateTrajectories(const std::vector<std::vector<Vec3>>& sets, double v_max, double a_max,
                                             double dt, double minDistance, bool canPassGate,
                                             std::vector<long>& firstInvalidRow, std::vector<long>& firstInvalidChord,
                                             std::vector<double>* firstInvalidTime) const {
    std::vector<double> rowTimes, chordTimes;
    fit_and_check_candidates("sweepCandidateTrajectories", sets.empty() ? nullptr : worldPtr->device(), sets, v_max,
                             a_max, dt, minDistance, canPassGate ? 1 : 0, firstInvalidRow, &rowTimes,
                             &firstInvalidChord, &chordTimes);
    bool all = true;
    if (firstInvalidTime) firstInvalidTime->assign(sets.size(), -1.0);
    for (size_t k = 0; k < sets.size(); ++k) {
        const long r = firstInvalidRow[k], c = firstInvalidChord[k];
        all = all && r < 0 && c < 0;
        // the earlier of the two findings (a failing row j and a failing chord j start at the same time)
        if (firstInvalidTime && (r >= 0 || c >= 0))
            (*firstInvalidTime)[k] = (c < 0 || (r >= 0 && r <= c)) ? rowTimes[k] : chordTimes[k];
    }
    return all;
}

}  // namespace epp
