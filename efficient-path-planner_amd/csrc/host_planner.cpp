// host_planner.cpp — epp::PathPlanner (drop-in for src/PathPlanner.cpp) on the batch
// GPU planner: the planner's driver.  See include/epp/PathPlanner.h for the algorithm;
// the batched solve is host_plan_solve.cpp, the simplification host_simplify.cpp, the
// trajectory checks host_candidates.cpp.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <utility>

#include "epp/PathPlanner.h"
#include "plan_solve.h"

namespace epp {

namespace {
std::mutex g_stats_mu;

uint64_t mix(uint64_t a, uint64_t b) {
    uint64_t x = a ^ (b + 0x9E3779B97F4A7C15ull + (a << 6) + (a >> 2));
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}
// Adds one launch set's phase times and per-problem counts to the call's statistics.
void add_stats(PlannerStats& st, const BatchSolution& sol, int64_t samples, double ms_solve, double ms_sc) {
    std::lock_guard<std::mutex> lk(g_stats_mu);
    st.ms_device += sol.ms_batch;
    st.ms_search += ms_sc;
    st.ms_batch += sol.ms_batch;
    st.ms_enqueue += sol.ms_enqueue;
    st.ms_solve += ms_solve;
    st.ms_shortcut += ms_sc;
    for (const ProblemOut& o : sol.out) {
        st.states_sampled += samples;
        st.states_valid += o.n - 2;
        st.edges_checked += o.edges_checked;
        st.edges_valid += o.edges_valid;
        st.rows_downloaded += o.rows_down;
        st.restricted_rows += o.restricted_rows;
        st.fallbacks += o.fallback;
        if (o.fallback && o.why >= 0) ++st.fallback_why[o.why];
        st.astar_pops += o.pops;
        st.restricted_symmetrised += o.symmetrised;
        st.symmetrised_after_census += o.census;
        st.restricted_nodes += o.nodes;
        if (o.ms_restricted > st.ms_restricted_max) {
            st.ms_restricted_max = o.ms_restricted;
            st.ms_copy_of_max = o.ms_copy;
        }
        st.ms_device += o.ms_dev;
        st.ms_search += o.ms_search;
    }
}
}  // namespace

PathPlanner::PathPlanner(const Matrix& gates, const Matrix& obstacles, std::shared_ptr<ConfigParser> cp,
                         AbiTag abi)
    : configParser(std::move(cp)) {
    if (abi.planner_size != sizeof(PathPlanner) || abi.stats_size != sizeof(PlannerStats) ||
        abi.version != kPlannerAbiVersion)
        throw std::runtime_error("PathPlanner: caller built against another epp/PathPlanner.h (PathPlanner " +
                                 std::to_string(abi.planner_size) + " B, PlannerStats " +
                                 std::to_string(abi.stats_size) + " B, version " + std::to_string(abi.version) +
                                 "; this library: " + std::to_string(sizeof(PathPlanner)) + " B, " +
                                 std::to_string(sizeof(PlannerStats)) + " B, version " +
                                 std::to_string(kPlannerAbiVersion) + "): rebuild the caller");
    worldPtr = std::make_shared<World>(configParser);
    parseGatesAndObstacles(gates, obstacles);  // src/PathPlanner.cpp:27-35
    // knobs of this build, read once: EPP_PLAN_ELLIPSE the row-restricted search's bound
    // factor (0: the whole table only; else >= 1), EPP_PLAN_THREADS the planner threads
    if (const char* ev = std::getenv("EPP_PLAN_ELLIPSE")) {
        char* end = nullptr;
        const double f = std::strtod(ev, &end);
        if (end != ev && *end == '\0' && (f == 0.0 || f >= 1.0)) ellipse_ = f;
        else std::cerr << "PathPlanner: EPP_PLAN_ELLIPSE=" << ev << " ignored (0, or a factor >= 1)" << std::endl;
    }
    if (const char* tv = std::getenv("EPP_PLAN_THREADS")) {
        const int t = std::atoi(tv);
        if (t >= 1 && t <= 64) threads_ = t;
    }
    // the device world (index build, its HBM and pinned buffers, the upload) now, as the
    // reference builds its World here, not inside the first planPath
    (void)worldPtr->device();
}

// src/PathPlanner.cpp:60-78
void PathPlanner::parseGatesAndObstacles(const Matrix& gates, const Matrix& obstacles) {
    fillWorld(*worldPtr, gates, obstacles);
}

void PathPlanner::fillWorld(World& world, const Matrix& gates, const Matrix& obstacles) {
    world.resetWorld();
    for (size_t i = 0; i < gates.rows; ++i) {
        std::vector<double> g(gates.row(i), gates.row(i) + gates.cols);
        if (g.size() < 7) throw std::invalid_argument("gate rows need 7 columns");
        g[2] = 0.0;  // put all gates to ground  :68
        world.addGate((int)i, g);
    }
    for (size_t i = 0; i < obstacles.rows; ++i) {
        std::vector<double> o(obstacles.row(i), obstacles.row(i) + obstacles.cols);
        if (o.size() < 6) throw std::invalid_argument("obstacle rows need 6 columns");
        world.addObstacle((int)i, o);
    }
}

void PathPlanner::updateGatePos(int gateId, const std::vector<double>& newPose) {
    worldPtr->updateGatePosition(gateId, newPose);  // src/PathPlanner.cpp:170-173
}

// One attempt for a batch of problems (the same sample count; their own seeds), at most 64
// problems per launch set (planChunk).
void PathPlanner::planAttempt(const std::vector<std::pair<Vec3, Vec3>>& problems, const std::vector<uint64_t>& seeds,
                              int64_t samples, std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                              GateEnds* ends) const {
    const size_t np = problems.size();
    paths.assign(np, {});
    ok.assign(np, 0);
    for (size_t b0 = 0; b0 < np; b0 += 64) {
        const size_t b1 = std::min(np, b0 + 64);
        std::vector<std::pair<Vec3, Vec3>> sub(problems.begin() + b0, problems.begin() + b1);
        std::vector<uint64_t> sseeds(seeds.begin() + b0, seeds.begin() + b1);
        std::vector<std::vector<Vec3>> sp;
        std::vector<char> so;
        planChunk(sub, sseeds, samples, sp, so, ends ? ends + b0 : nullptr);
        for (size_t i = b0; i < b1; ++i) {
            paths[i] = std::move(sp[i - b0]);
            ok[i] = so[i - b0];
        }
    }
}

// One launch set: the problems' segments (plan_geometry.h), the batched solve (plan_solve.h:
// layout and scratch, launch and wait, the searches on the planner threads), one batched
// shortcut of the paths found, the statistics.
void PathPlanner::planChunk(const std::vector<std::pair<Vec3, Vec3>>& problems, const std::vector<uint64_t>& seeds,
                            int64_t samples, std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                            GateEnds* ends) const {
    const auto t_dev0 = std::chrono::steady_clock::now();
    const Vec3 lo = configParser->getWorldProperties().lowerBound, hi = configParser->getWorldProperties().upperBound;
    const int S = (int)problems.size();
    PlanContext c{worldPtr->device(), k_, configParser->getPathPlannerProperties().canPassGate, threads_,
                  {{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}, samples + 2, ellipse_, false}};
    // (the rows' motion check needs the world's tile tables: a world without OBBs or past the
    // LDS budget builds every problem's whole table, whose check has the other kernels)
    c.box.restrict_ok = ellipse_ >= 1.0 && (c.k == 4 || c.k == 8 || c.k == 16) && c.box.nmax <= 4 * 65536 &&
                        knn_motions_rows_supported(c.world);
    std::vector<PlanSeg> segs(S);
    std::vector<std::array<double, 6>> kbox(S);  // the whole table's k-NN box (fallback)
    for (int p = 0; p < S; ++p) {
        PlanSeg& q = segs[p];
        q = PlanSeg{};
        q.seed = seeds[p];
        for (int d = 0; d < 3; ++d) {
            q.s[d] = problems[p].first[d];
            q.g[d] = problems[p].second[d];
        }
        plan_geometry(q, kbox[p].data(), c.box);
    }
    BatchSolution sol = solve_batch(c, segs, kbox, t_dev0);
    // ---- one batched shortcut for every path found (reduceVertices' role) ---------------
    const auto t_sc = std::chrono::steady_clock::now();
    const double ms_solve = std::chrono::duration<double, std::milli>(t_sc - t_dev0).count() - sol.ms_batch;
    std::vector<std::vector<Vec3>> shortcut_in;
    std::vector<int> which;
    std::vector<GateEnds*> sc_ends;  // (planPathsIncludeGates2: the pruning's pairs too)
    for (int p = 0; p < S; ++p)
        if (sol.out[p].found) {
            shortcut_in.push_back(std::move(sol.out[p].path));
            which.push_back(p);
            if (ends) sc_ends.push_back(ends + p);
        }
    std::vector<std::vector<Vec3>> shortcut_out = shortcutAll(shortcut_in, ends ? &sc_ends : nullptr);
    paths.assign(S, {});
    ok.assign(S, 0);
    for (size_t i = 0; i < which.size(); ++i) {
        paths[which[i]] = std::move(shortcut_out[i]);
        ok[which[i]] = 1;
    }
    const double ms_sc = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sc).count();
    add_stats(stats_, sol, samples, ms_solve, ms_sc);
}

bool PathPlanner::planOnce(const Vec3& start, const Vec3& goal, int64_t samples, uint64_t seed,
                           std::vector<Vec3>& out) const {
    std::vector<std::vector<Vec3>> paths;
    std::vector<char> ok;
    planAttempt({{start, goal}}, {seed}, samples, paths, ok);
    if (ok[0]) out = std::move(paths[0]);
    return ok[0] != 0;
}

// The planner choice of src/PathPlanner.cpp:106-123.  "rrt" cannot be honoured (OMPL's
// RRT* is third-party and not part of this build; its `range` has no counterpart): it
// runs the same batch planner as "fmt", and says so once per process.  The reference
// itself never reads optimality_threshold_percentage (getStraightLineObjective,
// src/PathPlanner.cpp:160-168, is never called), so neither does this build.
static void checkPlannerConfig(const PathPlannerProperties& pp) {
    if (pp.planner != "rrt" && pp.planner != "fmt") {
        std::cerr << "Unknown planner" << std::endl;
        throw std::runtime_error("Unknown planner");  // :121-123
    }
    if (pp.planner == "rrt") {
        static std::once_flag once;
        std::call_once(once, [] {
            std::cerr << "PathPlanner: planner \"rrt\" runs the batch sampling planner of this build (OMPL's RRT* "
                         "is not available); path_planner_properties.range is not used"
                      << std::endl;
        });
    }
}

// PathPlanner::planPath — src/PathPlanner.cpp:80-158
bool PathPlanner::planPath(const Vec3& start, const Vec3& goal, double timeLimit, std::vector<Vec3>& resultPath) const {
    if (!resultPath.empty()) {
        resultPath.clear();
        std::cerr << "Result path not empty, clearing it" << std::endl;
    }
    std::vector<std::vector<Vec3>> paths;
    std::vector<char> ok;
    planPathsWith({{start, goal}}, timeLimit, paths, ok, nullptr);  // (one problem: the next call number)
    if (ok[0]) resultPath = std::move(paths[0]);
    return ok[0] != 0;
}

// Problems with the call numbers base, base + 1, ...: attempt a with samples_fmt x 2^a
// samples and the seed mix(seed(call), a), the problems still without a path batched
// together; up to 4 attempts while inside timeLimit (the role of solve(timeLimit),
// src/PathPlanner.cpp:126-136).  Returns the attempts made.
int PathPlanner::planCalls(const std::vector<std::pair<Vec3, Vec3>>& problems, uint64_t base, double timeLimit,
                           std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                           std::vector<GateEnds>* ends) const {
    const auto t0 = std::chrono::steady_clock::now();
    const auto& pp = configParser->getPathPlannerProperties();
    const size_t n = problems.size();
    paths.assign(n, {});
    ok.assign(n, 0);
    std::vector<uint64_t> seeds(n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t seed = mix(seed_, base + i);
        for (int d = 0; d < 3; ++d) seed = mix(mix(seed, bits_of(problems[i].first[d])), bits_of(problems[i].second[d]));
        seeds[i] = seed;
    }
    std::vector<size_t> pending(n);
    for (size_t i = 0; i < n; ++i) pending[i] = i;
    int64_t samples = pp.samplesFMT > 0 ? pp.samplesFMT : 4096;
    int attempts = 0;
    for (int a = 0; a < 4 && !pending.empty(); ++a) {
        std::vector<std::pair<Vec3, Vec3>> sub;
        std::vector<uint64_t> sseeds;
        for (size_t i : pending) {
            sub.push_back(problems[i]);
            sseeds.push_back(mix(seeds[i], (uint64_t)a));
        }
        std::vector<std::vector<Vec3>> sp;
        std::vector<char> so;
        std::vector<GateEnds> se;
        if (ends)
            for (size_t i : pending) se.push_back((*ends)[i]);
        planAttempt(sub, sseeds, samples, sp, so, ends ? se.data() : nullptr);
        attempts = a + 1;
        std::vector<size_t> still;
        for (size_t j = 0; j < pending.size(); ++j) {
            if (so[j]) {
                paths[pending[j]] = std::move(sp[j]);
                ok[pending[j]] = 1;
                if (ends) (*ends)[pending[j]] = std::move(se[j]);
            } else {
                still.push_back(pending[j]);
            }
        }
        pending.swap(still);
        // (every pending problem ran in each attempt, concurrently with the others, so the
        // batch's elapsed time is each problem's own, as for concurrent planPath calls
        // (src/OnlineTrajGenerator.cpp:324-340); consecutive planPath calls -- the
        // reference's preComputeTraj -- would each restart the clock: a problem that keeps
        // failing here gets at most the attempts timeLimit allows from the batch's start)
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (!pending.empty() && el > timeLimit) break;  // out of time: give up like solve(timeLimit)
        samples *= 2;
    }
    return attempts;
}

void PathPlanner::planPaths(const std::vector<std::pair<Vec3, Vec3>>& problems, double timeLimit,
                            std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok) const {
    planPathsWith(problems, timeLimit, paths, ok, nullptr);
}

bool PathPlanner::planPathsIncludeGates2(const std::vector<std::pair<Vec3, Vec3>>& problems, double timeLimit,
                                         std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                                         std::vector<Vec3>& pruned) const {
    // (EPP_FUSED_PRUNE=0: the two calls as they are, for A/B)
    static const bool fused = [] {
        const char* e = std::getenv("EPP_FUSED_PRUNE");
        return !(e && std::string(e) == "0");
    }();
    std::vector<GateEnds> ends;
    if (fused && configParser->getPathPlannerProperties().pathSimplification == "custom") {
        ends.resize(problems.size());
        for (size_t s = 0; s + 1 < problems.size(); ++s) {  // includeGates2's (a + b) / 2 of the ends
            const Vec3 c = (problems[s].second + problems[s + 1].first) / 2;
            ends[s].has_next = ends[s + 1].has_prev = true;
            ends[s].next = ends[s + 1].prev = c;
        }
    }
    planPathsWith(problems, timeLimit, paths, ok, ends.empty() ? nullptr : &ends);
    for (char o : ok)
        if (!o) return false;
    pruned = includeGates2With(paths, ends.empty() ? nullptr : &ends);
    return true;
}

void PathPlanner::planPathsWith(const std::vector<std::pair<Vec3, Vec3>>& problems, double timeLimit,
                                std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                                std::vector<GateEnds>* ends) const {
    checkPlannerConfig(configParser->getPathPlannerProperties());
    const size_t n = problems.size();
    paths.assign(n, {});
    ok.assign(n, 0);
    if (n == 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> lk(g_stats_mu);
        stats_ = PlannerStats();
    }
    (void)worldPtr->device();  // the device world, before the planner threads share it
    const uint64_t base = __atomic_fetch_add(&calls_, (uint64_t)n, __ATOMIC_RELAXED);
    const int attempts = planCalls(problems, base, timeLimit, paths, ok, ends);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    stats_.attempts = attempts;
    stats_.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace epp
