// epp/PathPlanner.h — drop-in for the reference's PathPlanner (include/PathPlanner.h:30-80,
// src/PathPlanner.cpp).  OMPL is replaced by a batch planner on the GPU:
//
//   planPath:  sample `samples_fmt` states in the world bounds (counter RNG), check them
//              (StateValidator semantics), connect every node to its k = 16 nearest
//              neighbours, check all edges at once (MotionValidator semantics), search the
//              shortest valid path on the host, then shortcut it greedily with one batched
//              motion check of all vertex pairs (the role of reduceVertices).
//   includeGates2 / pruneWaypoints / checkTrajectoryValidity: the reference's host logic,
//              with every validity query batched into one GPU launch.
//
// Unlike RRT* with no cost threshold (which always runs to timeLimit), planPath returns
// as soon as the batch search is done; timeLimit only bounds the retries with more
// samples when no path is found.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "epp/ConfigParser.h"
#include "epp/World.h"
#include "epp/types.h"

namespace epp {

// Layout version of PlannerStats / PathPlanner below: raise it whenever either changes.
constexpr uint32_t kPlannerAbiVersion = 6;

struct PlannerStats {
    // ABI guard (first, so a caller built against any version reads it): the size of the
    // struct the library filled in; a caller checks lastStats().size == sizeof(PlannerStats)
    uint32_t size = sizeof(PlannerStats);
    uint32_t version = kPlannerAbiVersion;
    int64_t states_sampled = 0;
    int64_t states_valid = 0;
    int64_t edges_checked = 0;    // edges of the graphs searched (the final table's on a fallback)
    int64_t edges_valid = 0;
    int attempts = 0;
    int64_t rows_downloaded = 0;  // k-NN table rows copied to the host (see planPath)
    int64_t restricted_rows = 0;  // of which packed rows of the row-restricted searches
    int64_t fallbacks = 0;        // searches that took the whole table after the restricted rows
    // why (diagnostics): [0] rows past the capacity or > 65,535 nodes, [1] an inexact row,
    // [2] no kept edge into the goal among the rows but one elsewhere in the whole table,
    // [3] a pop above the bound,
    // [4] (forward exhausted: the symmetrised search follows), [5] symmetrised: a pop above
    // the bound, [6] symmetrised: exhausted in the rows
    int64_t fallback_why[7] = {0, 0, 0, 0, 0, 0, 0};
    int64_t restricted_symmetrised = 0;  // searches the rows' symmetrised graph decided
    // of which: after the whole table's k-NN (run for its goal-edge count only: the forward
    // search popped above the bound with no kept edge into the goal among the rows)
    int64_t symmetrised_after_census = 0;
    int64_t astar_pops = 0, restricted_nodes = 0;  // (diagnostics) the restricted searches' closed nodes / node lists
    double ms_restricted_max = 0;                  // (diagnostics) the slowest problem's restricted search
    double ms_copy_of_max = 0;                     // (diagnostics) of which its copy out of pinned memory
    double ms = 0;         // wall time of the last planPath
    double ms_device = 0;  // of which: sampling, checks, k-NN, transfers (GPU phases)
    double ms_search = 0;  // of which: graph build + A* + shortcut on the host
    // wall time of the batched planner's phases (summed over its attempts): the device
    // stages up to the emitted results, the searches on the planner threads, the shortcut
    double ms_batch = 0, ms_solve = 0, ms_shortcut = 0;
    double ms_enqueue = 0;  // of ms_batch: the host until every stage of the batch was queued
};

class PathPlanner {
public:
    // The caller's view of the layout (sizes and version compiled into the CALLER from this
    // header) is handed to the library, which throws std::runtime_error when it differs from
    // its own: a caller built against a stale header (PlannerStats grew, cd38a05) fails at
    // construction instead of reading or writing past the object.
    struct AbiTag {
        uint32_t planner_size, stats_size, version;
    };
    PathPlanner(const Matrix& nominalGatePositionAndType, const Matrix& nominalObstaclePosition,
                std::shared_ptr<ConfigParser> configParser)
        : PathPlanner(nominalGatePositionAndType, nominalObstaclePosition, std::move(configParser),
                      AbiTag{sizeof(PathPlanner), sizeof(PlannerStats), kPlannerAbiVersion}) {}
    PathPlanner(const Matrix& nominalGatePositionAndType, const Matrix& nominalObstaclePosition,
                std::shared_ptr<ConfigParser> configParser, AbiTag callerAbi);

    void parseGatesAndObstacles(const Matrix& nominalGatePositionAndType, const Matrix& nominalObstaclePosition);
    // The world build of parseGatesAndObstacles into any World (src/PathPlanner.cpp:60-78):
    // reset, gates with z := 0, obstacles.
    static void fillWorld(World& world, const Matrix& nominalGatePositionAndType, const Matrix& nominalObstaclePosition);
    // checkTrajectoryValidity against any World (one batched launch)
    static bool checkTrajectoryValidityOn(const World& world, const Matrix& trajectory, double minDistance);
    bool planPath(const Vec3& start, const Vec3& goal, double timeLimit, std::vector<Vec3>& resultPath) const;
    // Independent (start, goal) problems planned together: every device stage runs once
    // for all of them (one launch each, blockIdx.y = the problem), the searches run on
    // planner threads, the shortcut checks are one batch.  Problem i gets the seed of the
    // i-th of consecutive planPath calls, so results do not depend on the batching or on
    // thread timing.  ok[i] / paths[i] as planPath's return value / resultPath; stats =
    // the sum, ms = the batch's wall time.
    void planPaths(const std::vector<std::pair<Vec3, Vec3>>& problems, double timeLimit,
                   std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok) const;
    void updateGatePos(int gateId, const std::vector<double>& newPose);
    bool checkTrajectoryValidity(const Matrix& trajectory, double minDistance) const;
    // The C5 online step in one GPU launch (an addition of this build): returns
    // checkTrajectoryValidity(trajectory, minDistance) and sets `result` to
    // poly_traj::generateTrajectory(waypoints, vMax, aMax, samplingInterval,
    // startTimeOffset, v0, a0) -- the two are independent, so the check runs on extra
    // workgroups of the refit's kernel (epp_check_and_generate_trajectory_host).  Same
    // answers as the two calls; a check too large for the small path makes the two calls.
    bool checkTrajectoryValidityAndGenerate(const Matrix& trajectory, double minDistance,
                                            const std::vector<Vec3>& waypoints, double vMax, double aMax,
                                            double samplingInterval, double startTimeOffset, const Vec3& v0,
                                            const Vec3& a0, Matrix& result) const;
    // Which of K candidate waypoint sets give a collision-free trajectory, and where the
    // others first collide (an addition of this build): poly_traj::generateTrajectory's fit of
    // every set (epp_minsnap_batch) and checkTrajectoryValidity of each fit's rows at
    // samplingInterval (epp_traj_check_batch: no row is written) on one stream against the
    // planner's world; the call itself synchronises once, at the end (epp_minsnap_batch reads
    // the track offsets back to size its launch: a second, short host wait inside it).  firstInvalidRow[k]: the index of set
    // k's first row closer than minDistance to an obstacle, -1 if none; firstInvalidTime
    // (optional): that row's time, -1.0 if none.  Returns true iff every set is valid.
    // Throws std::invalid_argument("At least two waypoints are required") for a set with
    // fewer, std::runtime_error for a failed fit, as generateTrajectory.
    bool checkCandidateTrajectories(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max,
                                    double dt, double minDistance, std::vector<long>& firstInvalidRow,
                                    std::vector<double>* firstInvalidTime = nullptr) const;
    // checkCandidateTrajectories plus the swept check of the same fits (an addition of this
    // build): the rows only say where a track is every dt, so a track faster than a bar is
    // thick can step over it; the straight chords between consecutive rows are therefore
    // tested too, with World::checkRayValid(p_j, p_j+1, canPassGate) (epp_traj_sweep_batch),
    // on the same fitted batch and stream, synchronising once.  firstInvalidRow[k]: as
    // checkCandidateTrajectories; firstInvalidChord[k]: the smallest j whose chord row j ->
    // row j + 1 fails, -1 if none; firstInvalidTime (optional): the time of the earlier of the
    // two findings (row j and chord j both start at row j's time), -1.0 if neither.  Returns
    // true iff no row and no chord of any set fails.  Throws as checkCandidateTrajectories.
    bool sweepCandidateTrajectories(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max,
                                    double dt, double minDistance, bool canPassGate,
                                    std::vector<long>& firstInvalidRow, std::vector<long>& firstInvalidChord,
                                    std::vector<double>* firstInvalidTime = nullptr) const;
    // How close each of K candidate waypoint sets' trajectories comes to an obstacle (an
    // addition of this build), to rank valid candidates: the fit of every set as above and, on
    // the same stream with one synchronisation, epp_traj_clearance_batch (include/epp.h) of
    // the fits' rows at dt.  clearance[k]: the smallest Euclidean distance from a row of set k
    // to a collision (non-filling) OBB, 0 for a row inside one, +inf for a world without any;
    // row / time / nearest (optional): the earliest row that attains it, its time, and the
    // nearest OBB's index in the world's order (the lowest among equals); -1, -1.0, -1 when
    // the clearance is +inf.  Throws as checkCandidateTrajectories.
    void candidateClearances(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max, double dt,
                             std::vector<double>& clearance, std::vector<long>* row = nullptr,
                             std::vector<double>* time = nullptr, std::vector<int>* nearest = nullptr) const;
    // candidateClearances of the chords instead of the rows (an addition of this build): a
    // track that passes a bar between two rows keeps the margin of neither row.  The fit of
    // every set as above and, on the same stream with one synchronisation,
    // epp_traj_chord_clearance_batch (include/epp.h) of the straight chords between the fits'
    // consecutive rows at dt.  clearance[k]: the smallest Euclidean distance between a chord
    // of set k and a collision (non-filling) OBB, 0 for a chord that touches or enters one,
    // +inf for a world without any (never more than candidateClearances' for a track of two
    // rows or more); chord / t / time / nearest (optional): the earliest chord row j -> row
    // j + 1 that attains it, the parameter in [0, 1] along it, the track time of that point
    // and the nearest OBB's index in the world's order (the lowest among equals); -1, -1.0,
    // -1.0, -1 when the clearance is +inf.  Throws as checkCandidateTrajectories.
    void candidateSweptClearances(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max,
                                  double dt, std::vector<double>& clearance, std::vector<long>* chord = nullptr,
                                  std::vector<double>* t = nullptr, std::vector<double>* time = nullptr,
                                  std::vector<int>* nearest = nullptr) const;
    // How much room a waypoint polyline (planPath's result, a shortcut path, includeGates2's)
    // leaves (an addition of this build): the smallest Euclidean distance between one of its
    // edges path[j] -> path[j + 1] and a collision (non-filling) OBB, in one
    // World::edgeClearances call over the edges; edge / t / nearest (optional): the earliest
    // edge that attains it, the parameter in [0, 1] along it and the OBB's index in the world's
    // order; +inf, -1, -1.0, -1 without a collision OBB.  Throws std::invalid_argument for a
    // path of fewer than two points.
    double pathClearance(const std::vector<Vec3>& path, long* edge = nullptr, double* t = nullptr,
                         int* nearest = nullptr) const;
    // Where and against what each of K candidate waypoint sets' trajectories first fails the
    // swept check (an addition of this build): the fit of every set as above and, on the same
    // stream with one synchronisation, epp_traj_first_hit_batch (include/epp.h) of the fits'
    // chords at dt.  chord[k]: sweepCandidateTrajectories' firstInvalidChord; t[k]: the
    // parameter in [0, 1] along that chord at which it enters the blocking OBB (0: its start
    // row is in collision); time / obb (optional): the track time of that point and the OBB's
    // index in the world's order (the lowest among equals).  -1, +inf, -1.0, -1 for a set
    // without a failing chord.  Throws as checkCandidateTrajectories.
    void candidateFirstHits(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max, double dt,
                            bool canPassGate, std::vector<long>& chord, std::vector<double>& t,
                            std::vector<double>* time = nullptr, std::vector<int>* obb = nullptr) const;
    // The gate frame table of epp_gates_crossed / epp_traj_gate_pass_batch (include/epp.h) for
    // G gate rows [x, y, z, rx, ry, yaw, type] (an addition of this build): G x 5 rows
    // [cx, cy, cz, cos(yaw), sin(yaw)], the centre being the position plus (0, 0, height) of the
    // gate's type in this planner's config (getGateCenterAndNormal,
    // src/OnlineTrajGenerator.cpp:50-70), cos / sin from std::cos / std::sin.  Throws
    // std::invalid_argument for a row with a rotation about x or y, which
    // getGateCenterAndNormal rejects, and for rows of fewer than 7 columns.
    Matrix gateFrames(const Matrix& gates) const;
    // Which gates, in order, each of K candidate waypoint sets' trajectories passes, and when
    // (an addition of this build), to rank candidates after validity: the fit of every set as
    // above and, on the same stream with one synchronisation, epp_traj_gate_pass_batch
    // (include/epp.h) of the fits' chords at dt against `frames` (gateFrames' table, G <= 64
    // rows) with the opening's half edge `halfEdge` (the reference's constant: 0.425).  Row-major
    // K x G: chord[k * G + g] the chord row j -> row j + 1 of set k that passes gate g after
    // the gates before it, -1 if unpassed; time its split time, -1.0 if unpassed; offsets
    // (optional, K x G x 2) the crossing's midpoint offsets in the gate frame (x, z), NaN if
    // unpassed.  nPassed[k]: the leading gates set k passes.  Throws as
    // checkCandidateTrajectories.
    void candidateGatePasses(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max, double dt,
                             const Matrix& frames, double halfEdge, std::vector<long>& chord,
                             std::vector<double>& time, std::vector<int>& nPassed,
                             std::vector<double>* offsets = nullptr) const;
    // What a quadrotor must do to fly each of K candidate waypoint sets' trajectories (an
    // addition of this build), to rank candidates after validity: the fit of every set as
    // above and, on the same stream with one synchronisation, epp_traj_thrust_rates_batch
    // (include/epp.h) of the fits' rows at dt under the gravity g.  Row-major K x 8:
    // out[k * 8 + ..] = [f_min, t_fmin, f_max, t_fmax, rate_max, t_rate, cos_min, t_cos]: the
    // extremes over set k's rows of the mass-normalised thrust |a + g e_z|, the roll / pitch
    // body rate |F x j| / |F|^2 and the cosine of the tilt, each with its row's time; rows
    // (optional, K x 4): the earliest rows that attain them, -1 for a quantity that is NaN on
    // every row (its value then +inf for a minimum, -inf for a maximum).  Throws as
    // checkCandidateTrajectories.
    void candidateThrustRates(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max, double dt,
                              double g, std::vector<double>& out, std::vector<long>* rows = nullptr) const;
    // The duration at which each of K candidate waypoint sets' trajectories becomes flyable (an
    // addition of this build), to rank candidates: the fit of every set as above and, on the
    // same stream with one synchronisation, epp_traj_scale_to_thrust_limits (include/epp.h)
    // under `limits`.  scale[k]: the factor applied to set k's segment times (1.0: flyable as
    // fitted); duration[k]: the sum of the scaled segment times; status[k]: 0, or 1 when the
    // set is still infeasible at scale 1024 (duration then that of the fit); violated
    // (optional): the limits violated as fitted, bit 0 f_min, bit 1 f_max, bit 2 rate, bit 3
    // tilt.  The search looks at 65 points per segment, and only f_max is monotone in the
    // scale: the answer is a feasible scale, not a proven minimum.  Throws as
    // candidateThrustRates, and std::invalid_argument for limits outside 0 <= fMin < g < fMax,
    // rateMax > 0, cosTiltMin < 1.
    struct FlightLimits {
        double g, fMin, fMax, rateMax, cosTiltMin;
    };
    void candidateFlyableScales(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max,
                                const FlightLimits& limits, std::vector<double>& scale, std::vector<double>& duration,
                                std::vector<int>& status, std::vector<int>* violated = nullptr) const;
    // The snap cost of each of K candidate waypoint sets' trajectories (an addition of this
    // build), to rank candidates by smoothness: the fit of every set as above and, on the same
    // stream with one synchronisation, epp_traj_snap_cost (include/epp.h) of the fit; with
    // `optimize`, epp_minsnap_optimize_times (default parameters) from the fit's Nfabian times
    // first, and the cost of its result.  costs[k]: PolynomialOptimization::computeCost, the
    // integral of the squared snap; times (optional): the K sets' segment times, the optimised
    // ones with `optimize` (their sums are the fits').  Throws as candidateThrustRates.
    void candidateSnapCosts(const std::vector<std::vector<Vec3>>& waypointSets, double v_max, double a_max,
                            bool optimize, std::vector<double>& costs,
                            std::vector<std::vector<double>>* times = nullptr) const;
    std::vector<Vec3> includeGates2(std::vector<std::vector<Vec3>> waypoints) const;
    // planPaths of consecutive gate-to-gate segments, then includeGates2 of their paths (an
    // addition of this build, for OnlineTrajGenerator::preComputeTraj): the same answers as
    // the two calls.  The gate centres includeGates2 inserts are the midpoints of the
    // segments' ends, known before the plans, so with the "custom" pruning every ray the
    // pruning can ask rides in the shortcut's batch (each ray tested once for both
    // canPassGate answers): one synchronised launch fewer.  Returns false, `pruned`
    // untouched, when some ok[i] is 0.
    bool planPathsIncludeGates2(const std::vector<std::pair<Vec3, Vec3>>& problems, double timeLimit,
                                std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                                std::vector<Vec3>& pruned) const;

    // batch-planner knobs (defaults follow the config: samples_fmt samples, k = 16)
    void setSeed(uint64_t seed) { seed_ = seed; }
    void setNeighbours(int k) { k_ = k; }
    const PlannerStats& lastStats() const { return stats_; }
    // One batch-planner attempt with an explicit sample count and RNG seed (planPath makes
    // up to 4 of them); public for the CPU restatement's path-equality tests and baselines.
    bool planOnce(const Vec3& start, const Vec3& goal, int64_t samples, uint64_t seed,
                  std::vector<Vec3>& out) const;

    std::shared_ptr<World> worldPtr;

private:
    // A problem of a chain of gate-to-gate segments (planPathsIncludeGates2): the gate
    // centres includeGates2 will put before / after its path and, once the shortcut's batch
    // has run, the canPassGate = true answers of every pair the pruning can ask.
    struct GateEnds {
        bool has_prev = false, has_next = false;
        Vec3 prev, next;
        bool filled = false;       // pts / vis hold the answers
        std::vector<Vec3> pts;     // [prev] + the shortcut's input path + [next]
        std::vector<uint8_t> vis;  // pair (i, j) of pts, j >= i + 2, in the shortcut's queue order
    };
    std::vector<Vec3> pruneWaypoints(const std::vector<Vec3>& waypoints) const;
    std::vector<Vec3> shortcut(const std::vector<Vec3>& path) const;
    std::vector<std::vector<Vec3>> shortcutAll(const std::vector<std::vector<Vec3>>& paths,
                                               const std::vector<GateEnds*>* ends = nullptr) const;
    std::vector<std::vector<Vec3>> pruneAll(const std::vector<std::vector<Vec3>>& segments,
                                            const std::vector<GateEnds>* ends = nullptr) const;
    std::vector<Vec3> includeGates2With(std::vector<std::vector<Vec3>> waypoints,
                                        const std::vector<GateEnds>* ends) const;
    void planPathsWith(const std::vector<std::pair<Vec3, Vec3>>& problems, double timeLimit,
                       std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                       std::vector<GateEnds>* ends) const;
    // omplPrunePathAndInterpolate (src/PathPlanner.cpp:282-313) for every segment at once:
    // OMPL's PathSimplifier::smoothBSpline with its defaults, each step's state and motion
    // checks for all segments in one batch each
    std::vector<std::vector<Vec3>> smoothAll(const std::vector<std::vector<Vec3>>& segments) const;
    // ends (optional): one per problem, filled for the problems whose path is found
    int planCalls(const std::vector<std::pair<Vec3, Vec3>>& problems, uint64_t base, double timeLimit,
                  std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                  std::vector<GateEnds>* ends = nullptr) const;
    void planAttempt(const std::vector<std::pair<Vec3, Vec3>>& problems, const std::vector<uint64_t>& seeds,
                     int64_t samples, std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                     GateEnds* ends = nullptr) const;
    void planChunk(const std::vector<std::pair<Vec3, Vec3>>& problems, const std::vector<uint64_t>& seeds,
                   int64_t samples, std::vector<std::vector<Vec3>>& paths, std::vector<char>& ok,
                   GateEnds* ends = nullptr) const;

    std::shared_ptr<ConfigParser> configParser;
    uint64_t seed_ = 0x5eedull;
    int k_ = 16;
    double ellipse_ = 1.25;  // row-restricted search: bound = ellipse_ |start - goal| + 0.25 m (0: off)
    int threads_ = 16;      // planner threads of a batch's searches (at most one per problem)
    mutable uint64_t calls_ = 0;
    mutable PlannerStats stats_;
};

}  // namespace epp
