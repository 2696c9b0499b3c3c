// plan_solve.h — the batched solve of PathPlanner::planChunk (host_plan_solve.cpp): layout
// and scratch, launch and wait, then per problem, on the planner threads, the search.
#pragma once
#include <array>
#include <chrono>
#include <vector>

#include "epp/types.h"
#include "epp_internal.h"
#include "plan_geometry.h"

namespace epp {

struct PlanContext {
    const epp_world* world;
    int k;
    bool canPass;  // validators get can_pass_gate  src/PathPlanner.cpp:47-50
    int threads;   // planner threads (at most one per problem)
    PlanBox box;
};
struct ProblemOut {
    std::vector<Vec3> path;  // the raw path (before the shortcut) when found
    bool found = false;
    int64_t n = 0, edges_checked = 0, edges_valid = 0, rows_down = 0, restricted_rows = 0, pops = 0, nodes = 0;
    int fallback = 0;     // 1: the whole table after the restricted rows could not decide
    int why = -1;         // (PlannerStats::fallback_why)
    int symmetrised = 0;  // the restricted rows decided the symmetrised search
    int census = 0;       // ... after the whole table's k-NN counted the goal's edges
    double ms_dev = 0, ms_search = 0;
    double ms_restricted = 0, ms_copy = 0;  // the restricted search alone (row_of + A*); of which the copy out of pinned memory
};
struct BatchSolution {
    std::vector<ProblemOut> out;          // one per problem
    double ms_batch = 0, ms_enqueue = 0;  // since t0: results in (cold areas warmed), stages queued
};
// segs: seed, ends and geometry filled; kbox[p]: problem p's k-NN box; t0: the attempt's start
BatchSolution solve_batch(const PlanContext& c, std::vector<PlanSeg>& segs, const std::vector<std::array<double, 6>>& kbox,
                          std::chrono::steady_clock::time_point t0);

}  // namespace epp
