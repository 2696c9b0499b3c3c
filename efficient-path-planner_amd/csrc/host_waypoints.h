// host_waypoints.h — the two small pieces the host calls over waypoint lists share
// (host_trajgen.cpp, host_candidates.cpp, candidate_batch.h): the waypoints as x, y, z doubles
// and the row allocator that lets a single-track call write its rows straight into a Matrix.
// Host code only, no device call.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "epp/types.h"

namespace epp {

// Appends the x, y, z of every waypoint to out.
inline void flatten(const std::vector<Vec3>& waypoints, std::vector<double>& out) {
    out.reserve(out.size() + waypoints.size() * 3);
    for (const Vec3& p : waypoints) {
        out.push_back(p.x);
        out.push_back(p.y);
        out.push_back(p.z);
    }
}

// The alloc callback of generate_trajectory_into / check_and_generate_into over a Matrix (ctx):
// R rows of 10 columns, its storage reused.
inline double* matrix_rows(void* ctx, int64_t R) {
    Matrix& m = *static_cast<Matrix*>(ctx);
    m.rows = (size_t)R;
    m.cols = 10;
    m.data.resize((size_t)std::max<int64_t>(R, 1) * 10);
    return m.data.data();
}

}  // namespace epp
