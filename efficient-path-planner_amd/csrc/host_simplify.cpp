// host_simplify.cpp — epp::PathPlanner's path simplification: the shortcut of planned paths
// (reduceVertices' role), includeGates2 and its prunings, every validity query of a step
// batched into one GPU launch.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <utility>

#include "epp/PathPlanner.h"

namespace epp {

namespace {
// EPP_PAIRS_TRACE=1 (diagnostics): the shortcut's and the pruning's batched ray checks --
// pairs and wall time of each batch -- to stderr
bool pairs_trace() {
    static const bool t = [] {
        const char* e = std::getenv("EPP_PAIRS_TRACE");
        return e && std::atoi(e) == 1;
    }();
    return t;
}

// Queues the pairs (i, j), j >= i + 2, of the point list w row by row as rays s1 -> s2;
// returns their number.
size_t queue_pairs(const std::vector<Vec3>& w, std::vector<double>& s1, std::vector<double>& s2) {
    const size_t L = w.size(), before = s1.size();
    for (size_t i = 0; i < L; ++i)
        for (size_t j = i + 2; j < L; ++j) {
            s1.insert(s1.end(), {w[i].x, w[i].y, w[i].z});
            s2.insert(s2.end(), {w[j].x, w[j].y, w[j].z});
        }
    return (s1.size() - before) / 3;
}
// The index of pair (i, j) among those queue_pairs queued for an L-point list.
size_t pair_index(size_t L, size_t i, size_t j) {
    const size_t before = i * (L - 2) - (i * (i - 1)) / 2;  // pairs of rows < i: sum (L - 2 - r)
    return before + (j - i - 2);
}
double us_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t).count();
}
}  // namespace

// Greedy shortcutting with one batched check of every vertex pair of every path (the role
// of PathSimplifier::reduceVertices in src/PathPlanner.cpp:138-139).
std::vector<std::vector<Vec3>> PathPlanner::shortcutAll(const std::vector<std::vector<Vec3>>& ps,
                                                        const std::vector<GateEnds*>* ends) const {
    // ends: each path's list is [prev] + path + [next] (the pruning's points): all its pairs
    // are queued and each ray answers both canPassGate values (World::checkRaysBoth); the
    // shortcut reads the path's pairs, the pruning keeps the true answers of all of them
    const bool canPass = configParser->getPathPlannerProperties().canPassGate;
    std::vector<double> s1, s2;
    std::vector<size_t> base(ps.size() + 1, 0), off(ps.size(), 0);
    for (size_t q = 0; q < ps.size(); ++q) {
        const auto& p = ps[q];
        std::vector<Vec3> ext;
        if (ends) {
            GateEnds& g = *(*ends)[q];
            if (g.has_prev) ext.push_back(g.prev);
            off[q] = g.has_prev ? 1 : 0;
            ext.insert(ext.end(), p.begin(), p.end());
            if (g.has_next) ext.push_back(g.next);
        }
        base[q + 1] = base[q] + queue_pairs(ends ? ext : p, s1, s2);
        if (ends) (*ends)[q]->pts = std::move(ext);
    }
    std::vector<uint8_t> ok(base.back());
    const auto t_rays = std::chrono::steady_clock::now();
    if (!ok.empty()) {
        if (ends) worldPtr->checkRaysBoth(s1.data(), s2.data(), (int64_t)ok.size(), ok.data());
        else worldPtr->checkRays(s1.data(), s2.data(), (int64_t)ok.size(), canPass, ok.data());
    }
    if (pairs_trace())
        std::fprintf(stderr, "pairs_trace: shortcut paths %zu pairs %zu rays%s %.1f us\n", ps.size(), ok.size(),
                     ends ? " (both answers: the pruning's too)" : "", us_since(t_rays));
    const uint8_t bit = ends ? (canPass ? 2 : 1) : 0xFF;  // the shortcut's answer in a flag byte
    if (ends)
        for (size_t q = 0; q < ps.size(); ++q) {
            GateEnds& g = *(*ends)[q];
            g.vis.resize(base[q + 1] - base[q]);
            for (size_t t = 0; t < g.vis.size(); ++t) g.vis[t] = (ok[base[q] + t] >> 1) & 1;
            g.filled = true;
        }
    std::vector<std::vector<Vec3>> out(ps.size());
    for (size_t q = 0; q < ps.size(); ++q) {
        const auto& p = ps[q];
        const size_t L = p.size();
        if (L < 3) {
            out[q] = p;
            continue;
        }
        // vis(i, j) of pair (i, j), j >= i + 2, in the order they were queued
        const size_t LE = ends ? (*ends)[q]->pts.size() : L;
        auto vis = [&](size_t i, size_t j) {
            return (ok[base[q] + pair_index(LE, i + off[q], j + off[q])] & bit) != 0;
        };
        std::vector<Vec3> o = {p[0]};
        size_t cur = 0;
        while (cur + 1 < L) {
            size_t nxt = cur + 1;  // a path edge, valid by construction
            for (size_t j = L - 1; j > cur + 1; --j)
                if (vis(cur, j)) {
                    nxt = j;
                    break;
                }
            o.push_back(p[nxt]);
            cur = nxt;
        }
        out[q] = std::move(o);
    }
    return out;
}

std::vector<Vec3> PathPlanner::shortcut(const std::vector<Vec3>& p) const { return shortcutAll({p})[0]; }

// PathPlanner::includeGates2 — src/PathPlanner.cpp:175-230.  The segments' pruning checks
// are one batch (pruneAll).
std::vector<Vec3> PathPlanner::includeGates2(std::vector<std::vector<Vec3>> waypoints) const {
    return includeGates2With(std::move(waypoints), nullptr);
}

std::vector<Vec3> PathPlanner::includeGates2With(std::vector<std::vector<Vec3>> waypoints,
                                                 const std::vector<GateEnds>* ends) const {
    std::vector<Vec3> gateCenters;
    for (size_t s = 0; s + 1 < waypoints.size(); ++s) {
        const Vec3& a = waypoints[s].back();
        const Vec3& b = waypoints[s + 1].front();
        gateCenters.push_back((a + b) / 2);
    }
    for (size_t i = 0; i < gateCenters.size(); ++i) {
        waypoints[i].push_back(gateCenters[i]);
        waypoints[i + 1].insert(waypoints[i + 1].begin(), gateCenters[i]);
    }
    const std::string method = configParser->getPathPlannerProperties().pathSimplification;
    std::vector<std::vector<Vec3>> pruned;
    if (method == "none") {
        pruned = waypoints;
    } else if (method == "custom") {
        pruned = pruneAll(waypoints, ends);
    } else if (method == "ompl") {
        pruned = smoothAll(waypoints);
    } else {
        std::cerr << "Unknown pruning method" << std::endl;
        throw std::runtime_error("Unknown pruning method");
    }
    std::vector<Vec3> flat;
    for (const auto& seg : pruned)
        for (const auto& w : seg) {
            if (!flat.empty() && (flat.back() - w).norm() < 0.05) continue;  // :222
            flat.push_back(w);
        }
    return flat;
}

// PathPlanner::omplPrunePathAndInterpolate — src/PathPlanner.cpp:282-313: OMPL's
// PathSimplifier::smoothBSpline(path) with its defaults (maxSteps = 5, minChange = double
// epsilon), as OMPL 1.6 publishes it (PathSimplifier.cpp, PathGeometric::subdivide,
// RealVectorStateSpace::interpolate / distance).  Per step every live path is subdivided
// (a midpoint between every two states); then each even state i (2 <= i < n - 1) moves to
// the midpoint of the midpoints (i-1, i) and (i, i+1) when state i-1 is valid, both
// motions (i-1 -> new, new -> i+1) are valid and the move exceeds minChange.  The moves of
// one step touch only even states and read only odd ones, so they are independent: the
// step's state checks (all paths) are one batch, its motion checks another, on the
// planner's validators (src/PathPlanner.cpp:47-50: can_pass_gate from the config).  A path
// whose step moves nothing stops (OMPL's break); paths of < 3 states are returned as they
// are.
std::vector<std::vector<Vec3>> PathPlanner::smoothAll(const std::vector<std::vector<Vec3>>& segs) const {
    const bool canPass = configParser->getPathPlannerProperties().canPassGate;
    constexpr int kMaxSteps = 5;
    const double minChange = std::numeric_limits<double>::epsilon();
    auto half = [](const Vec3& a, const Vec3& b) {  // interpolate(a, b, 0.5): a + (b - a) * t
        return Vec3(a.x + (b.x - a.x) * 0.5, a.y + (b.y - a.y) * 0.5, a.z + (b.z - a.z) * 0.5);
    };
    auto distance = [](const Vec3& a, const Vec3& b) {  // left-to-right sum of squares
        double t = 0.0;
        for (int d = 0; d < 3; ++d) {
            const double diff = a[d] - b[d];
            t += diff * diff;
        }
        return std::sqrt(t);
    };
    std::vector<std::vector<Vec3>> st = segs;
    std::vector<char> live(st.size());
    for (size_t q = 0; q < st.size(); ++q) live[q] = st[q].size() >= 3;
    std::vector<double> pts, r1, r2;
    std::vector<Vec3> cand;
    std::vector<std::pair<uint32_t, uint32_t>> at;  // (path, state i) of each candidate move
    std::vector<uint8_t> okp, okr;
    for (int step = 0; step < kMaxSteps; ++step) {
        pts.clear();
        r1.clear();
        r2.clear();
        cand.clear();
        at.clear();
        for (size_t q = 0; q < st.size(); ++q) {
            if (!live[q]) continue;
            std::vector<Vec3>& s = st[q];
            std::vector<Vec3> sub;  // PathGeometric::subdivide
            sub.reserve(2 * s.size() - 1);
            sub.push_back(s[0]);
            for (size_t i = 1; i < s.size(); ++i) {
                const Vec3 m = half(sub.back(), s[i]);
                sub.push_back(m);
                sub.push_back(s[i]);
            }
            s.swap(sub);
            for (size_t i = 2; i + 1 < s.size(); i += 2) {
                Vec3 t1 = half(s[i - 1], s[i]);
                const Vec3 t2 = half(s[i], s[i + 1]);
                t1 = half(t1, t2);
                pts.insert(pts.end(), {s[i - 1].x, s[i - 1].y, s[i - 1].z});
                r1.insert(r1.end(), {s[i - 1].x, s[i - 1].y, s[i - 1].z, t1.x, t1.y, t1.z});
                r2.insert(r2.end(), {t1.x, t1.y, t1.z, s[i + 1].x, s[i + 1].y, s[i + 1].z});
                cand.push_back(t1);
                at.emplace_back((uint32_t)q, (uint32_t)i);
            }
        }
        if (cand.empty()) break;
        const int64_t n = (int64_t)cand.size();
        okp.assign((size_t)n, 0);
        okr.assign((size_t)(2 * n), 0);
        worldPtr->checkPoints(pts.data(), n, canPass, okp.data());
        worldPtr->checkRays(r1.data(), r2.data(), 2 * n, canPass, okr.data());
        std::vector<int> moved(st.size(), 0);
        for (int64_t j = 0; j < n; ++j) {
            if (!okp[j] || !okr[2 * j] || !okr[2 * j + 1]) continue;
            Vec3& si = st[at[j].first][at[j].second];
            if (distance(si, cand[j]) > minChange) {
                si = cand[j];
                ++moved[at[j].first];
            }
        }
        bool any = false;
        for (size_t q = 0; q < st.size(); ++q) {
            if (live[q] && moved[q] == 0) live[q] = 0;  // OMPL: a step that moved nothing ends the loop
            any = any || live[q];
        }
        if (!any) break;
    }
    return st;
}

// PathPlanner::pruneWaypoints — src/PathPlanner.cpp:232-265.  The reference checks
// ray(reference, current) one at a time; every pair it could ask for is checked in one
// batch (for all segments at once) and the same greedy walk is replayed on the answers.
std::vector<std::vector<Vec3>> PathPlanner::pruneAll(const std::vector<std::vector<Vec3>>& segs,
                                                     const std::vector<GateEnds>* ends) const {
    // ends (planPathsIncludeGates2): a segment whose points are, in order, among its
    // GateEnds' pts (bit for bit) reads the answers the shortcut's batch already holds
    auto same = [](const Vec3& a, const Vec3& b) { return std::memcmp(&a, &b, sizeof(Vec3)) == 0; };
    std::vector<std::vector<size_t>> at(segs.size());  // segment point -> its index in pts
    for (size_t q = 0; ends && q < segs.size() && q < ends->size(); ++q) {
        const GateEnds& g = (*ends)[q];
        if (!g.filled || segs[q].size() < 3) continue;
        std::vector<size_t> m;
        size_t k = 0;
        for (const Vec3& v : segs[q]) {
            while (k < g.pts.size() && !same(g.pts[k], v)) ++k;
            if (k == g.pts.size()) break;
            m.push_back(k++);
        }
        if (m.size() == segs[q].size()) at[q] = std::move(m);
    }
    std::vector<double> s1, s2;
    std::vector<size_t> base(segs.size() + 1, 0);
    size_t answered = 0;
    for (size_t q = 0; q < segs.size(); ++q) {
        base[q + 1] = base[q];
        if (segs[q].size() < 3) continue;
        if (!at[q].empty()) ++answered;
        else base[q + 1] += queue_pairs(segs[q], s1, s2);
    }
    std::vector<uint8_t> ok(base.back());
    const auto t_rays = std::chrono::steady_clock::now();
    if (!ok.empty()) worldPtr->checkRays(s1.data(), s2.data(), (int64_t)ok.size(), true, ok.data());  // canPassGate = true
    if (pairs_trace())
        std::fprintf(stderr, "pairs_trace: prune segments %zu (%zu answered by the shortcut's batch) pairs %zu rays %.1f us\n",
                     segs.size(), answered, ok.size(), us_since(t_rays));
    std::vector<std::vector<Vec3>> out(segs.size());
    for (size_t q = 0; q < segs.size(); ++q) {
        const auto& w = segs[q];
        const size_t L = w.size();
        if (L < 3) {
            out[q] = w;
            continue;
        }
        auto vis = [&](size_t i, size_t j) {  // pair (i, j), j >= i + 2, in the order queued
            if (!at[q].empty()) {
                const GateEnds& g = (*ends)[q];
                return g.vis[pair_index(g.pts.size(), at[q][i], at[q][j])] != 0;
            }
            return ok[base[q] + pair_index(L, i, j)] != 0;
        };
        std::vector<Vec3> pruned = {w[0]};
        size_t ref = 0;
        for (size_t cur = 2; cur < L; ++cur) {
            if (!vis(ref, cur)) {
                pruned.push_back(w[cur - 1]);
                ref = cur - 1;
            }
        }
        pruned.push_back(w[L - 1]);
        out[q] = std::move(pruned);
    }
    return out;
}

std::vector<Vec3> PathPlanner::pruneWaypoints(const std::vector<Vec3>& w) const { return pruneAll({w})[0]; }

}  // namespace epp
