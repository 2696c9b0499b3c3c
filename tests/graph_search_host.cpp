// Stand-alone host program for tests/test_graph_search_cpu.py: the planner's graph searches
// (csrc/graph_search.h) against a plain restatement written here, and the per-problem
// geometry (csrc/plan_geometry.h) printed for a numpy restatement.  One line per check,
// ending in "ok" or "FAIL"; the test asserts on the lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <queue>
#include <string>
#include <utility>
#include <vector>

#include "graph_search.h"
#include "plan_geometry.h"

using namespace epp;

namespace {
struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// A graph as the whole table: n x k, -1 no edge; node 0 the start, node 1 the goal.
struct Graph {
    int n = 0, k = 0;
    std::vector<double> xyz;
    std::vector<int32_t> nbr;
    std::vector<uint16_t> nbr16;  // the same, narrow
    Vec3 pos(int v) const { return Vec3(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]); }
    void narrow() {
        nbr16.resize(nbr.size());
        for (size_t e = 0; e < nbr.size(); ++e) nbr16[e] = nbr[e] < 0 ? 0xFFFF : (uint16_t)nbr[e];
    }
    std::vector<int> fwd(int u) const {
        std::vector<int> out;
        for (int c = 0; c < k; ++c)
            if (nbr[(size_t)u * k + c] >= 0) out.push_back(nbr[(size_t)u * k + c]);
        return out;
    }
    // forward edges, then the sources of the in-edges ascending (the symmetrised graph)
    std::vector<int> sym(int u) const {
        std::vector<int> out = fwd(u);
        for (int s = 0; s < n; ++s)
            for (int c = 0; c < k; ++c)
                if (nbr[(size_t)s * k + c] == u) out.push_back(s);
        return out;
    }
};

// Seeded uniform points in the unit cube, brute-force k nearest neighbours (nearest first),
// a random 30 % of the edges masked.
Graph knn_graph(int n, int k, uint64_t seed) {
    Graph g;
    g.n = n;
    g.k = k;
    Rng r{seed * 7919 + (uint64_t)n * 31 + k};
    g.xyz.resize(3 * (size_t)n);
    for (double& x : g.xyz) x = r.uni();
    g.nbr.assign((size_t)n * k, -1);
    std::vector<std::pair<double, int>> d;
    for (int u = 0; u < n; ++u) {
        d.clear();
        for (int v = 0; v < n; ++v)
            if (v != u) d.emplace_back((g.pos(v) - g.pos(u)).norm(), v);
        const size_t kk = std::min<size_t>(k, d.size());
        std::partial_sort(d.begin(), d.begin() + kk, d.end());
        for (size_t c = 0; c < kk; ++c) g.nbr[(size_t)u * k + c] = r.uni() < 0.3 ? -1 : d[c].second;
    }
    g.narrow();
    return g;
}

struct Ref {
    int code = 0;
    int64_t closed = 0;
    std::vector<int> path;
};
// The restatement: std::priority_queue of (f, node), plain dist / prev / closed, no stamps.
// gate(u, f): false aborts (-1), asked when u is popped first.
Ref ref_astar(int n, const std::function<Vec3(int)>& pos, const std::function<std::vector<int>(int)>& edges,
              const std::function<bool(int, double)>& gate) {
    Ref out;
    std::priority_queue<std::pair<double, int>, std::vector<std::pair<double, int>>, std::greater<>> pq;
    std::vector<double> dist(n, std::numeric_limits<double>::infinity());
    std::vector<int> prev(n, -1);
    std::vector<char> closed(n, 0);
    const Vec3 gp = pos(1);
    dist[0] = 0.0;
    pq.emplace((pos(0) - gp).norm(), 0);
    while (!pq.empty()) {
        const auto [f, u] = pq.top();
        pq.pop();
        if (closed[u]) continue;
        ++out.closed;
        if (!gate(u, f)) {
            out.code = -1;
            return out;
        }
        closed[u] = 1;
        if (u == 1) {
            out.code = 1;
            for (int v = 1; v >= 0; v = prev[v]) out.path.push_back(v);
            std::reverse(out.path.begin(), out.path.end());
            return out;
        }
        for (int v : edges(u)) {
            if (closed[v]) continue;
            const double nd = dist[u] + (pos(v) - pos(u)).norm();
            if (nd < dist[v]) {
                dist[v] = nd;
                prev[v] = u;
                pq.emplace(nd + (pos(v) - gp).norm(), v);
            }
        }
    }
    return out;
}

std::vector<int> nodes_of(const SearchState& ss) {
    std::vector<int> p;
    for (int v = 1; v >= 0; v = ss.prev_of(v)) p.push_back(v);
    std::reverse(p.begin(), p.end());
    return p;
}
bool same_bits(const Vec3& a, const Vec3& b) { return std::memcmp(&a, &b, sizeof(Vec3)) == 0; }

// s against the restatement: the code, the closed nodes and -- found -- the path's node
// indices and extract_path's positions, bit for bit.
template <class Pos>
bool equal(const Searched& s, const SearchState& ss, Pos&& pos, const Ref& ref) {
    if (s.r != ref.code || s.pops != ref.closed) return false;
    if (s.r != 1) return true;
    if (nodes_of(ss) != ref.path) return false;
    const std::vector<Vec3> p = extract_path(ss, pos);
    if (p.size() != ref.path.size()) return false;
    for (size_t i = 0; i < p.size(); ++i)
        if (!same_bits(p[i], pos(ref.path[i]))) return false;
    return true;
}

bool always(int, double) { return true; }

// The four whole-table searches (forward / symmetrised, wide / narrow) against the
// restatement, on ss.  The reverse CSR is built here by brute force, sources ascending.
bool check_table(const Graph& g, SearchState& ss, Ref* fwd_out = nullptr, Ref* sym_out = nullptr) {
    const NodePos pos{g.xyz.data()};
    auto P = [&](int v) { return g.pos(v); };
    const Ref rf = ref_astar(g.n, P, [&](int u) { return g.fwd(u); }, always);
    const Ref rs = ref_astar(g.n, P, [&](int u) { return g.sym(u); }, always);
    std::vector<int32_t> roff(g.n + 1, 0), radj;
    for (int v = 0; v < g.n; ++v) {
        for (int s = 0; s < g.n; ++s)
            for (int c = 0; c < g.k; ++c)
                if (g.nbr[(size_t)s * g.k + c] == v) radj.push_back(s);
        roff[v + 1] = (int32_t)radj.size();
    }
    std::vector<uint16_t> radj16(radj.begin(), radj.end());
    bool ok = true;
    for (int narrow = 0; narrow < 2; ++narrow) {
        Table t{narrow ? (const void*)g.nbr16.data() : (const void*)g.nbr.data(), narrow != 0, g.k, g.n};
        ok = ok && equal(search_table(ss, t, pos), ss, pos, rf);
        t.roff = roff.data();
        t.radj = narrow ? (const void*)radj16.data() : (const void*)radj.data();
        ok = ok && equal(search_table(ss, t, pos), ss, pos, rs);
    }
    if (fwd_out) *fwd_out = rf;
    if (sym_out) *sym_out = rs;
    return ok;
}

int mode_astar(int argc, char** argv) {  // astar n k seed...
    const int n = std::atoi(argv[2]), k = std::atoi(argv[3]);
    for (int a = 4; a < argc; ++a) {
        const Graph g = knn_graph(n, k, std::strtoull(argv[a], nullptr, 10));
        SearchState ss;
        Ref rf, rs;
        const bool ok = check_table(g, ss, &rf, &rs);
        std::printf("astar n %d k %d seed %s forward %d symmetrised %d closed %lld %s\n", n, k, argv[a], rf.code, rs.code,
                    (long long)rf.closed, ok ? "ok" : "FAIL");
    }
    // n = 2 with and without the edge 0 -> 1
    for (int edge = 0; edge < 2; ++edge) {
        Graph g;
        g.n = 2;
        g.k = k;
        g.xyz = {0.1, 0.2, 0.3, 0.9, 0.8, 0.7};
        g.nbr.assign(2 * (size_t)k, -1);
        if (edge) g.nbr[0] = 1;
        g.narrow();
        SearchState ss;
        Ref rf;
        const bool ok = check_table(g, ss, &rf);
        std::printf("astar n 2 k %d edge %d forward %d %s\n", k, edge, rf.code, ok && rf.code == edge ? "ok" : "FAIL");
    }
    return 0;
}

// A 9 x 9 x 1 unit lattice, the 4 axis neighbours: many nodes share f.
Graph lattice() {
    Graph g;
    g.n = 81;
    g.k = 4;
    std::vector<int> id(81);  // cell -> node: the corners (0, 0) and (8, 8) are nodes 0 and 1
    int next = 2;
    for (int c = 0; c < 81; ++c) id[c] = c == 0 ? 0 : c == 80 ? 1 : next++;
    g.xyz.resize(3 * 81);
    g.nbr.assign(81 * 4, -1);
    const int dx[4] = {1, -1, 0, 0}, dy[4] = {0, 0, 1, -1};
    for (int y = 0; y < 9; ++y)
        for (int x = 0; x < 9; ++x) {
            const int u = id[9 * y + x];
            g.xyz[3 * u] = x;
            g.xyz[3 * u + 1] = y;
            g.xyz[3 * u + 2] = 0;
            for (int c = 0; c < 4; ++c) {
                const int X = x + dx[c], Y = y + dy[c];
                if (X >= 0 && X < 9 && Y >= 0 && Y < 9) g.nbr[4 * u + c] = id[9 * Y + X];
            }
        }
    g.narrow();
    return g;
}

int mode_ties() {
    const Graph g = lattice();
    SearchState ss;
    Ref rf;
    const bool ok = check_table(g, ss, &rf);
    std::printf("ties forward %d closed %lld path %zu %s\n", rf.code, (long long)rf.closed, rf.path.size(),
                ok && rf.code == 1 ? "ok" : "FAIL");
    return 0;
}

int mode_stamps() {
    const Graph big = knn_graph(2000, 8, 3), small = knn_graph(64, 8, 3);
    {  // searches across the stamp's wrap-around, over stale stamps equal to those used after it
        SearchState ss;
        const bool s = check_table(small, ss) && check_table(big, ss);  // (stamps 1..8 left behind)
        ss.cur = 0xFFFFFFFEu;
        const bool a = check_table(big, ss);  // (four searches: the second wraps, then stamps 1..3)
        std::printf("stamps wrap cur %u %s\n", ss.cur, s && a && ss.cur == 3u ? "ok" : "FAIL");
    }
    {  // n = 64 after n = 2000 on one state: no stale entry is read
        SearchState ss;
        const bool a = check_table(big, ss), b = check_table(small, ss);
        std::printf("stamps small-after-big %s\n", a && b ? "ok" : "FAIL");
    }
    return 0;
}

// The rows of graph g as the device emits them for `bound`: a row for every node inside the
// ellipsoid |x - s| + |x - g| <= bound, the nodes the rows reference (and start, goal)
// numbered in node order (compact), row_of = -1 for those without a row.
struct RowSet {
    std::vector<int> node_of;  // compact -> node
    std::vector<double> xyz;
    std::vector<uint16_t> rows;
    std::vector<int32_t> row_of;
    Rows view(int k) const { return Rows{rows.data(), row_of.data(), k, (int64_t)node_of.size()}; }
};
RowSet rows_of(const Graph& g, double bound) {
    const Vec3 s = g.pos(0), t = g.pos(1);
    std::vector<char> has_row(g.n, 0), used(g.n, 0);
    used[0] = used[1] = 1;
    for (int u = 0; u < g.n; ++u)
        if (u < 2 || (g.pos(u) - s).norm() + (g.pos(u) - t).norm() <= bound) {
            has_row[u] = used[u] = 1;
            for (int v : g.fwd(u)) used[v] = 1;
        }
    RowSet rs;
    std::vector<int> compact(g.n, -1);
    for (int u = 0; u < g.n; ++u)
        if (used[u]) {
            compact[u] = (int)rs.node_of.size();
            rs.node_of.push_back(u);
            rs.xyz.insert(rs.xyz.end(), {g.xyz[3 * u], g.xyz[3 * u + 1], g.xyz[3 * u + 2]});
        }
    rs.row_of.assign(rs.node_of.size(), -1);
    for (int u = 0; u < g.n; ++u)
        if (has_row[u]) {
            rs.row_of[compact[u]] = (int32_t)(rs.rows.size() / g.k);
            for (int c = 0; c < g.k; ++c) {
                const int v = g.nbr[(size_t)u * g.k + c];
                rs.rows.push_back(v < 0 ? 0xFFFF : (uint16_t)compact[v]);
            }
        }
    return rs;
}

// path of the rows' search (compact) == path of the whole table's (node indices), positions bit-equal
bool same_path(const SearchState& ss, const RowSet& rs, const Graph& g, const Ref& whole) {
    const std::vector<int> p = nodes_of(ss);
    const std::vector<Vec3> xyz = extract_path(ss, NodePos{rs.xyz.data()});
    if (p.size() != whole.path.size() || xyz.size() != p.size()) return false;
    for (size_t i = 0; i < p.size(); ++i)
        if (rs.node_of[p[i]] != whole.path[i] || !same_bits(xyz[i], g.pos(whole.path[i]))) return false;
    return true;
}

int mode_rows(int argc, char** argv) {  // rows n k factor seed...
    const int n = std::atoi(argv[2]), k = std::atoi(argv[3]);
    const double factor = std::atof(argv[4]);
    for (int a = 5; a < argc; ++a) {
        const Graph g = knn_graph(n, k, std::strtoull(argv[a], nullptr, 10));
        auto P = [&](int v) { return g.pos(v); };
        const Ref wf = ref_astar(g.n, P, [&](int u) { return g.fwd(u); }, always);
        const Ref ws = ref_astar(g.n, P, [&](int u) { return g.sym(u); }, always);
        const double bound = factor * (g.pos(1) - g.pos(0)).norm() + 0.05;
        const RowSet rs = rows_of(g, bound);
        const Rows view = rs.view(k);
        const NodePos pos{rs.xyz.data()};
        SearchState ss;
        const Searched f = search_rows(ss, view, pos, bound);
        bool ok = true;
        int sym = -2;  // (-2: not run)
        int64_t pops = f.pops;  // of the search that decided
        if (f.r == 1) ok = wf.code == 1 && f.pops == wf.closed && same_path(ss, rs, g, wf);
        if (f.r == 0) {
            ok = wf.code == 0;  // the whole table's forward search fails too
            RowsReverse rev;
            rev.build(view);
            const Searched s2 = search_rows(ss, view, pos, bound, &rev);
            sym = s2.r;
            pops = s2.pops;
            if (s2.r == 1) ok = ok && ws.code == 1 && s2.pops == ws.closed && same_path(ss, rs, g, ws);
        }
        std::printf("rows n %d k %d seed %s forward %d symmetrised %d nodes %zu closed %lld %s\n", n, k, argv[a], f.r, sym,
                    rs.node_of.size(), (long long)pops, ok ? "ok" : "FAIL");
    }
    return 0;
}

// RowsReverse::build against "for every v, ascending u with v in row(u)".  A k-NN row lists k
// distinct nodes, so the device emits no node twice in a row; a made-up row that does is
// included all the same (the CSR then holds the source twice).
int mode_csr(int argc, char** argv) {  // csr n k seed...
    const int n = std::atoi(argv[2]), k = std::atoi(argv[3]);
    for (int a = 4; a <= argc; ++a) {
        const bool dup = a == argc;  // the last round: seed 1 with a duplicated entry
        const Graph g = knn_graph(n, k, dup ? 1 : std::strtoull(argv[a], nullptr, 10));
        RowSet rs = rows_of(g, 1.25 * (g.pos(1) - g.pos(0)).norm() + 0.05);
        if (dup) rs.rows[0] = rs.rows[1] = 1;
        const Rows view = rs.view(k);
        RowsReverse rev;
        rev.roff.assign(7, 99);  // (stale contents of a reused scratch)
        rev.build(view);
        bool ok = rev.roff[0] == 0;
        for (int64_t v = 0; v < view.m && ok; ++v) {
            std::vector<int32_t> want;
            for (int64_t u = 0; u < view.m; ++u)
                if (view.row_of[u] >= 0)
                    for (int c = 0; c < k; ++c)
                        if (view.rows[(size_t)view.row_of[u] * k + c] == v) want.push_back((int32_t)u);
            const std::vector<int32_t> got(rev.radj.begin() + rev.roff[v], rev.radj.begin() + rev.roff[v + 1]);
            ok = got == want;
        }
        std::printf("csr n %d k %d %s edges %d %s\n", n, k, dup ? "duplicate" : argv[a], (int)rev.roff[view.m], ok ? "ok" : "FAIL");
    }
    return 0;
}

int mode_geometry(char** argv) {  // geometry sx sy sz gx gy gz lox loy loz hix hiy hiz nmax ellipse restrict_ok
    double v[12];
    for (int i = 0; i < 12; ++i) v[i] = std::atof(argv[2 + i]);
    PlanBox b{{v[6], v[7], v[8]}, {v[9], v[10], v[11]}, std::atoll(argv[14]), std::atof(argv[15]), std::atoi(argv[16]) != 0};
    struct {  // (the fields of PlanSeg that plan_geometry reads and writes)
        double s[3], g[3], bound, gbound, glo[3], ghi[3], h;
        int32_t cap;
    } q{{v[0], v[1], v[2]}, {v[3], v[4], v[5]}, 0, 0, {}, {}, 0, 0};
    double kbox[6];
    plan_geometry(q, kbox, b);
    std::printf("%.17g %.17g %.17g %d", q.bound, q.gbound, q.h, (int)q.cap);
    for (int d = 0; d < 6; ++d) std::printf(" %.17g", kbox[d]);
    for (int d = 0; d < 3; ++d) std::printf(" %.17g", q.glo[d]);
    for (int d = 0; d < 3; ++d) std::printf(" %.17g", q.ghi[d]);
    std::printf("\n");
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "astar" && argc >= 4) return mode_astar(argc, argv);
    if (mode == "ties") return mode_ties();
    if (mode == "stamps") return mode_stamps();
    if (mode == "rows" && argc >= 5) return mode_rows(argc, argv);
    if (mode == "csr" && argc >= 4) return mode_csr(argc, argv);
    if (mode == "geometry" && argc == 17) return mode_geometry(argv);
    std::fprintf(stderr, "usage: graph_search_host astar|ties|stamps|rows|csr|geometry ...\n");
    return 2;
}
