// graph_search.h — the planner's host graph searches (standard library and epp/types.h only,
// so tests/graph_search_host.cpp runs them without a device): A* with stamped per-thread
// state, and its two graphs -- a problem's restricted rows and the whole k-NN table -- each
// searched forward and symmetrised (a node's edges: its row and the reverse of every row
// holding it).  Nodes 0 and 1 are start and goal; node indices are in node order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "epp/types.h"

namespace epp {

// A*'s state per host thread, reused across searches: an entry counts only when its stamp
// is the search's (no O(n) clearing per search); the heap keeps its storage.
struct QE {  // (16 bytes: the heap moves less than with a separate tie-break key)
    double f;
    int v;  // the node (its index is in node order): ties in f pop the lower index first, as
            // std::priority_queue<pair<double, int>, ..., std::greater<>> does
};
struct QECmp {
    bool operator()(const QE& a, const QE& b) const { return b.f < a.f || (!(a.f < b.f) && b.v < a.v); }
};
template <class V>  // (room to spare: a thread's first searches pay the page faults, not later ones)
void grow_to(V& v, size_t need, size_t init) {
    if (v.size() < need) v.resize(std::max<size_t>(need, std::max<size_t>(2 * v.size(), init)));
}
struct SearchState {
    std::vector<double> dist;
    std::vector<int> prev;
    std::vector<uint32_t> seen, done;  // stamps: dist/prev valid, closed
    std::vector<QE> heap;
    uint32_t cur = 0;
    int64_t pops = 0;  // nodes closed by the last search
    void begin(size_t n) {
        if (dist.size() < n) {  // (the stamps grow zeroed; the heap's storage reserved)
            const size_t c = std::max<size_t>(n, std::max<size_t>(2 * dist.size(), 16384));
            dist.resize(c);
            prev.resize(c);
            seen.resize(c, 0u);
            done.resize(c, 0u);
            heap.reserve(16 * c);
        }
        if (++cur == 0u) {  // (stamp wrap-around: clear once)
            std::fill(seen.begin(), seen.end(), 0u);
            std::fill(done.begin(), done.end(), 0u);
            cur = 1u;
        }
        heap.clear();
    }
    int prev_of(int v) const { return seen[v] == cur ? prev[v] : -1; }
};

// A* from node 0 to node 1 with the Euclidean distance to the goal (admissible and
// consistent for Euclidean edge costs).  pos(v): coordinates (node indices in node order:
// the lower breaks ties); expand(u, f, relax, closing): closing = false asks whether u may be
// closed -- false aborts (the caller then takes another graph) -- and closing = true calls
// relax(v) for u's edges.  Returns 1 (goal closed), 0 (exhausted), -1 (aborted).
template <class Pos, class Expand>
int astar(SearchState& ss, size_t nv, Pos&& pos, Expand&& expand) {
    ss.begin(nv);
    ss.pops = 0;
    const QECmp cmp;
    std::vector<QE>& q = ss.heap;
    const Vec3 gp = pos(1);
    auto push = [&](QE e) {
        q.push_back(e);
        std::push_heap(q.begin(), q.end(), cmp);
    };
    ss.seen[0] = ss.cur;
    ss.dist[0] = 0.0;
    ss.prev[0] = -1;
    push({(pos(0) - gp).norm(), 0});
    while (!q.empty()) {
        const QE top = q.front();
        std::pop_heap(q.begin(), q.end(), cmp);
        q.pop_back();
        const int u = top.v;
        if (ss.done[u] == ss.cur) continue;
        ++ss.pops;
        const Vec3 pu = pos(u);
        auto relax = [&](int v) {
            if (ss.done[v] == ss.cur) return;
            const Vec3 pv = pos(v);
            const double nd = ss.dist[u] + (pv - pu).norm();
            if (!(ss.seen[v] == ss.cur) || nd < ss.dist[v]) {
                ss.seen[v] = ss.cur;
                ss.dist[v] = nd;
                ss.prev[v] = u;
                push({nd + (pv - gp).norm(), v});
            }
        };
        if (!expand(u, top.f, relax, /*closing=*/false)) return -1;
        ss.done[u] = ss.cur;
        if (u == 1) return 1;
        expand(u, top.f, relax, /*closing=*/true);
    }
    return 0;
}

struct Searched {
    int r;         // astar's 1 / 0 / -1
    int64_t pops;  // nodes it closed
};
struct NodePos {  // pos(v) of nodes stored x, y, z
    const double* xyz;
    Vec3 operator()(int v) const { return Vec3(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2]); }
};
// The path of the last search on ss, which returned 1: start first.
template <class Pos>
std::vector<Vec3> extract_path(const SearchState& ss, Pos&& pos) {
    std::vector<Vec3> path;
    for (int v = 1; v >= 0; v = ss.prev_of(v)) path.push_back(pos(v));
    std::reverse(path.begin(), path.end());
    return path;
}

// ---- a problem's restricted rows: m nodes (compact indices), node u's row at row_of[u]
// (-1: none, the node lies outside the ellipsoid), k entries each, 0xFFFF: no edge
struct Rows {
    const uint16_t* rows;
    const int32_t* row_of;
    int k;
    int64_t m;
    template <class Relax>
    void edges(int u, Relax&& relax) const {
        const uint16_t* row = rows + (size_t)row_of[u] * k;
        for (int c = 0; c < k; ++c)
            if (row[c] != 0xFFFF) relax((int)row[c]);
    }
};
// The rows' reverse edges as a CSR: node v's sources at radj[roff[v] .. roff[v + 1]),
// ascending (compact = node order), as the device's reverse CSR gives the whole table's.
struct RowsReverse {
    std::vector<int32_t> roff, radj, fill;
    void build(const Rows& g) {
        const size_t m = (size_t)g.m;
        grow_to(roff, m + 1, 16384);
        std::fill(roff.begin(), roff.begin() + m + 1, 0);
        for (int u = 0; u < g.m; ++u)
            if (g.row_of[u] >= 0) g.edges(u, [&](int v) { ++roff[(size_t)v + 1]; });
        for (size_t v = 0; v < m; ++v) roff[v + 1] += roff[v];
        grow_to(radj, (size_t)roff[m], (size_t)16384 * g.k);
        grow_to(fill, m, 16384);
        std::copy(roff.begin(), roff.begin() + m, fill.begin());
        for (int u = 0; u < g.m; ++u)  // (u ascending: every run comes out sorted)
            if (g.row_of[u] >= 0) g.edges(u, [&](int v) { radj[(size_t)fill[v]++] = u; });
    }
    template <class Relax>
    void edges(int u, Relax&& relax) const {
        for (int32_t q = roff[(size_t)u]; q < roff[(size_t)u + 1]; ++q) relax(radj[(size_t)q]);
    }
};
// A* on the rows while every pop stays inside the bound and has its row (else -1): such a
// search pops exactly what the search over the whole table pops (host_plan_solve.cpp).
// rev: the symmetrised graph.  While the pops stay within the bound the reverse edges
// needed are those of rows here: a node without a row lies outside the ellipse
// (|s w| + |w g| > bound), so it is pushed with f > bound and never popped first.
template <class Pos>
Searched search_rows(SearchState& ss, const Rows& g, Pos&& pos, double bound, const RowsReverse* rev = nullptr) {
    const int r = astar(ss, (size_t)g.m, pos, [&](int u, double f, auto&& relax, bool closing) {
        if (!closing) return (f <= bound) && g.row_of[u] >= 0;
        g.edges(u, relax);
        if (rev) rev->edges(u, relax);
        return true;
    });
    return {r, ss.pops};
}

// ---- the whole k-NN table of n nodes as downloaded: narrow (n <= 65535) u16 entries,
// 0xFFFF: no edge, else i32, -1: no edge; roff / radj (for the symmetrised search): its
// reverse CSR, sources ascending, radj as narrow as nbr
struct Table {
    const void* nbr;
    bool narrow;
    int k;
    int32_t n;
    const int32_t* roff = nullptr;
    const void* radj = nullptr;
    int at(size_t e) const {
        if (!narrow) return static_cast<const int32_t*>(nbr)[e];
        const uint16_t x = static_cast<const uint16_t*>(nbr)[e];
        return x == 0xFFFF ? -1 : (int)x;
    }
    template <class Relax>
    void edges(int u, Relax&& relax) const {
        for (int c = 0; c < k; ++c) {
            const int v = at((size_t)u * k + c);
            if (v >= 0) relax(v);
        }
        for (int32_t q = roff ? roff[u] : 0, e = roff ? roff[u + 1] : 0; q < e; ++q)
            relax(narrow ? (int)static_cast<const uint16_t*>(radj)[q] : static_cast<const int32_t*>(radj)[q]);
    }
};
template <class Pos>
Searched search_table(SearchState& ss, const Table& t, Pos&& pos) {
    const int r = astar(ss, (size_t)t.n, pos, [&](int u, double, auto&& relax, bool closing) {
        if (closing) t.edges(u, relax);
        return true;
    });
    return {r, ss.pops};
}

}  // namespace epp
