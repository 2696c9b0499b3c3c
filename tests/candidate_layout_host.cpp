// candidate_layout_host — the host image and the device block layout of a batch of candidate
// waypoint sets (csrc/candidate_batch.h: CandidateLayout), stand-alone on the CPU.
//   candidate_layout_host G W_0 W_1 ...   sets of W_k waypoints, a gate table of G frames
// Reserves, after the parts every call shares, the parts of each candidate call of
// host_candidates.cpp in turn (each on a layout of its own) and checks that every part starts
// 256-byte aligned, that no two parts with elements overlap, that all lie inside the block and
// that the block is a multiple of 256 bytes; and the host image: offsets, waypoints, the
// segment ranges.  One line per check, ending in " ok" or " FAILED".  A set of fewer than two
// waypoints must throw before anything is laid out: the line "short ok".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "candidate_batch.h"

using epp::CandidateLayout;
using epp::Part;
using epp::Vec3;

namespace {
struct Span {
    std::string name;
    size_t off, bytes;
};
int failures = 0;
void line(const std::string& what, bool ok) {
    std::printf("%s %s\n", what.c_str(), ok ? "ok" : "FAILED");
    failures += !ok;
}
template <class T>
void add(std::vector<Span>& v, const char* name, const Part<T>& p) {
    v.push_back({name, p.off, p.bytes()});
}
std::vector<Span> shared(const CandidateLayout& L) {
    std::vector<Span> v;
    add(v, "wp", L.p_wp);
    add(v, "T", L.p_T);
    add(v, "C", L.p_C);
    add(v, "off", L.p_off);
    add(v, "fit", L.p_fit);
    return v;
}
void check(const std::string& call, const CandidateLayout& L, const std::vector<Span>& v) {
    bool aligned = true, inside = L.bytes % 256 == 0, apart = true;
    for (const Span& a : v) {
        aligned = aligned && a.off % 256 == 0;
        inside = inside && a.off + a.bytes <= L.bytes;
        for (const Span& b : v)
            if (&a != &b && a.bytes && b.bytes) apart = apart && (a.off + a.bytes <= b.off || b.off + b.bytes <= a.off);
    }
    line(call + " aligned", aligned);
    line(call + " inside", inside);
    line(call + " apart", apart);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: candidate_layout_host G W_0 W_1 ...\n");
        return 2;
    }
    const size_t G = (size_t)std::atol(argv[1]);
    std::vector<std::vector<Vec3>> sets;
    bool any_short = false;
    for (int i = 2; i < argc; ++i) {
        const long W = std::atol(argv[i]);
        any_short = any_short || W < 2;
        std::vector<Vec3> s;
        for (long w = 0; w < W; ++w) s.emplace_back(i + 0.25 * w, -(double)w, 100.0 * i + w);
        sets.push_back(std::move(s));
    }
    if (any_short) {
        bool threw = false;
        try {
            CandidateLayout L(sets);
        } catch (const std::invalid_argument& e) {
            threw = std::string(e.what()) == "At least two waypoints are required";
        }
        line("short", threw);
        return failures != 0;
    }
    const size_t n = sets.size();
    {  // the host image
        const CandidateLayout L(sets);
        size_t total = 0;
        bool off_ok = L.off.size() == n + 1 && L.off[0] == 0, wp_ok = true, seg_ok = true;
        for (size_t k = 0; k < n && off_ok; ++k) {
            seg_ok = seg_ok && L.seg_begin(k) == total - k;
            for (size_t w = 0; w < sets[k].size(); ++w, ++total)
                wp_ok = wp_ok && L.wp.size() >= 3 * (total + 1) && L.wp[3 * total] == sets[k][w].x &&
                        L.wp[3 * total + 1] == sets[k][w].y && L.wp[3 * total + 2] == sets[k][w].z;
            off_ok = L.off[k + 1] == (int32_t)total;
        }
        std::printf("image n %zu total %zu nseg %zu bytes %zu\n", L.n, L.total, L.nseg, L.bytes);
        line("counts", L.n == n && L.total == total && L.nseg == total - n && L.wp.size() == 3 * total);
        line("offsets", off_ok);
        line("waypoints", wp_ok);
        line("segments", seg_ok && L.seg_begin(n) == L.nseg);
        line("shared sizes", L.p_wp.count == 3 * total && L.p_T.count == L.nseg && L.p_C.count == 30 * L.nseg &&
                                 L.p_off.count == n + 1 && L.p_fit.count == n);
        check("shared", L, shared(L));
    }
    {  // checkCandidateTrajectories
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "row", L.part<int64_t>(n));
        add(v, "time", L.part<double>(n));
        check("check", L, v);
    }
    {  // sweepCandidateTrajectories
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "row", L.part<int64_t>(n));
        add(v, "chord", L.part<int64_t>(n));
        add(v, "row_time", L.part<double>(n));
        add(v, "chord_time", L.part<double>(n));
        check("sweep", L, v);
    }
    {  // candidateFirstHits, candidateClearances: int64, two doubles, int32 per set
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "chord", L.part<int64_t>(n));
        add(v, "t", L.part<double>(n));
        add(v, "time", L.part<double>(n));
        add(v, "obb", L.part<int32_t>(n));
        check("hits", L, v);
    }
    for (int with_offsets = 0; with_offsets < 2; ++with_offsets) {  // candidateGatePasses
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "frames", L.part<double>(G * 5));
        add(v, "chord", L.part<int64_t>(n * G));
        add(v, "time", L.part<double>(n * G));
        add(v, "offsets", L.part<double>(with_offsets ? n * G * 2 : 0));
        add(v, "passed", L.part<int32_t>(n));
        check(with_offsets ? "gates+offsets" : "gates", L, v);
    }
    for (int with_rows = 0; with_rows < 2; ++with_rows) {  // candidateThrustRates
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "out", L.part<double>(n * 8));
        add(v, "rows", L.part<int64_t>(with_rows ? n * 4 : 0));
        check(with_rows ? "thrust+rows" : "thrust", L, v);
    }
    {  // candidateFlyableScales
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "scale", L.part<double>(n));
        add(v, "status", L.part<int32_t>(n));
        add(v, "violated", L.part<int32_t>(n));
        check("flyable", L, v);
    }
    for (int optimize = 0; optimize < 2; ++optimize) {  // candidateSnapCosts
        CandidateLayout L(sets);
        auto v = shared(L);
        add(v, "cost0", L.part<double>(optimize ? n : 0));
        add(v, "cost", L.part<double>(n));
        add(v, "iters", L.part<int32_t>(optimize ? n : 0));
        add(v, "status", L.part<int32_t>(n));
        check(optimize ? "snap+optimize" : "snap", L, v);
    }
    return failures != 0;
}
