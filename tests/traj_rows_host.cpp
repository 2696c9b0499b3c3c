// Host program of tests/test_trajcheck_cpu.py, over csrc/traj_sample.h's chunk producer
// (range_produce: the loop the kernels and the host paths run).  Plain C++: the header needs
// no HIP runtime on the host.  argv[1] = the step, or "samples" and then the step; then each
// track's segment times, tracks separated by "/".
//   rows (default)  per track one line: the number of rows and the last row's time
//   samples         per track one line per way of stepping, "<way> <rows> | seg tin tac ...":
//                   "step" (plain next / advance single steps; its line also carries
//                   range_count's answer after the rows) and "cap<N>" (range_produce called
//                   again and again with room for N samples)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "traj_sample.h"

static const int kCaps[] = {1, 7, 8, 9, 512, 513};

static void rows(const std::vector<double>& T, double dt) {
    epp::RangeIter it;
    it.init(T.data(), (int)T.size());
    int seg[epp::kRowChunk];
    double tin[epp::kRowChunk], tac[epp::kRowChunk], last = -1.0;
    long n = 0;
    for (int done = 0; !done;) {
        const int c = epp::range_produce(it, dt, epp::kRowChunk, seg, tin, tac, done);
        if (c) last = tac[c - 1];
        n += c;
    }
    std::printf("%ld %.17g\n", n, last);
}

static void samples(const std::vector<double>& T, double dt) {
    const int M = (int)T.size();
    epp::RangeIter it;
    it.init(T.data(), M);
    const long counted = (long)epp::range_count(it, dt);
    std::vector<int> seg;
    std::vector<double> tin, tac;
    auto line = [&](const char* way, int cap, long extra) {
        if (cap)
            std::printf("%s%d %zu |", way, cap, seg.size());
        else
            std::printf("%s %zu %ld |", way, seg.size(), extra);
        for (size_t k = 0; k < seg.size(); ++k) std::printf(" %d %a %a", seg[k], tin[k], tac[k]);
        std::printf("\n");
        seg.clear();
        tin.clear();
        tac.clear();
    };
    it.init(T.data(), M);
    int sg;
    double ti, ta;
    while (it.next(sg, ti, ta)) {
        seg.push_back(sg);
        tin.push_back(ti);
        tac.push_back(ta);
        it.advance(dt);
    }
    line("step", 0, counted);
    for (const int cap : kCaps) {
        std::vector<int> bs(cap);
        std::vector<double> bi(cap), ba(cap);
        it.init(T.data(), M);
        for (int done = 0; !done;) {
            const int c = epp::range_produce(it, dt, cap, bs.data(), bi.data(), ba.data(), done);
            seg.insert(seg.end(), bs.begin(), bs.begin() + c);
            tin.insert(tin.end(), bi.begin(), bi.begin() + c);
            tac.insert(tac.end(), ba.begin(), ba.begin() + c);
        }
        line("cap", cap, -1);
    }
}

int main(int argc, char** argv) {
    const bool all = argc > 1 && !std::strcmp(argv[1], "samples");
    const int first = all ? 3 : 2;
    if (argc < first + 1) return 2;
    const double dt = std::strtod(argv[first - 1], nullptr);
    std::vector<double> T;
    for (int i = first; i <= argc; ++i) {
        if (i == argc || argv[i][0] == '/') {
            (all ? samples : rows)(T, dt);
            T.clear();
        } else {
            T.push_back(std::strtod(argv[i], nullptr));
        }
    }
    return 0;
}
