// Host program of tests/test_trajcheck_cpu.py: for every track on the command line
// (argv[1] = the step, then each track's segment times, tracks separated by "/") one line
// with the number of rows csrc/traj_sample.h's RangeIter produces, stepped exactly as the
// kernels step it (eight samples at once where none rolls over, else one), and the last
// row's time.  Plain C++: the header needs no HIP runtime on the host.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "traj_sample.h"

static void track(const std::vector<double>& T, double dt) {
    epp::RangeIter it;
    it.init(T.data(), (int)T.size());
    long n = 0;
    int seg = 0;
    double tin = 0, tac = 0, last = -1.0, tin8[8], tac8[8];
    for (;;) {
        if (it.fast8(dt, tin8, tac8)) {
            n += 8;
            last = tac8[7];
            continue;
        }
        if (!it.next(seg, tin, tac)) break;
        ++n;
        last = tac;
        it.advance(dt);
    }
    std::printf("%ld %.17g\n", n, last);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const double dt = std::strtod(argv[1], nullptr);
    std::vector<double> T;
    for (int i = 2; i < argc; ++i) {
        if (argv[i][0] == '/') {
            track(T, dt);
            T.clear();
        } else {
            T.push_back(std::strtod(argv[i], nullptr));
        }
    }
    track(T, dt);
    return 0;
}
