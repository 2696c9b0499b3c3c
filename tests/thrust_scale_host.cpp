// Host program of tests/test_thrust_scale_cpu.py, over csrc/thrust_scale.h (with poly_deriv.h
// and thrust_rates.h).  Plain C++: the headers need no HIP runtime on the host.  Reads tracks
// as hex floats from stdin, one per record:
//   argv[1] = "scale":  M g f_min f_max rate_max cos_tilt_min T[M] C[M * 30]
//                       ->  scale status violated T[M] C[M * 30]   (thrust_scale_track)
//   argv[1] = "grid":   M g s T[M] C[M * 30]  ->  out[8]           (thrust_grid_track)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "thrust_scale.h"

static bool next(double& v) {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) return false;
    v = std::strtod(tok, nullptr);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const bool grid = !std::strcmp(argv[1], "grid");
    double m;
    while (next(m)) {
        const int M = (int)m;
        double head[5];
        for (int i = 0; i < (grid ? 2 : 5); ++i)
            if (!next(head[i])) return 3;
        std::vector<double> T((size_t)M), C((size_t)M * 30);
        for (double& v : T)
            if (!next(v)) return 3;
        for (double& v : C)
            if (!next(v)) return 3;
        if (grid) {
            double out[8];
            epp::thrust_grid_track(T.data(), C.data(), M, head[1], head[0], out);
            for (double v : out) std::printf("%a ", v);
        } else {
            const epp::ThrustLimits L{head[0], head[1], head[2], head[3], head[4]};
            if (!epp::thrust_limits_ok(L)) return 4;
            const epp::ThrustScale r = epp::thrust_scale_track(T.data(), C.data(), M, L);
            std::printf("%a %d %d ", r.scale, r.status, r.violated);
            for (double v : T) std::printf("%a ", v);
            for (double v : C) std::printf("%a ", v);
        }
        std::printf("\n");
    }
    return 0;
}
