// Host program of tests/test_thrust_rates_cpu.py, over csrc/thrust_rates.h (the per-sample
// arithmetic) and csrc/traj_sample.h (poly_eval, poly_eval_order, falling_factorial).  Plain
// C++: the headers need no HIP runtime on the host.  Reads lines of hex floats from stdin:
//   argv[1] = "samples":  ax ay az jx jy jz g   ->  thrust rate cos_tilt
//   argv[1] = "deriv":    t c0 .. c9            ->  for k = 0..9 poly_eval(B, c, t, k) with the
//                         table filled from falling_factorial, then poly_eval_order<2> and <3>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "thrust_rates.h"
#include "traj_sample.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const bool deriv = !std::strcmp(argv[1], "deriv");
    constexpr int N = epp::kPolyCoeffs;
    double B[N * N];
    for (int e = 0; e < N * N; ++e) B[e] = epp::falling_factorial(e / N, e % N);
    char tok[64];
    double v[N + 1];
    for (;;) {
        const int want = deriv ? N + 1 : 7;
        int got = 0;
        while (got < want && std::scanf("%63s", tok) == 1) v[got++] = std::strtod(tok, nullptr);
        if (got < want) break;
        if (deriv) {
            for (int k = 0; k < N; ++k) std::printf("%a ", epp::poly_eval(B, v + 1, v[0], k));
            std::printf("%a %a\n", epp::poly_eval_order<2>(v + 1, v[0]), epp::poly_eval_order<3>(v + 1, v[0]));
        } else {
            const epp::ThrustRates r = epp::thrust_rates(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
            std::printf("%a %a %a\n", r.thrust, r.rate, r.cos_tilt);
        }
    }
    return 0;
}
