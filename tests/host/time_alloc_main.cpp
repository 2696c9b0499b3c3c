// Stand-alone host program over csrc/time_alloc.h (its own main; built by
// tests/test_time_alloc_host_cpu.py, also with AddressSanitizer and UBSan).  Reads records of
// hexadecimal doubles from stdin, one per line, and answers one line each:
//   cost   M T[M] C[M*30]                 ->  J status
//   times  M n h t_min T[M]               ->  variant n of the Mellinger gradient's times (M)
//   dir    M g[M]                         ->  the descent direction (M)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "time_alloc.h"

static bool read_all(const std::string& line, std::vector<double>& v) {
    std::istringstream in(line);
    std::string w;
    v.clear();
    while (in >> w) {
        char* end = nullptr;
        v.push_back(std::strtod(w.c_str(), &end));
        if (end == w.c_str()) return false;
    }
    return !v.empty();
}

static void put(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %a" : "%a", v[i]);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    std::string line;
    std::vector<double> v;
    while (std::getline(std::cin, line)) {
        if (!read_all(line, v)) return 2;
        const int M = (int)v[0];
        if (mode == "cost") {
            if (M < 0 || v.size() != 1 + (size_t)M * 31) return 3;
            int status = 0;
            const double J = epp::snap_cost_track(v.data() + 1, v.data() + 1 + M, M, &status);
            std::printf("%a %d\n", J, status);
        } else if (mode == "times") {
            if (M < 2 || v.size() != 4 + (size_t)M) return 3;
            std::vector<double> out(M);
            for (int i = 0; i < M; ++i) out[i] = epp::mellinger_time(v[4 + i], i, (int)v[1], M, v[2], v[3]);
            put(out);
            std::printf("\n");
        } else if (mode == "dir") {
            if (M < 2 || v.size() != 1 + (size_t)M) return 3;
            std::vector<double> out(M);
            for (int i = 0; i < M; ++i) out[i] = epp::descent_direction(v.data() + 1, i, M);
            put(out);
            std::printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}
