// traj_sample.h — the sampling arithmetic of a fitted trajectory: the evaluateRange time
// recurrence (RangeIter), the one loop that steps it (range_produce / range_count), the
// polynomial evaluation and the Nfabian segment time.  Everything that samples a track runs
// these: the row sampler (minsnap.hip: k_sample_count, k_sample_rows), the host recurrences
// of the single-track paths (minsnap_refit.hip, host_generate.cpp), the fused checks (trajcheck.hip: k_traj_check, k_traj_sweep), the derivative sampler
// and the thrust / rate walk (thrust_rates.hip) and tests/traj_rows_host.cpp.  One definition,
// so all produce the same sample times, segments and positions bit for bit.  Plain C++ apart
// from the HIP qualifiers: a host program may include it without the HIP runtime.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPP_TS_HD __host__ __device__
#define EPP_TS_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define EPP_TS_HD
#define EPP_TS_FN inline
#endif

namespace epp {

constexpr int kPolyCoeffs = 10;  // coefficients per polynomial (mav_trajectory_generation::Polynomial, N = 10)
constexpr int kRowChunk = 512;   // samples a kernel's lane 0 produces per round (k_sample_rows, k_traj_*: per LDS half)

// One segment's time from its two waypoints.  The host paths (minsnap_refit.hip,
// host_generate.cpp) run it with the host's libm, as the reference does; the batch fit runs
// it on the device (solve_track, minsnap_solve.h).
EPP_TS_FN double nfabian(const double* p, const double* q, double vmax,
                                          double amax) {
    // estimateSegmentTimesNfabian — src/vertex.cpp:272-289 (magic 6.5)
    const double d0 = q[0] - p[0], d1 = q[1] - p[1], d2 = q[2] - p[2];
    const double distance = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    return distance / vmax * 2 * (1.0 + 6.5 * vmax / amax * exp(-distance / vmax * 2));
}

// Trajectory::evaluateRange control flow — src/trajectory.cpp:81-141.
struct RangeIter {
    const double* T;
    int M, i;
    double t_end, acc, tis, Ti;  // Ti = T[i], kept in a register (one LDS read per segment)
    EPP_TS_HD void init(const double* T_, int M_) {
        T = T_;
        M = M_;
        t_end = 0.0;  // max_time_ += segment.getTime()  trajectory.h:63-70
        for (int k = 0; k < M; ++k) t_end = t_end + T[k];
        acc = 0.0;
        for (i = 0; i < M; ++i) {  // t_start = 0
            acc = acc + T[i];
            if (acc > 0.0) break;
        }
        if (i >= M) i = M - 1;
        acc = acc - T[i];
        tis = 0.0 - acc;
        Ti = T[i];
    }
    // Advances to the next sample; returns false when the loop ends.
    EPP_TS_HD bool next(int& seg, double& t_in, double& t_acc) {
        while (acc < t_end) {
            if (tis > Ti) {
                tis = tis - Ti;
                i++;
                if (i >= M) return false;
                Ti = T[i];
                continue;
            }
            seg = i;
            t_in = tis;
            t_acc = acc;
            return true;
        }
        return false;
    }
    EPP_TS_HD void advance(double dt) {
        tis = tis + dt;
        acc = acc + dt;
    }
    // The next 8 samples at once when none of them rolls over into the next segment or
    // reaches the end (the same additions, in the same order, as 8 next/advance steps;
    // acc and tis only grow, so checking the 8th sample covers all).  False: nothing
    // consumed, take single steps.
    EPP_TS_HD bool fast8(double dt, double (&tin)[8], double (&tac)[8]) {
        double t = tis, a = acc;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 0; k < 8; ++k) {
            tin[k] = t;
            tac[k] = a;
            t = t + dt;
            a = a + dt;
        }
        if (!(tac[7] < t_end) || tin[7] > Ti) return false;
        tis = t;
        acc = a;
        return true;
    }
};

// THE stepping loop of the recurrence: eight samples at once where none rolls over, else
// one.  ROWS: the next (up to) cap samples into seg / tin / tac (segment, time in the segment,
// time), the eight only while eight more fit; else every sample left, stored nowhere.
// Returns how many; sets done to 1 when the recurrence ended, else leaves it alone (a call
// that fills cap exactly at the end reports the end with the next one, which returns 0).
template <bool ROWS, class Int>
EPP_TS_FN Int range_steps(RangeIter& iter, double dt, Int cap, int* seg, double* tin, double* tac, int& done) {
    RangeIter it = iter;  // (a local copy: the loop keeps it in registers)
    Int c = 0;
    int sg;
    double ti, ta, tin8[8], tac8[8];
    while (!ROWS || c < cap) {
        if ((!ROWS || c + 8 <= cap) && it.fast8(dt, tin8, tac8)) {
            if (ROWS) {
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int k = 0; k < 8; ++k) {
                    seg[c + k] = it.i;
                    tin[c + k] = tin8[k];
                    tac[c + k] = tac8[k];
                }
            }
            c += 8;
            continue;
        }
        if (!it.next(sg, ti, ta)) {
            done = 1;
            break;
        }
        if (ROWS) {
            seg[c] = sg;
            tin[c] = ti;
            tac[c] = ta;
        }
        ++c;
        it.advance(dt);
    }
    iter = it;
    return c;
}
EPP_TS_FN int range_produce(RangeIter& it, double dt, int cap, int* seg, double* tin, double* tac, int& done) {
    return range_steps<true>(it, dt, cap, seg, tin, tac, done);
}
EPP_TS_FN long long range_count(RangeIter& it, double dt) {
    int done;
    return range_steps<false>(it, dt, 0LL, nullptr, nullptr, nullptr, done);
}

// Polynomial::evaluate(t, k) — polynomial.h:136-149; B: the falling factorials
// B[k][j] = j! / (j-k)! (src/polynomial.cpp:145-160), row-major 10 x 10
// (Horner with fused multiply-adds: the sampled values are compared at 1e-6, the time
// column, which does not go through here, exactly)
EPP_TS_FN double poly_eval(const double* B, const double* c, double t, int k) {
    constexpr int N = kPolyCoeffs;
    double r = B[k * N + N - 1] * c[N - 1];
    for (int j = N - 2; j >= k; --j) r = fma(r, t, B[k * N + j] * c[j]);
    return r;
}

// B[k][j] = j! / (j-k)! itself (0 for j < k): an exact small integer (at most 9! = 362880),
// so a table filled from here, or a product with it, has the bits of the staged table's.
EPP_TS_FN constexpr double falling_factorial(int k, int j) {
    int f = j >= k ? 1 : 0;
    for (int i = 0; i < k; ++i) f *= j - i;
    return (double)f;
}

// poly_eval(B, c, t, K) for a compile-time K, without the table: the same products
// B[K][j] * c[j], each rounded once, and the same fused Horner steps, so the same bits
// (tests/test_gpu_thrust_rates.py compares them through the fused thrust / rate call).
template <int K>
EPP_TS_FN double poly_eval_order(const double* c, double t) {
    constexpr int N = kPolyCoeffs;
    double r = falling_factorial(K, N - 1) * c[N - 1];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = N - 2; j >= K; --j) r = fma(r, t, falling_factorial(K, j) * c[j]);
    return r;
}

// poly_eval(B, c, t, 0) without the table: B[0][j] = 1 and 1 * c[j] is c[j] exactly, so the
// same fused Horner steps give the same bits (tests/test_gpu_trajcheck.py compares them).
EPP_TS_FN double poly_eval_pos(const double* c, double t) {
    constexpr int N = kPolyCoeffs;
    double r = c[N - 1];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = N - 2; j >= 0; --j) r = fma(r, t, c[j]);
    return r;
}

}  // namespace epp
