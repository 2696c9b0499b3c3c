// poly_deriv.h — derivatives of a segment's polynomials by Horner over the derivative's own
// coefficients, and the time scaling of one polynomial: the two pieces feasibility.hip
// (k_traj_peaks, k_traj_scale) and thrust_scale.h share, so both compute the same bits.
// Every step is one IEEE fp64 multiply or add (-ffp-contract=off: no fused multiply-add).
// Plain C++ apart from the HIP qualifiers.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EPP_PD_FN __host__ __device__ __forceinline__
#else
#define EPP_PD_FN inline
#endif

namespace epp {

constexpr int kDerivCoeffs = 10;  // coefficients per polynomial (mav_trajectory_generation::Polynomial, N = 10)

// j! / (j-K)!: the coefficient of t^(j-K) in the K-th derivative of t^j (Polynomial::
// base_coefficients_, src/polynomial.cpp:145-160)
template <int K>
EPP_PD_FN constexpr double falling(int j) {
    double f = 1.0;
    for (int i = 0; i < K; ++i) f *= (double)(j - i);
    return f;
}

// Polynomial::evaluate(t, K) (polynomial.h:136-149): Horner over the derivative's coefficients
template <int K>
EPP_PD_FN double deriv(const double (&c)[kDerivCoeffs], double t) {
    constexpr int N = kDerivCoeffs;
    double r = falling<K>(N - 1) * c[N - 1];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = N - 2; j >= K; --j) r = r * t + falling<K>(j) * c[j];
    return r;
}

// Polynomial::scalePolynomialInTime(inv) (src/polynomial.cpp:199-205) in place: c[n] *= inv^n
// with the running factor f = f * inv
EPP_PD_FN void scale_polynomial_in_time(double* c, double inv) {
    double f = 1.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int n = 0; n < kDerivCoeffs; ++n) {
        c[n] = c[n] * f;
        f = f * inv;
    }
}

}  // namespace epp
