"""numpy truth for the peak search and the time scaling, in the reference's formulation
(not the kernels'): per segment, convolve derivative k with derivative k + 1 per dimension
and sum (external/poly_traj/src/segment.cpp:83-134), take the roots of that polynomial,
keep the real ones in [0, T], add both ends, evaluate the magnitude and take the maximum
(segment.cpp:136-185, src/trajectory.cpp:191-227); the scaling loop of
src/trajectory.cpp:385-429 with Polynomial::scalePolynomialInTime (src/polynomial.cpp:199-205).

Coefficients are (M, 3, 10) in increasing powers, as epp_minsnap_batch writes them.
"""
import numpy as np

N = 10
MAX_ROUNDS = 20   # kMaxCounter
TOL = 1e-3        # kTolerance


def deriv_coeffs(c, k):
    """Increasing-power coefficients of the k-th derivative of the polynomial c."""
    c = np.asarray(c, np.float64)
    for _ in range(k):
        c = c[1:] * np.arange(1, len(c))
    return c


def _polyval_inc(c, t):
    return np.polyval(np.asarray(c)[::-1], t)


def magnitude(seg, t, k):
    """|p^(k)(t)| of one segment (3, 10)."""
    return float(np.sqrt(sum(_polyval_inc(deriv_coeffs(seg[d], k), t) ** 2 for d in range(3))))


def segment_peak(seg, T, k):
    """(max magnitude of derivative k on [0, T], the earliest time it is reached at)."""
    conv = np.zeros(2 * (N - k) - 2)
    for d in range(3):
        conv += np.convolve(deriv_coeffs(seg[d], k), deriv_coeffs(seg[d], k + 1))
    cands = [0.0, float(T)]
    hi = np.trim_zeros(conv[::-1], "f")  # decreasing powers, leading zeros dropped
    if len(hi) > 1:
        for r in np.roots(hi):
            if abs(r.imag) <= 1e-9 * max(1.0, abs(r.real)) and 0.0 <= r.real <= T:
                cands.append(float(r.real))
    best_m, best_t = -1.0, 0.0
    for t in sorted(cands):
        m = magnitude(seg, t, k)
        if m > best_m:
            best_m, best_t = m, t
    return best_m, best_t


def traj_peaks(T, C):
    """[v_peak, t_v, a_peak, t_a] of one track; times from the start of the track."""
    T = np.asarray(T, np.float64)
    out = []
    for k in (1, 2):
        best_m, best_t, start = -1.0, 0.0, 0.0
        for i in range(len(T)):
            m, t = segment_peak(C[i], T[i], k)
            if m > best_m:
                best_m, best_t = m, start + t
            start += T[i]
        out += [best_m, best_t]
    return np.array(out)


def scale_polynomial_in_time(c, f):
    c = np.array(c, np.float64)
    scale = 1.0
    for n in range(c.shape[-1]):
        c[..., n] *= scale
        scale *= f
    return c


def scale_to_limits(T, C, v_max, a_max):
    """Trajectory::scaleSegmentTimesToMeetConstraints: (T, C, product of the factors,
    within_range, number of rounds that scaled)."""
    T = np.array(T, np.float64)
    C = np.array(C, np.float64)
    product, rounds, within = 1.0, 0, False
    for _ in range(MAX_ROUNDS):
        pk = traj_peaks(T, C)
        vv, av = pk[0] / v_max, pk[2] / a_max
        within = vv <= 1.0 + TOL and av <= 1.0 + TOL
        if within:
            break
        s = max(1.0, max(vv, np.sqrt(av)))
        T = T * s
        C = scale_polynomial_in_time(C, 1.0 / s)
        product *= s
        rounds += 1
    return T, C, product, within, rounds


def position(T, C, t):
    """Position (3,) of the track at time t from its start (t in [0, sum T])."""
    T = np.asarray(T, np.float64)
    i = 0
    while i < len(T) - 1 and t > T[i]:
        t -= T[i]
        i += 1
    return np.array([_polyval_inc(C[i][d], t) for d in range(3)])


def locate(T, t):
    """(segment, time in the segment) of the track time t, by the running sum peaks use."""
    T = np.asarray(T, np.float64)
    start = 0.0
    for i in range(len(T)):
        if t <= start + T[i] or i == len(T) - 1:
            return i, min(max(t - start, 0.0), T[i])
        start += T[i]
