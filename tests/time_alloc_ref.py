"""TEST INFRASTRUCTURE ONLY — the truth of the segment-time allocation (epp_traj_snap_cost,
epp_minsnap_time_gradient, epp_minsnap_optimize_times) in numpy.

The solve is oracle/minsnap_np.track_batch_refined (long double, refined, pinned to mpmath).
The cost is the closed-form Q of computeQuadraticCostJacobian (impl/
polynomial_optimization_linear_impl.h:567-583, derivative 4) in long double.  The gradient is
getCostAndGradientMellinger (impl/polynomial_optimization_nonlinear_impl.h:286-364) and the
descent is the rule of include/epp.h / DESIGN.md section 4, restated from those texts: nothing
here reads the kernels."""
from __future__ import annotations

from collections import namedtuple
from math import factorial

import numpy as np

import minsnap_np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

Params = namedtuple("Params", "h t_min step0 max_halvings ftol max_iter")
DEFAULTS = Params(0.1, 0.1, 0.5, 8, 1e-4, 20)


def b4(j: int) -> int:
    return factorial(j) // factorial(j - 4) if j >= 4 else 0


def q_terms(T, C):
    """c_a Q_ab c_b of every (segment, axis, a, b) in long double: (M, 3, 6, 6)."""
    T = np.asarray(T, np.float64).astype(LD).reshape(-1)
    C = np.asarray(C, np.float64).astype(LD).reshape(len(T), 3, 10)
    out = np.zeros((len(T), 3, 6, 6), LD)
    for a in range(4, 10):
        for b in range(4, 10):
            e = a + b - 7
            q = LD(b4(a) * b4(b) * 2) / LD(e) * T ** e
            out[:, :, a - 4, b - 4] = C[:, :, a] * q[:, None] * C[:, :, b]
    return out


def cost(T, C) -> float:
    """J = 0.5 sum c^T Q(T) c (PolynomialOptimization::computeCost)."""
    return float(LD(0.5) * q_terms(T, C).sum())


def cost_abs(T, C) -> float:
    """sum |c_a Q_ab c_b|: what the rounding of the 36-product sums scales with."""
    return float(np.abs(q_terms(T, C)).sum())


def cost_by_quadrature(T, C) -> float:
    """The integral of the squared snap by 6-point Gauss-Legendre per segment (exact for the
    degree-10 integrand), in long double."""
    x, w = np.polynomial.legendre.leggauss(6)
    x, w = x.astype(LD), w.astype(LD)
    T = np.asarray(T, np.float64).astype(LD).reshape(-1)
    C = np.asarray(C, np.float64).astype(LD).reshape(len(T), 3, 10)
    tot = LD(0)
    for i, Ti in enumerate(T):
        t = LD(0.5) * Ti * (x + 1)
        for d in range(3):
            snap = sum(LD(b4(j)) * C[i, d, j] * t ** (j - 4) for j in range(4, 10))
            tot += LD(0.5) * Ti * (w * snap * snap).sum()
    return float(tot)


def solve(wp, times, v0=None, a0=None, kkt=False):
    """Coefficients (B, M, 3, 10) of one waypoint set at B time allocations (B, M)."""
    wp = np.asarray(wp, np.float64).reshape(-1, 3)
    times = np.atleast_2d(np.asarray(times, np.float64))
    v0 = (0, 0, 0) if v0 is None else v0
    a0 = (0, 0, 0) if a0 is None else a0
    f = minsnap_np.track_batch if kkt else minsnap_np.track_batch_refined
    return f(np.broadcast_to(wp, (len(times),) + wp.shape), times, v0, a0)


def costs_at(wp, times, v0=None, a0=None, kkt=False) -> np.ndarray:
    times = np.atleast_2d(np.asarray(times, np.float64))
    C = solve(wp, times, v0, a0, kkt)
    return np.array([cost(t, c) for t, c in zip(times, C)])


def variants(T, h, t_min) -> np.ndarray:
    """(M + 1, M): row 0 the times themselves, row 1 + n the gradient's variant n."""
    T = np.asarray(T, np.float64)
    M = len(T)
    out = [T.copy()]
    for n in range(M if M > 1 else 0):
        v = np.array([T[i] + h if i == n else T[i] - h / (M - 1.0) for i in range(M)])
        out.append(np.maximum(t_min, v))
    return np.array(out)


def gradient(wp, T, h, t_min, v0=None, a0=None, kkt=False):
    """(J, g, Jv): the cost at T, the Mellinger quotients, every variant's cost."""
    V = variants(T, h, t_min)
    Jv = costs_at(wp, V, v0, a0, kkt)
    g = (Jv[1:] - Jv[0]) / h if len(V) > 1 else np.zeros(len(T))
    return Jv[0], g, Jv


def direction(g) -> np.ndarray:
    g = np.asarray(g, np.float64)
    M = len(g)
    d = np.zeros(M)
    for i in range(M):
        s = 0.0
        for n in range(M):
            if n != i:
                s = s + g[n]
        d[i] = g[i] - s / (M - 1.0)
    return d


def seq_sum(x) -> float:
    s = 0.0
    for v in x:
        s = s + float(v)
    return s


def first_alpha(T, d, step0) -> float:
    return step0 * float(np.min(T)) / float(np.max(np.abs(d)))


def rescale(T, sum0) -> np.ndarray:
    return np.asarray(T, np.float64) * (sum0 / seq_sum(T))


def step_from_grad(T, g, halvings, step0, sum0=None) -> np.ndarray:
    """One accepted step from a given gradient after `halvings` halvings, then the rescaling."""
    T = np.asarray(T, np.float64)
    d = direction(g)
    alpha = first_alpha(T, d, step0)
    for _ in range(halvings):
        alpha = 0.5 * alpha
    return rescale(T - alpha * d, seq_sum(T) if sum0 is None else sum0)


Result = namedtuple("Result", "T C cost0 cost1 iters status trace")
# one entry per iteration: halvings of the accepted step (-1: none accepted), the smallest
# relative margin of its J' < J comparisons and of its stopping test, the smallest distance of
# a trial time from t_min, whether a trial was refused by the bound / by the cost
Iter = namedtuple("Iter", "halvings cost_margin tmin_margin refused_bound refused_cost costs")


def descent(wp, T, p: Params = DEFAULTS, v0=None, a0=None) -> Result:
    T = np.asarray(T, np.float64).copy()
    M = len(T)
    J0 = float(costs_at(wp, T, v0, a0)[0])
    trace = []
    if M == 1 or p.max_iter <= 0 or not np.isfinite(J0):
        return Result(T, solve(wp, T, v0, a0)[0], J0, J0, 0, 0, trace)
    sum0 = seq_sum(T)
    J, iters, status = J0, 0, 2
    for _ in range(p.max_iter):
        Jc, g, _ = gradient(wp, T, p.h, p.t_min, v0, a0)
        assert Jc == J
        d = direction(g)
        if not np.isfinite(d).all():
            status = 1
            break
        if np.max(np.abs(d)) == 0.0:
            status = 0
            break
        alpha = first_alpha(T, d, p.step0)
        acc, cm, tm, rb, rc, js = -1, np.inf, np.inf, 0, 0, [J]
        for k in range(p.max_halvings + 1):
            Tn = T - alpha * d
            tm = min(tm, float(np.min(np.abs(Tn - p.t_min))))
            if (Tn >= p.t_min).all():
                Jn = float(costs_at(wp, Tn, v0, a0)[0])
                js.append(Jn)
                cm = min(cm, abs(Jn - J) / J)
                if Jn < J:
                    acc = k
                    break
                rc += 1
            else:
                rb += 1
            alpha = 0.5 * alpha
        if acc < 0:
            trace.append(Iter(-1, cm, tm, rb, rc, js))
            status = 1
            break
        iters += 1
        dec, Jold = J - Jn, J
        T, J = Tn, Jn
        cm = min(cm, abs(dec - p.ftol * Jold) / Jold)
        trace.append(Iter(acc, cm, tm, rb, rc, js))
        if dec <= p.ftol * Jold:
            status = 0
            break
    T = rescale(T, sum0)
    C = solve(wp, T, v0, a0)[0]
    return Result(T, C, J0, cost(T, C), iters, status, trace)


def scipy_optimum(wp, T, t_min, v0=None, a0=None):
    """(T*, J*): the truth cost minimised over the segment times at constant total time and
    T >= t_min by scipy's SLSQP, started from T and restarted from its own answer."""
    from scipy.optimize import minimize
    T = np.asarray(T, np.float64)
    total = seq_sum(T)
    scale = float(costs_at(wp, T, v0, a0)[0])
    x = T
    for _ in range(3):
        res = minimize(lambda t: float(costs_at(wp, t, v0, a0)[0]) / scale, x, method="SLSQP",
                       bounds=[(t_min, None)] * len(T),
                       constraints=[{"type": "eq", "fun": lambda t: np.sum(t) - total}],
                       options={"ftol": 1e-14, "maxiter": 200})
        x = res.x
    return x, float(costs_at(wp, x, v0, a0)[0])


def reference_arithmetic_cost(T, C) -> float:
    """computeCost as the reference computes it: Q and c^T Q c in doubles."""
    s = 0.0
    for Ti, Ci in zip(np.asarray(T, np.float64), np.asarray(C, np.float64)):
        Q = np.zeros((10, 10))
        for a in range(4, 10):
            for b in range(4, 10):
                e = a + b - 7
                Q[a, b] = float(b4(a)) * float(b4(b)) * Ti ** e * 2.0 / e
        for d in range(3):
            s += Ci[d] @ Q @ Ci[d]
    return 0.5 * s


def reference_distance(tracks, h, t_min):
    """How far the reference-arithmetic solve (minsnap_np.track_batch, the oracle's KKT
    formulation, its cost summed in doubles) lands from the truth in J, over every variant of
    every track given, in units of sum |c_a Q_ab c_b| (what a cost's rounding scales with; the
    sum cancels to ~1e-6 of it): the maximum.  Returns (distance, {name: (V, J, A)}) with each
    track's variants V, truth costs J and scales A."""
    worst, per = 0.0, {}
    for tr in tracks:
        V = variants(tr.T, h, t_min)
        Ct = solve(tr.wp, V, tr.v0, tr.a0)
        Ck = solve(tr.wp, V, tr.v0, tr.a0, kkt=True)
        J = np.array([cost(v, c) for v, c in zip(V, Ct)])
        A = np.array([cost_abs(v, c) for v, c in zip(V, Ct)])
        Jk = np.array([reference_arithmetic_cost(v, c) for v, c in zip(V, Ck)])
        worst = max(worst, float(np.max(np.abs(Jk - J) / A)))
        per[tr.name] = (V, J, A)
    return worst, per
