"""TEST INFRASTRUCTURE ONLY -- a refined truth for the min-snap fit under arbitrary vertex
constraints: the KKT system of oracle/minsnap_np.solve (per-segment coefficients in normalised
time, equality constraints for the fixed derivatives and for the continuity of the free ones),
assembled in numpy.longdouble from exact integers and the segment times, solved by LU in
doubles and refined four times against the residual formed in numpy.longdouble.

The inputs the GPU tests use are measured against it (test_constrained_fit_inputs_cpu.py): the
oracle the device is compared with has to be ten times closer to it than the device's 1e-6.
"""
from math import factorial

import numpy as np

N = 10
K = 4  # snap
LD = np.longdouble


def _ff(j, k):
    return factorial(j) // factorial(j - k) if j >= k else 0


def _deriv_row(k, tau):
    """d^k/dtau^k of [1, tau, ..., tau^9] at tau = 0 or 1, exact integers as long doubles."""
    return np.array([LD(_ff(j, k)) * (LD(1) if tau == 1 or j == k else LD(0)) if j >= k else LD(0)
                     for j in range(N)], dtype=LD)


def _cost_unit():
    Q = np.zeros((N, N), LD)
    for a in range(K, N):
        for b in range(K, N):
            Q[a, b] = LD(_ff(a, K) * _ff(b, K)) / LD(a + b - 2 * K + 1)
    return Q


def kkt_system(fixed, n_vertices, times, dim):
    """The KKT matrix and right-hand side of minsnap_np.solve (fixed[(v, k)] = value vector of
    derivative k at vertex v; every vertex fixes its position; unfixed derivatives 1..4 of inner
    vertices are continuous) in long double.  Returns (kkt, rhs, nv): nv = 10 x segments."""
    M = n_vertices - 1
    T = np.asarray(times, np.float64).astype(LD)
    nv = N * M
    Qu = _cost_unit()
    rows, vals = [], []
    for v in range(n_vertices):
        for k in range(5):
            end = beg = None
            if v > 0:
                end = np.zeros(nv, LD)
                end[N * (v - 1):N * v] = _deriv_row(k, 1) / T[v - 1] ** k
            if v < M:
                beg = np.zeros(nv, LD)
                beg[N * v:N * v + N] = _deriv_row(k, 0) / T[v] ** k
            if (v, k) in fixed:
                val = np.asarray(fixed[(v, k)], np.float64).astype(LD)
                if end is not None:
                    rows.append(end)
                    vals.append(val)
                if beg is not None:
                    rows.append(beg)
                    vals.append(val)
            elif 0 < v < M:
                rows.append(end - beg)
                vals.append(np.zeros(dim, LD))
            else:
                raise ValueError("the end vertices fix all five derivatives")
    A = np.array(rows, dtype=LD)
    nc = len(rows)
    kkt = np.zeros((nv + nc, nv + nc), LD)
    for i in range(M):
        kkt[N * i:N * i + N, N * i:N * i + N] = 2 * Qu / T[i] ** (2 * K - 1)
    kkt[:nv, nv:] = A.T
    kkt[nv:, :nv] = A
    rhs = np.vstack([np.zeros((nv, dim), LD), np.array(vals, dtype=LD)])
    return kkt, rhs, nv


def solve_refined(fixed, n_vertices, times, dim, rounds=4, plain=False):
    """Coefficients (segments, dim, 10) in increasing powers of t.  plain: the LU solve without
    the refinement (what minsnap_np.solve computes, from the long-double matrix rounded)."""
    kkt, rhs, nv = kkt_system(fixed, n_vertices, times, dim)
    k64 = kkt.astype(np.float64)
    x = np.linalg.solve(k64, rhs.astype(np.float64)).astype(LD)
    for _ in range(0 if plain else rounds):
        res = rhs - kkt @ x
        x = x + np.linalg.solve(k64, res.astype(np.float64)).astype(LD)
    M = n_vertices - 1
    T = np.asarray(times, np.float64).astype(LD)
    out = np.zeros((M, dim, N))
    for i in range(M):
        scale = T[i] ** -np.arange(N).astype(LD)
        out[i] = (x[N * i:N * i + N] * scale[:, None]).T.astype(np.float64)
    return out
