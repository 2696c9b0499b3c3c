"""CPU restatement of "clearance" (include/epp.h: epp_states_clearance, epp_traj_clearance_batch)
in numpy float64, every operation one IEEE multiply, add or subtract in the definition's
association:

    dx = px - cx;  dy = py - cy;  dz = pz - cz
    lx = c*dx + s*dy;  ly = c*dy - s*dx
    ex = max(|lx| - hx, 0);  ey = max(|ly| - hy, 0);  ez = max(|dz| - hz, 0)
    d2_i = (ex*ex + ey*ey) + ez*ez            (filling OBBs: skipped)

d2 = min_i d2_i, nearest = the lowest i that attains it, (+inf, -1) when nothing does (no
collision OBB, or a non-finite point: a NaN d2_i never updates the minimum).

The rows of a track are those of Trajectory::evaluateRange(0, max_time, dt): the recurrence of
csrc/traj_sample.h restated here (its row count and time column are checked against the
oracle's sampler, oracle.sample_traj, in test_clearance_inputs_cpu.py) and the positions by
the device's fused Horner, each step one correctly rounded fma (libm's through ctypes; exact
rational arithmetic where there is no libm).  The oracle's own positions come from an unfused
Horner and differ from the device's by ~1e-15, more than the 1 ulp the distances are held to.
"""
import ctypes
import ctypes.util
from fractions import Fraction

import numpy as np


def d2_matrix(obbs, pts):
    """(n_points, n_obbs) d2_i, +inf in the columns of filling OBBs (NaN for NaN points)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty((len(pts), len(obbs)))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, o in enumerate(obbs):
            c, s = float(o["rot"][0]), float(o["rot"][3])
            dx, dy, dz = pts[:, 0] - o["center"][0], pts[:, 1] - o["center"][1], pts[:, 2] - o["center"][2]
            lx = c * dx + s * dy
            ly = c * dy - s * dx
            e = []
            for l, h in ((lx, o["half"][0]), (ly, o["half"][1]), (dz, o["half"][2])):
                a = np.abs(l) - h
                e.append(np.where(a < 0.0, 0.0, a))
            d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            out[:, i] = np.where(np.isnan(d2), np.nan, np.inf) if o["filling"] else d2
    return out


def reduce_min(d2):
    """(min, lowest index attaining it) per row of d2_matrix's result; (+inf, -1) if none."""
    d = np.where(np.isnan(d2), np.inf, d2)
    if d.shape[1] == 0:
        return np.full(len(d), np.inf), np.full(len(d), -1, np.int32)
    best = d.min(axis=1)
    idx = d.argmin(axis=1).astype(np.int32)  # (the first minimum)
    idx[np.isinf(best)] = -1
    return best, idx


def states(obbs, pts):
    """(d2, nearest) per point."""
    return reduce_min(d2_matrix(obbs, pts))


# ---- the rows of a fitted track ------------------------------------------------------------
def _libm_fma():
    name = ctypes.util.find_library("m")
    if not name:
        return None
    f = ctypes.CDLL(name).fma
    f.restype = ctypes.c_double
    f.argtypes = [ctypes.c_double] * 3
    return f


_FMA = _libm_fma()


def fma(a, b, c):
    """a * b + c rounded once."""
    if _FMA is not None:
        return _FMA(a, b, c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def recurrence(T, dt):
    """(segment, time in the segment, time) per row: RangeIter (csrc/traj_sample.h) step by step."""
    T = [float(t) for t in T]
    M = len(T)
    seg, tin, tac = [], [], []
    if M == 0:
        return np.zeros(0, int), np.zeros(0), np.zeros(0)
    t_end = 0.0
    for t in T:
        t_end = t_end + t
    acc, i = 0.0, M
    for k in range(M):
        acc = acc + T[k]
        if acc > 0.0:
            i = k
            break
    if i >= M:
        i = M - 1
    acc = acc - T[i]
    tis = 0.0 - acc
    while acc < t_end:
        if tis > T[i]:
            tis = tis - T[i]
            i += 1
            if i >= M:
                break
            continue
        seg.append(i)
        tin.append(tis)
        tac.append(acc)
        tis = tis + dt
        acc = acc + dt
    return np.array(seg, int), np.array(tin), np.array(tac)


def horner(c, t):
    """poly_eval_pos: fused Horner, the highest coefficient first."""
    c = [float(v) for v in c]
    k = len(c) - 1
    while k > 0 and c[k] == 0.0:  # (fma(+0, t, c) = c for finite t: the leading zeros change nothing)
        k -= 1
    r = c[k]
    for j in range(k - 1, -1, -1):
        r = fma(r, t, c[j])
    return r


def sample_rows(T, C, dt):
    """(positions R x 3, time column R) of a track's rows; the time column as epp_sample_batch
    writes it with t0 == NULL (time + 0.0)."""
    seg, tin, tac = recurrence(T, dt)
    C = np.asarray(C, np.float64)
    xyz = np.empty((len(seg), 3))
    for r in range(len(seg)):
        for d in range(3):
            xyz[r, d] = horner(C[seg[r], d], float(tin[r])) if np.isfinite(tin[r]) else np.nan
    return xyz, tac + 0.0


def track_from_rows(d2, near, time):
    """(d2, row, time, nearest) of one track from its rows' (d2, nearest): the earliest row
    that attains the minimum; (+inf, -1, -1.0, -1) without a finite one."""
    if len(d2) == 0 or not np.isfinite(d2).any():
        return np.inf, -1, -1.0, -1
    r = int(np.argmin(d2))
    return float(d2[r]), r, float(time[r]), int(near[r])


def tracks(obbs, Ts, Cs, dt, rows=None):
    """(d2, row, time, nearest) arrays over the tracks; rows: precomputed sample_rows results."""
    out = []
    for k in range(len(Ts)):
        xyz, time = rows[k] if rows is not None else sample_rows(Ts[k], Cs[k], dt)
        d2, near = states(obbs, xyz)
        out.append(track_from_rows(d2, near, time))
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out], np.int64),
            np.array([o[2] for o in out]), np.array([o[3] for o in out], np.int32))


def ulps(a, b):
    """|a - b| in units of the spacing at b; 0 where both are the same infinity."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (a == b)
    with np.errstate(invalid="ignore"):
        u = np.abs(a - b) / np.spacing(np.where(np.isfinite(b), np.abs(b), 1.0))
    return np.where(same, 0.0, u)
