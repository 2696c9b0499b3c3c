"""CPU restatement of "edge clearance" (include/epp.h: epp_motions_clearance,
epp_traj_chord_clearance_batch; csrc/edge_clearance.h): the Euclidean distance between a
straight edge s -> e and the nearest collision OBB, in numpy float64, every operation one IEEE
multiply, add, subtract or divide in the definition's association (numpy fuses nothing).

Per OBB i (centre, c, s, half sizes h; not inflated), with the endpoints taken into the box
frame as clearance's d2 takes a point (a from s, b from e) and d = b - a per axis:

    F(q) = (ex*ex + ey*ey) + ez*ez,   e_k = max(|q_k| - h_k, 0)            (clearance's d2)
    G(q) = (wx + wy) + wz,            w_k = e_k * (q_k < 0 ? -d_k : d_k)   (half of f')
    q(t) = a + t*d  per axis

    1. t = 0:  f = F(a)                      2. t = 1:  f = F(b)
    3. axes x, y, z, face -h_k then +h_k:  t = (-+h_k - a_k) / d_k, kept iff 0 < t < 1: f = F(q(t))
       the bracket of the zero of G:  (tl, gl) starts at (0, G(a)), (tr, gr) at (1, G(b));
       a kept t with g = G(q(t)) < 0 and t > tl replaces (tl, gl), one with g >= 0 and t < tr
       replaces (tr, gr)
    4. iff G(a) < 0 < G(b):  t* = tl + (tr - tl) * ((-gl) / (gr - gl)),  f = F(q(t*))

d2_i = the smallest f, strict < in this order from +inf, and t_i its t.  Over the world: every
OBB in order, strict <, so the lowest index wins; an edge with a non-finite coordinate takes
part in nothing: (+inf, -1.0, -1), as does a world without a collision OBB.  A filling OBB's
column is +inf.

truth(): independent of all that -- a ternary search of the convex f(t) on [0, 1] per OBB in
long double, minimum over the OBBs.
"""
import numpy as np

import clearance_ref as cr


def _local(o, p):
    c, s = float(o["rot"][0]), float(o["rot"][3])
    dx, dy, dz = p[:, 0] - o["center"][0], p[:, 1] - o["center"][1], p[:, 2] - o["center"][2]
    return [c * dx + s * dy, c * dy - s * dx, dz]


def _F(q, h):
    e = []
    for k in range(3):
        a = np.abs(q[k]) - h[k]
        e.append(np.where(a < 0.0, 0.0, a))
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], e


def _G(q, e, d):
    w = [e[k] * np.where(q[k] < 0.0, -d[k], d[k]) for k in range(3)]
    return (w[0] + w[1]) + w[2]


def obb_d2(o, s1, s2):
    """(d2_i, t_i) of OBB o (not filling) for the edges s1 -> s2 (n x 3 each, finite)."""
    h = [float(v) for v in o["half"]]
    with np.errstate(all="ignore"):
        a, b = _local(o, s1), _local(o, s2)
        d = [b[k] - a[k] for k in range(3)]
        best, tb = np.full(len(s1), np.inf), np.full(len(s1), -1.0)

        def cand(ok, t, f):
            nonlocal best, tb
            lt = ok & (f < best)
            best = np.where(lt, f, best)
            tb = np.where(lt, t, tb)

        yes = np.ones(len(s1), bool)
        f0, e0 = _F(a, h)
        f1, e1 = _F(b, h)
        g0, g1 = _G(a, e0, d), _G(b, e1, d)
        cand(yes, np.zeros(len(s1)), f0)
        cand(yes, np.ones(len(s1)), f1)
        tl, gl = np.zeros(len(s1)), g0
        tr, gr = np.ones(len(s1)), g1
        for k in range(3):
            for face in (-h[k], h[k]):
                t = (face - a[k]) / d[k]
                ok = (0.0 < t) & (t < 1.0)
                q = [a[j] + t * d[j] for j in range(3)]
                f, e = _F(q, h)
                g = _G(q, e, d)
                cand(ok, t, f)
                lo = ok & (g < 0.0) & (t > tl)
                hi = ok & (g >= 0.0) & (t < tr)
                tl, gl = np.where(lo, t, tl), np.where(lo, g, gl)
                tr, gr = np.where(hi, t, tr), np.where(hi, g, gr)
        ts = tl + (tr - tl) * ((-gl) / (gr - gl))
        q = [a[j] + ts * d[j] for j in range(3)]
        cand((g0 < 0.0) & (0.0 < g1), ts, _F(q, h)[0])
    return best, tb


def finite_edges(s1, s2):
    return np.isfinite(s1).all(axis=1) & np.isfinite(s2).all(axis=1)


def matrices(obbs, s1, s2):
    """((n, n_obb) d2_i, (n, n_obb) t_i): +inf / -1.0 in the columns of filling OBBs and in the
    rows of non-finite edges."""
    s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3)
    s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3)
    d2, t = np.full((len(s1), len(obbs)), np.inf), np.full((len(s1), len(obbs)), -1.0)
    fin = np.flatnonzero(finite_edges(s1, s2))
    for i, o in enumerate(obbs):
        if not o["filling"] and len(fin):
            d2[fin, i], t[fin, i] = obb_d2(o, s1[fin], s2[fin])
    return d2, t


def edges(obbs, s1, s2):
    """(d2, t, nearest) per edge: the lowest index attaining the minimum; (+inf, -1.0, -1)."""
    d2, t = matrices(obbs, s1, s2)
    best, idx = cr.reduce_min(d2)
    tb = np.where(idx >= 0, t[np.arange(len(t)), np.maximum(idx, 0)], -1.0) if d2.shape[1] else np.full(len(d2), -1.0)
    return best, tb, idx


def dist(d2):
    return np.sqrt(d2)


def chords_min(d, t, near, time):
    """(clearance, chord, t, time, nearest) of one track from its chords' (dist, t, nearest)
    and its rows' time column: the earliest chord that attains the minimum distance, and
    time = t_j + t * (t_j+1 - t_j); (+inf, -1, -1.0, -1.0, -1) without a finite one."""
    if len(d) == 0 or not np.isfinite(d).any():
        return np.inf, -1, -1.0, -1.0, -1
    j = int(np.argmin(np.where(np.isnan(d), np.inf, d)))
    return float(d[j]), j, float(t[j]), float(time[j] + t[j] * (time[j + 1] - time[j])), int(near[j])


def tracks(obbs, rows):
    """The five outputs over the tracks; rows: per track (positions R x 3, time column R)."""
    out = []
    for xyz, time in rows:
        if len(xyz) < 2:
            out.append((np.inf, -1, -1.0, -1.0, -1))
            continue
        d2, t, near = edges(obbs, xyz[:-1], xyz[1:])
        out.append(chords_min(dist(d2), t, near, time))
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]), np.array([o[4] for o in out], np.int32))


# ---- the independent truth ---------------------------------------------------------------------
def truth(obbs, s1, s2, iters=200):
    """min over the collision OBBs and over t in [0, 1] of the squared distance from s + t (e - s)
    to the box (as the OBB's own c, s map it), by ternary search in long double.  +inf without
    a collision OBB; finite edges only."""
    L = np.longdouble
    s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3).astype(L)
    s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3).astype(L)
    best = np.full(len(s1), np.inf, L)
    third = L(1) / L(3)
    for o in obbs:
        if o["filling"]:
            continue
        c, s = L(float(o["rot"][0])), L(float(o["rot"][3]))
        ctr = [L(float(v)) for v in o["center"]]
        h = [L(float(v)) for v in o["half"]]

        def local(p):
            dx, dy, dz = p[:, 0] - ctr[0], p[:, 1] - ctr[1], p[:, 2] - ctr[2]
            return [c * dx + s * dy, c * dy - s * dx, dz]

        a, b = local(s1), local(s2)

        def f(t):
            out = np.zeros(len(s1), L)
            for k in range(3):
                e = np.maximum(np.abs(a[k] + t * (b[k] - a[k])) - h[k], L(0))
                out = out + e * e
            return out

        lo, hi = np.zeros(len(s1), L), np.ones(len(s1), L)
        for _ in range(iters):
            m1 = lo + (hi - lo) * third
            m2 = hi - (hi - lo) * third
            left = f(m1) <= f(m2)
            hi = np.where(left, m2, hi)
            lo = np.where(left, lo, m1)
        best = np.minimum(best, np.minimum(np.minimum(f(lo), f(hi)), np.minimum(f(np.zeros(len(s1), L)),
                                                                                  f(np.ones(len(s1), L)))))
    return best
