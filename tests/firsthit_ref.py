"""CPU restatement of "first hit" (include/epp.h: epp_motions_first_hit,
epp_traj_first_hit_batch): where along a straight edge s -> e the world first blocks it, and
which OBB does.  Python floats and numpy float64 are IEEE doubles and neither fuses a
multiply-add, so every operation is one IEEE multiply, add, subtract or divide in the
definition's association.

The candidates are the OBBs World::checkRayValid tests (pyref_obb.ray_valid, lines 79-85): the
closed overlap of the OBB's stored inflated AABB with the edge's bounding box, filling OBBs
skipped when can_pass.  Per candidate, pyref_obb.ray_hit extended to keep its sub-answers:

    start_hit, end_hit   the endpoint tests (inflated iff the OBB is not filling)
    slab_hit             the final predicate on tMin / tMax after the three axes
    t_i = 0.0 if start_hit, else tMin if slab_hit, else 1.0 if end_hit, else none

and the edge's answer is (min_i t_i, the lowest i that attains it), (+inf, -1) when nothing
blocks.  Two forms: a scalar one (first_hit: a plain transcription, for hand values and as a
cross-check) and a numpy one over all edges at once (edges / matrices: what the GPU tests
compare against); test_firsthit_inputs_cpu.py holds them equal on the crafted inputs.
"""
import numpy as np

import pyref_obb as P

_SX = (-1, 1, 1, -1, -1, 1, 1, -1)
_SY = (-1, -1, 1, 1, -1, -1, 1, 1)
_SZ = (-1, -1, -1, -1, 1, 1, 1, 1)


def world(obbs, rg, ro):
    """capi OBB records -> pyref_obb's dicts, with the inflated AABB of OBB::getAABB
    (src/OBB.cpp:93-123; pyref_obb.build's corner loop): the doubles the device records hold."""
    out = []
    for o in obbs:
        R = [float(v) for v in o["rot"]]
        ctr, half = [float(v) for v in o["center"]], [float(v) for v in o["half"]]
        lo, hi = [0.0] * 3, [0.0] * 3
        for j in range(8):
            cr = [_SX[j] * half[0], _SY[j] * half[1], _SZ[j] * half[2]]
            for i in range(3):
                v = ((R[3 * i] * cr[0] + R[3 * i + 1] * cr[1]) + R[3 * i + 2] * cr[2]) + ctr[i]
                lo[i] = v if j == 0 else min(lo[i], v)
                hi[i] = v if j == 0 else max(hi[i], v)
        if not o["filling"]:
            infl = rg if o["is_gate"] else ro
            lo = [x - infl for x in lo]
            hi = [x + infl for x in hi]
        out.append({"center": ctr, "half": half, "rot": R, "filling": bool(o["filling"]), "is_gate": bool(o["is_gate"]),
                    "aabb_lo": lo, "aabb_hi": hi})
    return out


# ---- scalar ------------------------------------------------------------------------------------
def slab(o, s, e, inflate):
    """pyref_obb.ray_hit's axis loop: tMin if the final predicate holds (slab_hit), else None."""
    ls, le = P._local(o, s), P._local(o, e)
    ld = [le[i] - ls[i] for i in range(3)]
    tmin, tmax = 0.0, 1.0
    for i in range(3):
        ih = o["half"][i] + inflate
        bmin, bmax = -ih, ih
        if abs(ld[i]) < 1e-6:
            if ls[i] < bmin or ls[i] > bmax:
                return None
        else:
            inv = 1.0 / ld[i]
            t1 = (bmin - ls[i]) * inv
            t2 = (bmax - ls[i]) * inv
            te = t2 if t2 < t1 else t1
            tx = t2 if t1 < t2 else t1
            tmin = te if tmin < te else tmin
            tmax = tx if tx < tmax else tmax
            if tmin > tmax:
                return None
    return tmin if (0 <= tmin <= 1 and 0 <= tmax <= 1) else None


def entry(o, s, e, inflate):
    """t_i of one OBB, None when it does not block the edge."""
    if P.point_hit(o, s, inflate):
        return 0.0
    t = slab(o, s, e, inflate)
    if t is not None:
        return t
    return 1.0 if P.point_hit(o, e, inflate) else None


def first_hit(w, rg, ro, s, e, can_pass):
    """(t_hit, obb) of one edge over the world w (dicts): pyref_obb.ray_valid's loop with a
    strict < minimum in place of the early return."""
    lo = [min(s[i], e[i]) for i in range(3)]
    hi = [max(s[i], e[i]) for i in range(3)]
    best, obb = float("inf"), -1
    for i, o in enumerate(w):
        if any(o["aabb_hi"][k] < lo[k] or hi[k] < o["aabb_lo"][k] for k in range(3)):
            continue
        if o["filling"] and can_pass:
            continue
        t = entry(o, s, e, rg if o["is_gate"] else ro)
        if t is not None and t < best:
            best, obb = t, i
    return best, obb


# ---- numpy, all edges at once --------------------------------------------------------------------
def _parts(o, r, s, e):
    """(start_hit, slab_hit, end_hit, tMin) of OBB o for the edges s -> e (k x 3 each)."""
    c, sn = o["rot"][0], o["rot"][3]
    ctr, half = o["center"], o["half"]
    with np.errstate(all="ignore"):
        dx, dy, dz = s[:, 0] - ctr[0], s[:, 1] - ctr[1], s[:, 2] - ctr[2]
        ls = [c * dx + sn * dy, c * dy - sn * dx, dz]
        ex, ey, ez = e[:, 0] - ctr[0], e[:, 1] - ctr[1], e[:, 2] - ctr[2]
        le = [c * ex + sn * ey, c * ey - sn * ex, ez]
        ph = [h if o["filling"] else h + r for h in half]
        start = (np.abs(ls[0]) <= ph[0]) & (np.abs(ls[1]) <= ph[1]) & (np.abs(ls[2]) <= ph[2])
        end = (np.abs(le[0]) <= ph[0]) & (np.abs(le[1]) <= ph[1]) & (np.abs(le[2]) <= ph[2])
        tmin, tmax = np.zeros(len(s)), np.ones(len(s))
        rejected = np.zeros(len(s), bool)
        for k in range(3):
            ld = le[k] - ls[k]
            ih = half[k] + r
            bmin, bmax = -ih, ih
            par = np.abs(ld) < 1e-6
            outside = (ls[k] < bmin) | (ls[k] > bmax)
            inv = 1.0 / ld
            t1 = (bmin - ls[k]) * inv
            t2 = (bmax - ls[k]) * inv
            te = np.where(t2 < t1, t2, t1)
            tx = np.where(t1 < t2, t2, t1)
            nmin = np.where(tmin < te, te, tmin)
            nmax = np.where(tx < tmax, tx, tmax)
            rejected |= (par & outside) | (~par & (nmin > nmax))
            tmin = np.where(par, tmin, nmin)
            tmax = np.where(par, tmax, nmax)
        slab_hit = ~rejected & (0 <= tmin) & (tmin <= 1) & (0 <= tmax) & (tmax <= 1)
    return start, slab_hit, end, tmin


def _takes_part(o, can_pass, lo, hi):
    if o["filling"] and can_pass:
        return np.zeros(len(lo), bool)
    a, b = o["aabb_lo"], o["aabb_hi"]
    with np.errstate(invalid="ignore"):
        out = (b[0] < lo[:, 0]) | (hi[:, 0] < a[0]) | (b[1] < lo[:, 1]) | (hi[:, 1] < a[1]) | (b[2] < lo[:, 2]) | \
              (hi[:, 2] < a[2])
    return ~out


def _edges(s1, s2):
    s1 = np.ascontiguousarray(s1, np.float64).reshape(-1, 3)
    s2 = np.ascontiguousarray(s2, np.float64).reshape(-1, 3)
    # min / max as the selects of World::checkRayValid's ray box
    return s1, s2, np.where(s2 < s1, s2, s1), np.where(s1 < s2, s2, s1)


def edges(w, rg, ro, s1, s2, can_pass):
    """(t_hit float64[n], obb int32[n]) over the world w (dicts); only the edges an OBB's
    prefilter lets through are evaluated against it."""
    s1, s2, lo, hi = _edges(s1, s2)
    best, obb = np.full(len(s1), np.inf), np.full(len(s1), -1, np.int32)
    for i, o in enumerate(w):
        idx = np.flatnonzero(_takes_part(o, can_pass, lo, hi))
        if len(idx) == 0:
            continue
        start, slab_hit, end, tmin = _parts(o, rg if o["is_gate"] else ro, s1[idx], s2[idx])
        t = np.where(start, 0.0, np.where(slab_hit, tmin, np.where(end, 1.0, np.inf)))
        lt = t < best[idx]
        best[idx[lt]] = t[lt]
        obb[idx[lt]] = i
    return best, obb


def matrices(w, rg, ro, s1, s2, can_pass):
    """Every (edge, OBB) pair, for the tests of the inputs: dict of (n, n_obb) arrays part
    (takes part), start, slab, end and t (t_i, +inf where the OBB does not take part or does
    not block)."""
    s1, s2, lo, hi = _edges(s1, s2)
    n, m = len(s1), len(w)
    out = {k: np.zeros((n, m), bool) for k in ("part", "start", "slab", "end")}
    out["t"] = np.full((n, m), np.inf)
    for i, o in enumerate(w):
        part = _takes_part(o, can_pass, lo, hi)
        start, slab_hit, end, tmin = _parts(o, rg if o["is_gate"] else ro, s1, s2)
        out["part"][:, i], out["start"][:, i], out["slab"][:, i], out["end"][:, i] = part, start, slab_hit, end
        t = np.where(start, 0.0, np.where(slab_hit, tmin, np.where(end, 1.0, np.inf)))
        out["t"][:, i] = np.where(part, t, np.inf)
    return out


def reduce_min(t):
    """(min, lowest index attaining it) per row of matrices()["t"]; (+inf, -1) if none."""
    if t.shape[1] == 0:
        return np.full(len(t), np.inf), np.full(len(t), -1, np.int32)
    best = t.min(axis=1)
    idx = t.argmin(axis=1).astype(np.int32)  # (the first minimum)
    idx[np.isinf(best)] = -1
    return best, idx
