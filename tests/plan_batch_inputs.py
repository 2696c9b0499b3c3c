"""Inputs for the stage-level tests of the batched planner (tests/plan_batch_ref.py is the
reference, tests/test_plan_batch_inputs_cpu.py checks on the CPU that the inputs reach what
they claim, tests/test_gpu_plan_batch.py runs them on the device).

The world is synth.c1_world(): one gate and four obstacles in [-2, 2]^2 x [0, 2].  A case is a
batch: dict(can_pass, lo, hi, ns, k, segs), segs the caller-filled fields of PlanSeg.

Product geometry is plan_geometry (csrc/plan_geometry.h) restated in numpy; the other cases
scale its cell edge h (the first radius 1.6 h then holds ~17 rho h^3 candidates, rho the
node density), tighten gbound, collapse the sampling box to a point (every distance ties) or
shape the grid box.
"""
import functools
import re
import os

import numpy as np

import oracle as O
from eppamd import config, synth

from conftest import CONFIG, ROOT

import plan_batch_ref as R

LO, HI = synth.C1_BOUNDS
ELLIPSE = 1.25


def compact_chunk():
    """kCompactChunk (csrc/planner_common.h): the chunk of the ordered compactions."""
    src = open(os.path.join(ROOT, "efficient-path-planner_amd", "csrc", "planner_common.h")).read()
    v = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (kCompact\w+) = (\d+);", src)}
    return v["kCompactThreads"] * v["kCompactRounds"]


@functools.lru_cache(maxsize=None)
def world():
    cfg = config.load(CONFIG)
    geom = config.geometry(cfg)
    gates, obstacles, _, _ = synth.c1_world()
    rg, ro = config.inflate_radii(cfg)
    return O.world_build(geom, gates, obstacles, rg, ro), rg, ro


def device_world():
    from eppamd import capi
    cfg = config.load(CONFIG)
    geom = config.geometry(cfg)
    gates, obstacles, _, _ = synth.c1_world()
    rg, ro = config.inflate_radii(cfg)
    return capi.World(capi.build_obbs(geom, gates, obstacles), rg, ro)


def geometry(seed, s, g, ns, lo=LO, hi=HI, ellipse=ELLIPSE, h_scale=1.0, gmargin=7.5, cap=None):
    """plan_geometry for the problem (s, g) with ns samples in the box, then: h scaled by
    h_scale, gbound = bound + gmargin h, the grid box that ellipsoid's box; cap: the product's
    when None."""
    s, g = np.asarray(s, float), np.asarray(g, float)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    nmax = ns + 2
    vbox = float(np.prod(hi - lo))
    h = float(np.cbrt(1.5 * max(vbox, 1e-12) / nmax)) * h_scale
    dv = g - s
    d = float(np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]))
    bound = ellipse * d + 0.25
    gbound = bound + gmargin * h
    a = 0.5 * gbound
    b2 = max(0.0, a * a - 0.25 * d * d)
    klo, khi = np.minimum(lo, np.minimum(s, g)), np.maximum(hi, np.maximum(s, g))
    u = dv / d if d > 0 else np.zeros(3)
    e = np.sqrt(a * a * u * u + b2 * (1.0 - u * u)) * (1.0 + 1e-6) + 1e-6
    c = 0.5 * (s + g)
    if cap is None:
        vell = np.pi * bound * (bound * bound - d * d) / 6.0
        want = 1.25 * (min(1.0, vell / vbox) if vbox > 0 else 1.0) * nmax + 1024.0
        cap = int(want) if want < 0.5 * nmax else 0
    return dict(seed=seed, s=s, g=g, bound=bound, gbound=gbound, glo=np.maximum(klo, c - e), ghi=np.minimum(khi, c + e),
                h=h, cap=int(cap))


# (start, goal) pairs inside the box, on both sides of the obstacles and the gate
ENDS = [((0.0, -1.6, 0.3), (0.3, -0.5, 0.9)), ((-1.5, -0.2, 1.2), (-0.4, 0.9, 0.6)), ((1.4, 1.2, 1.5), (0.5, 0.2, 0.8)),
        ((-0.3, 1.5, 0.4), (0.9, 1.7, 1.3)), ((1.6, -1.5, 1.0), (0.4, -1.2, 0.5)), ((-1.7, 1.6, 1.6), (-1.0, 0.3, 1.1))]


CENTRAL = ((-0.5, -0.7, 1.0), (0.5, -0.6, 1.1))  # far from the box's faces: every first radius is whole


def _batch(can_pass, ns, k, segs, lo=LO, hi=HI):
    return dict(can_pass=bool(can_pass), lo=np.asarray(lo, float), hi=np.asarray(hi, float), ns=int(ns), k=int(k),
                segs=segs)


def _nq(b, q):
    """The query count of problem q in batch b (from the reference)."""
    return len(R.problem_ref(world(), b["can_pass"], b["lo"], b["hi"], b["ns"], b["k"], dict(q, cap=1))["queries"])


def _ns_for_nodes(seed, n_nodes, can_pass=False):
    """The smallest ns whose node count (valid samples + 2) is n_nodes."""
    w, rg, ro = world()
    xyz = synth.sample_states(seed, LO, HI, 2 * n_nodes)
    valid = O.check_states(w, rg, ro, xyz, can_pass).astype(bool)
    return int(np.nonzero(np.cumsum(valid) == n_nodes - 2)[0][0]) + 1


# The degenerate sampling box: every sample is this (valid) point, so the lists are runs of
# exact ties.  One end, A, lies 0.31 m beside it (0.31^2 is no bisection midpoint of
# [0, 0.4^2]); the other, B, 0.27 m below A: nearer to A than the samples are, and in the
# grid's lowest z layer, so B is the first entry of A's candidate list (cells are walked z, y,
# x) and belongs at the front of A's row -- a ranking that loses or miscounts its list's first
# entry shows there.  B's own list is empty at r = 0.4 and holds everything at the second
# radius.
POINT = np.array([0.0, -1.2, 1.0])


def _degenerate(ns, k):
    a = POINT + np.array([0.31, 0.0, 0.0])
    b = a + np.array([0.0, 0.0, -0.27])
    segs = []
    for seed, (s, g) in ((5, (b, a)), (6, (a, b))):
        q = geometry(seed, s, g, ns, cap=ns + 2)
        q["h"] = 0.25
        q["bound"] = 1.0  # every node is a query
        q["gbound"] = q["bound"] + 7.5 * q["h"]
        q["glo"], q["ghi"] = POINT - 0.35, POINT + 0.35  # 27 cells: no coarsening at ns = 40
        segs.append(q)
    return _batch(False, ns, k, segs, lo=POINT, hi=POINT)


@functools.lru_cache(maxsize=None)
def case(name):
    ns = 4000
    if name.startswith("product"):  # product_k{4,8,16}_p{0,1}
        k, cp = int(name.split("_")[1][1:]), int(name.split("_")[2][1:])
        return _batch(cp, ns, k, [geometry(101 + p + 10 * cp, *ENDS[p], ns) for p in range(3)])
    if name.startswith("scaled"):  # scaled_k{4,16}: rho h_eff^3 ~ 8, 20, 45 (up), 0.5 (down), tight gbound
        k = int(name.split("_")[1][1:])
        rho = 0.8 * ns / 32.0  # (about a fifth of the samples are invalid)
        h0 = geometry(0, *ENDS[0], ns)["h"]
        ends = [ENDS[0], ENDS[1], CENTRAL, ENDS[3]]
        segs = [geometry(201 + i, *ends[i], ns, h_scale=float(np.cbrt(t / rho)) / h0, cap=ns + 2)
                for i, t in enumerate((8.0, 20.0, 45.0, 0.5))]
        segs.append(geometry(205, *ENDS[4], ns, gmargin=2.0, cap=ns + 2))
        return _batch(False, ns, k, segs)
    if name.startswith("degenerate"):  # degenerate_{40,100,300,600}
        n = int(name.split("_")[1])
        return _degenerate(n, {40: 16, 100: 8, 300: 4, 600: 8}[n])
    if name == "grid":  # a cell edge the cell-count loop coarsens; a flat grid
        ns = 1500
        a = geometry(301, *ENDS[1], ns, h_scale=0.2, gmargin=60.0, cap=ns + 2)
        b = geometry(302, (-1.2, -1.5, 1.0), (0.2, -1.4, 1.0), ns, cap=ns + 2)
        b["glo"][2] = b["ghi"][2] = 1.0
        return _batch(True, ns, 8, [a, b])
    if name == "capacity":  # rows capped, cap == queries, cap == 0 beside cap > 0
        ns = 3000
        b = _batch(False, ns, 8, [geometry(401 + p, *ENDS[p], ns, cap=ns + 2) for p in range(4)])
        b["segs"][0]["cap"] = _nq(b, b["segs"][0]) - 37
        b["segs"][1]["cap"] = _nq(b, b["segs"][1])
        b["segs"][2]["cap"] = 0
        return b
    if name.startswith("batch"):  # batch_{1,16,17,64}: different seeds and ends, every fifth problem cap == 0
        S, ns = int(name.split("_")[1]), 500
        segs = []
        for p in range(S):
            s, g = ENDS[p % len(ENDS)]
            sh = np.array([0.01 * p, -0.005 * p, 0.002 * p])
            segs.append(geometry(501 + 7 * p, np.asarray(s) + sh, np.asarray(g) - sh, ns, cap=0 if p % 5 == 4 else ns + 2))
        return _batch(S % 2, ns, (4, 8, 16)[S % 3], segs)
    if name.startswith("samples"):  # samples_{chunk, chunk + 1, 4 chunk, 4 chunk + 1}: k_pb_compact's chunks
        ns = int(name.split("_")[1])
        return _batch(False, ns, 8, [geometry(601, *ENDS[0], ns, h_scale=1.0, cap=ns + 2)])
    if name.startswith("nodes"):  # nodes_{chunk, chunk + 1, 4 chunk, 4 chunk + 1}: k_pb_number's chunks
        ns = _ns_for_nodes(602, int(name.split("_")[1]))
        return _batch(False, ns, 8, [geometry(602, *ENDS[1], ns, gmargin=7.5, cap=ns + 2)])
    raise KeyError(name)


def case_names():
    c = compact_chunk()
    return ([f"product_k{k}_p{cp}" for k in (4, 8, 16) for cp in (0, 1)] + ["scaled_k4", "scaled_k16"] +
            [f"degenerate_{n}" for n in (40, 100, 300, 600)] + ["grid", "capacity"] +
            [f"batch_{S}" for S in (1, 16, 17, 64)] + [f"samples_{n}" for n in (c, c + 1, 4 * c, 4 * c + 1)] +
            [f"nodes_{n}" for n in (c, c + 1, 4 * c, 4 * c + 1)])


@functools.lru_cache(maxsize=None)
def reference(name):
    b = case(name)
    return R.batch_ref(world(), b["can_pass"], b["lo"], b["hi"], b["ns"], b["k"], b["segs"])


def reverse_table(n, k=16, seed=1):
    """A masked k-NN-like table (n x k, entries in [-1, n), distinct within a row): node 0 has
    in-degree 0, and about min(3000, n / 2) rows point at the hub n - 1."""
    rng = np.random.default_rng(seed + n)
    tab = np.full((n, k), -1, np.int32)
    if n > 1:
        tab = rng.integers(1, n, (n, k)).astype(np.int32)
        for j in range(1, k):  # distinct within a row
            tab[(tab[:, j:j + 1] == tab[:, :j]).any(axis=1), j] = -1
        tab[tab == np.arange(n, dtype=np.int32)[:, None]] = -1  # no self edge
        tab[tab == n - 1] = -1
        hub = rng.choice(n - 1, size=min(3000, n // 2), replace=False)
        tab[hub, rng.integers(0, k, len(hub))] = n - 1
        tab[rng.random(tab.shape) < 0.2] = -1  # the mask
    return tab
