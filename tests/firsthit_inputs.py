"""Inputs of the first-hit tests (test_gpu_firsthit.py) and of the CPU test of those inputs
(test_firsthit_inputs_cpu.py): worlds and crafted edge sets, and what each set claims to hold.

Worlds: clearance_inputs' 1, 3 (all filling), 2, 72, 300 and 1100 OBBs under
configs/config_filling.json, and the first T and T + 1 of the 1100 (T = kHitTile, the LDS tile
of k_motions_first_hit, read from csrc/first_hit.h).

An edge set's first BLOCK + 1 edges hold, shuffled: starts inside a box; end-only hits through
the |d| < 1e-6 parallel branch (the start 5e-7 outside an inflated face, the end 4e-7 inside
it); hits with 0 < t < 1; misses that pass the AABB prefilter (across a corner) and misses
that fail it (50 m away); zero-length edges inside and outside a box; edges through the
filling boxes (the gate openings) along their thin axis, through the centre and beside a bar;
starts inside two overlapping inflated boxes (ties at t = 0); hits aimed at the last record of
the first tile and the first record of the next; random edges.  Random edges after that.

Everything is input data: built once per process, shared, read-only.
"""
import functools
import os
import re

import numpy as np

import clearance_inputs as ci
import firsthit_ref as fr
import small_path_inputs as spi
from eppamd import synth

from conftest import PKG

T = int(re.search(r"kHitTile = (\d+);", open(os.path.join(PKG, "csrc", "first_hit.h")).read()).group(1))
BLOCK = 256  # k_motions_first_hit's workgroup

WORLDS = ("1", "filling", "2", "72", "300", "1100", "T", "T+1")
EDGE_COUNTS = (1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1)
MANY = 100_000
MANY_WORLDS = ("72", "T+1")  # one tile and the tile loop at 100,000 edges
CAN_PASS = (False, True)
HAS_GATES = ("72", "300", "1100", "T", "T+1")  # worlds with gates: filling openings, bars that touch


@functools.lru_cache(maxsize=None)
def obbs(name):
    if name in ("T", "T+1"):
        o = ci.obbs("1100")[:T + (name == "T+1")].copy()
        o.setflags(write=False)
        return o
    return ci.obbs(name)


@functools.lru_cache(maxsize=None)
def ref_world(name):
    """The restatement's world (dicts with the inflated AABBs)."""
    _, rg, ro = spi.setup()
    return fr.world(obbs(name), rg, ro)


def _radius(o):
    _, rg, ro = spi.setup()
    return rg if o["is_gate"] else ro


def _crafted(name):
    ob = obbs(name)
    n = len(ob)
    s, e = [], []

    def add(a, b):
        s.append(np.asarray(a, float))
        e.append(np.asarray(b, float))

    targets = sorted({(k * 37) % n for k in range(12)} | {i for i in (T - 1, T) if i < n})
    for i in targets:
        o = ob[i]
        r = _radius(o)
        H = o["half"] + r  # the inflated half sizes (the slab test's, always)
        add(o["center"], ci._to_world(o, [H[0] + 0.6, 0.1, 0.0]))                            # start inside
        add(ci._to_world(o, [-(H[0] + 0.3), 0.0, 0.0]), o["center"])                         # 0 < t < 1
        add(ci._to_world(o, [H[0] + 0.4, 0.01, 0.02]), ci._to_world(o, [-(H[0] + 0.4), -0.01, 0.0]))   # through
        if not o["filling"]:
            add(ci._to_world(o, [H[0] + 5e-7, 0.0, 0.0]), ci._to_world(o, [H[0] - 4e-7, 0.0, 0.0]))    # end-only
        d = 0.05                                                                             # across a corner: a miss
        add(ci._to_world(o, [H[0] + 3 * d, H[1] - d, 0.0]), ci._to_world(o, [H[0] - d, H[1] + 3 * d, 0.0]))
        if o["filling"]:  # (its AABB is not inflated: a longer diagonal, whose box reaches it)
            L = H[0] + H[1] + 2 * d + 0.3
            add(ci._to_world(o, [L, -0.3, 0.0]), ci._to_world(o, [-0.3, L, 0.0]))
    for i in (T - 1, T):                                                                     # the tile's edge, from
        if i < n:                                                                            # every side
            o = ob[i]
            H = o["half"] + _radius(o)
            for k in range(3):
                for sg in (-1.0, 1.0):
                    u = np.zeros(3)
                    u[k] = sg * (H[k] + 0.3)
                    add(ci._to_world(o, u), o["center"])
    for i in targets[:4]:
        o = ob[i]
        add(o["center"], o["center"])                                                        # zero length, inside
        p = ci._to_world(o, [o["half"][0] + _radius(o) + 0.4, 0.0, 0.0])
        add(p, p)                                                                            # zero length, outside
    add([50.0, 50.0, 50.0], [51.0, 50.5, 50.0])                                              # far from everything
    add([-50.0, 3.0, 1.0], [-50.0, 3.0, 2.0])
    add([0.0, 0.0, -50.0], [0.5, 0.5, -50.0])
    add([60.0, -60.0, 1.0], [60.0, -60.0, 1.0])
    for i in np.flatnonzero(ob["filling"])[:4]:                                              # through the filling boxes
        o = ob[i]
        k = int(np.argmin(o["half"][:2]))  # the thin axis: the opening's normal
        j = 1 - k
        u, v = np.zeros(3), np.zeros(3)
        u[k], v[j] = o["half"][k] + 0.4, o["half"][j] - 0.01
        add(ci._to_world(o, -u), ci._to_world(o, u))            # through the centre
        add(ci._to_world(o, v - u), ci._to_world(o, v + u))     # beside the bar
    w = ref_world(name)
    _, rg, ro = spi.setup()
    pairs = 0
    for i in range(n - 1):                                                                   # starts inside two boxes
        if pairs == 4:
            break
        for j in range(i + 1, min(i + 6, n)):
            if ob[i]["filling"] or ob[j]["filling"]:
                continue
            p = 0.5 * (ob[i]["center"] + ob[j]["center"])
            if fr.P.point_hit(w[i], list(p), _radius(ob[i])) and fr.P.point_hit(w[j], list(p), _radius(ob[j])):
                add(p, p + np.array([0.3, 0.2, 0.1]))
                pairs += 1
                break
    return np.array(s), np.array(e)


@functools.lru_cache(maxsize=None)
def edges(name, n):
    """(s1, s2): n edges of the world's set."""
    ob = obbs(name)
    rs = np.random.RandomState(5000 + len(ob))
    cs, ce = _crafted(name)
    assert len(cs) <= BLOCK + 1 - 32
    r1, r2 = synth.edges(910 + len(ob), 920 + len(ob), *synth.C2_BOUNDS, BLOCK + 1 - len(cs), max_len=1.5)
    p = rs.permutation(BLOCK + 1)
    s1, s2 = np.vstack([cs, r1])[p], np.vstack([ce, r2])[p]
    if n > BLOCK + 1:
        r1, r2 = synth.edges(911 + len(ob), 921 + len(ob), *synth.C2_BOUNDS, n - (BLOCK + 1), max_len=1.5)
        s1, s2 = np.vstack([s1, r1]), np.vstack([s2, r2])
    s1, s2 = np.ascontiguousarray(s1[:n]), np.ascontiguousarray(s2[:n])
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


@functools.lru_cache(maxsize=None)
def expected(name, n, can_pass):
    """The restatement's (t_hit, obb) of edges(name, n): computed once, shared, read-only."""
    _, rg, ro = spi.setup()
    t, o = fr.edges(ref_world(name), rg, ro, *edges(name, n), can_pass)
    t.setflags(write=False)
    o.setflags(write=False)
    return t, o
