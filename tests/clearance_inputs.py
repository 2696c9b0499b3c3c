"""Inputs of the clearance tests (test_gpu_clearance.py) and of the CPU test of those inputs
(test_clearance_inputs_cpu.py): worlds, state sets and tracks, and what each case claims.

Worlds, under configs/config_filling.json (6 OBBs per gate, one of them filling; 1 per
obstacle): 1 OBB (trajsweep_inputs' pole), 2, 72, 300 and 1100 OBBs, the first T and T + 1 of
the 1100 (T = kClearTile, the kernels' LDS tile, read from csrc/clearance.h), and a world whose
three OBBs are all marked filling.

Everything is input data: built once per process, shared, read-only.
"""
import functools
import os
import re

import numpy as np

import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi, synth

from conftest import PKG

T = int(re.search(r"kClearTile = (\d+);", open(os.path.join(PKG, "csrc", "clearance.h")).read()).group(1))
K_SEG_LDS = int(re.search(r"kTcSegLds = (\d+);", open(os.path.join(PKG, "csrc", "trajcheck.hip")).read()).group(1))
BLOCK = 256  # k_states_clearance's workgroup

WORLDS = ("1", "filling", "2", "72", "300", "1100", "T", "T+1")
STATE_COUNTS = (1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1)
MANY = 100_000
MANY_WORLDS = ("72", "T+1")  # one tile and the tile loop at 100,000 states
DT = 0.1       # the edge tracks
FIT_DT = 0.1   # the fitted tracks against the restatement


@functools.lru_cache(maxsize=None)
def obbs(name):
    fgeom, _, _ = spi.setup()
    if name == "1":
        o = tsi.thin_obbs()
    elif name == "filling":
        o = spi.world(3)[0].copy()
        o["filling"] = 1
    elif name in ("2", "72"):
        o = spi.world(int(name))[0].copy()
    elif name == "300":
        o = capi.build_obbs(fgeom, *synth.track_world(7, n_gates=8, n_obstacles=252))
    elif name == "1100":
        o = capi.build_obbs(fgeom, *synth.track_world(1600, n_gates=8, n_obstacles=1052))
    else:
        o = obbs("1100")[:T + (name == "T+1")].copy()
    assert len(o) == {"1": 1, "filling": 3, "2": 2, "72": 72, "300": 300, "1100": 1100, "T": T, "T+1": T + 1}[name]
    o.setflags(write=False)
    return o


def _to_world(o, l):
    c, s = o["rot"][0], o["rot"][3]
    return o["center"] + np.array([c * l[0] - s * l[1], s * l[0] + c * l[1], l[2]])


@functools.lru_cache(maxsize=None)
def points(name, n):
    """n states: in the first BLOCK + 1, points inside boxes, on faces, beyond corners, 50 m
    outside everything, NaN / inf rows and random ones, shuffled; random ones after that."""
    ob = obbs(name)
    rs = np.random.RandomState(4000 + len(ob))
    sp = []
    for k in range(24):
        o = ob[(k * 37) % len(ob)]
        h = o["half"]
        sp += [o["center"].copy(),                                     # inside
               _to_world(o, [0.5 * h[0], -0.25 * h[1], 0.5 * h[2]]),   # inside, off centre
               _to_world(o, [h[0], 0.0, 0.0]),                         # on a face
               _to_world(o, [h[0] + 0.3, h[1] + 0.2, h[2] + 0.1]),     # beyond a corner
               _to_world(o, [0.0, -h[1] - 0.25, 0.0])]                 # off a face
    sp += [np.array([50.0, 50.0, 50.0]), np.array([-50.0, 3.0, 1.0]), np.array([0.0, 0.0, -50.0]),
           np.array([np.nan, 0.0, 1.0]), np.array([0.0, np.nan, 1.0]), np.array([1.0, 1.0, np.nan]),
           np.array([np.inf, 0.0, 1.0]), np.array([0.0, -np.inf, 1.0])]
    base = np.vstack([np.array(sp), synth.sample_states(900 + len(ob), *synth.C2_BOUNDS, BLOCK + 1 - len(sp))])
    base = base[rs.permutation(len(base))]
    assert len(base) == BLOCK + 1
    if n > len(base):
        base = np.vstack([base, synth.sample_states(901 + len(ob), *synth.C2_BOUNDS, n - len(base))])
    out = np.ascontiguousarray(base[:n])
    out.setflags(write=False)
    return out


# ---- straight tracks past the pole of the 1-OBB world ------------------------------------------
def line(p0, v, n_seg=1, T0=0.0):
    """Coefficients of p = p0 + v t; n_seg > 1: further segments that continue the line, each
    starting T0 after the one before."""
    p0, v = np.asarray(p0, float), np.asarray(v, float)
    c = np.zeros((n_seg, 3, 10))
    for s in range(n_seg):
        c[s, :, 0] = p0 + v * (T0 * s)
        c[s, :, 1] = v
    return c


def last_box_track(name):
    """(T, C): one segment that starts 0.02 m off a face of the world's LAST box and leaves
    along its local x at 0.5 m/s: row 0 is the closest, and its nearest OBB is the last one --
    for the T + 1 world the only entry of the second tile."""
    o = obbs(name)[-1]
    c, s = o["rot"][0], o["rot"][3]
    return np.array([1.0]), line(_to_world(o, [o["half"][0] + 0.02, 0.0, 0.0]), 0.5 * np.array([c, s, 0.0]))


V = 8.0
STEP = V * DT
SIDE = 0.5  # the passing tracks fly this far beside the pole's face


def _pole():
    return obbs("1")[0]


def _past(J, R, n_seg=1, T0=0.0):
    """R rows (one segment) along the pole's local x, SIDE beside its face; row J lies 0.05 m
    past the pole's centre plane, so it is the closest by far (its neighbours: 0.75 / 0.85 m)."""
    o = _pole()
    c, s = o["rot"][0], o["rot"][3]
    d = np.array([c, s, 0.0])
    p0 = _to_world(o, [0.05 - J * STEP, o["half"][1] + SIDE, 0.0])
    T = np.array([(R - 0.5) * DT]) if n_seg == 1 else np.full(n_seg, T0)
    return T, line(p0, V * d, n_seg, T0)


@functools.lru_cache(maxsize=None)
def edge_tracks():
    """(names, Ts, Cs, want row, want zero clearance): the closest row at each edge of the
    walk's bookkeeping (64 checking lanes, kRowChunk = 512 rows per half of the double buffer),
    tracks of exactly 1, 2, 512 and 513 rows, tracks without rows, more than kTcSegLds segments,
    a resting track and one that enters the pole."""
    o = _pole()
    c, s = o["rot"][0], o["rot"][3]
    cases = [
        ("row 0", *_past(0, 20), 0, False),
        ("row R-1", *_past(19, 20), 19, False),
        ("row 63", *_past(63, 100), 63, False),
        ("row 64", *_past(64, 100), 64, False),
        ("row 511", *_past(511, 530), 511, False),
        ("row 512", *_past(512, 530), 512, False),
        ("row 513", *_past(513, 530), 513, False),
        ("row 1023", *_past(1023, 1040), 1023, False),
        ("row 1024", *_past(1024, 1040), 1024, False),
        # rows 0..5 in segment 0 (5.5 DT long), row 6 half a step into segment 1
        ("segment boundary, row 5", *_past(5, 0, 2, 5.5 * DT), 5, False),
        ("segment boundary, row 6", *_past(6, 0, 2, 5.5 * DT), 6, False),
        ("1 row", *_past(0, 1), 0, False),
        ("2 rows", *_past(1, 2), 1, False),
        ("512 rows", *_past(300, 512), 300, False),
        ("513 rows", *_past(512, 513), 512, False),
        ("one waypoint", np.zeros(0), np.zeros((0, 3, 10)), -1, False),
        ("NaN times", np.full(2, np.nan), np.full((2, 3, 10), np.nan), -1, False),
        (f"{K_SEG_LDS + 1} segments", *_past(200, 0, K_SEG_LDS + 1, 5.5 * DT), 200, False),
        ("resting", np.array([2.0]), line(_to_world(o, [0.3, o["half"][1] + SIDE, 0.1]), [0.0, 0.0, 0.0]), 0, False),
        # 0.02 m per row along the local x through the centre: row 5 is 0.01 m outside, row 6 inside
        ("enters the pole", np.array([3.0]),
         line(_to_world(o, [-o["half"][0] - 0.11, 0.0, 0.0]), 0.2 * np.array([c, s, 0.0])), 6, True),
    ]
    names = [x[0] for x in cases]
    return names, [x[1] for x in cases], [x[2] for x in cases], [x[3] for x in cases], [x[4] for x in cases]


EDGE_ROWS = {"1 row": 1, "2 rows": 2, "512 rows": 512, "513 rows": 513, "one waypoint": 0, "NaN times": 0,
             "resting": 20}
