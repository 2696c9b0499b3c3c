"""Inputs of the edge-clearance tests (test_gpu_edge_clearance.py, test_edge_clearance_cpu.py):
worlds, seeded edge sets and tracks, and what each case claims.

Worlds, under configs/config_filling.json: none ("0": no OBB at all), clearance_inputs' three
filling OBBs, its single pole ("1"), and the first T - 1, T and T + 1 OBBs of its 1100-OBB synth
world (T = kClearTile, the LDS tile of k_motions_clearance and k_traj_chord_clearance, read
from csrc/clearance.h), and the 72-OBB track world the sibling tests use.

An edge set's first BLOCK + 1 edges hold, shuffled: per target box an endpoint inside it, an
edge through it with both ends outside, edges parallel to each local axis beside it, edges
lying in a face plane, edges across a corner that only graze it, zero-length edges inside and
outside, edges aimed at the last entry of the first tile and the first of the next; edges far
from everything; edges with a NaN or infinite coordinate; random edges.  Random edges after that.

Everything is input data: built once per process, shared, read-only.
"""
import functools

import numpy as np

import clearance_inputs as ci
import edge_clearance_ref as er
import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi, synth

T = ci.T
K_SEG_LDS = ci.K_SEG_LDS
K_ROW_CHUNK = 512  # traj_sample.h: kRowChunk, the rows per half of the walker's double buffer
BLOCK = 256        # k_motions_clearance's workgroup

WORLDS = ("0", "filling", "1", "T-1", "T", "T+1")
EDGE_COUNTS = (0, 1, 63, 64, 65, BLOCK, BLOCK + 1)
N_BAD = 6  # the non-finite edges of a set


@functools.lru_cache(maxsize=None)
def obbs(name):
    if name == "0":
        o = ci.obbs("1")[:0].copy()
    elif name in ("T-1", "T", "T+1"):
        o = ci.obbs("1100")[:T + {"T-1": -1, "T": 0, "T+1": 1}[name]].copy()
    else:
        return ci.obbs(name)
    o.setflags(write=False)
    return o


def _crafted(ob):
    s, e = [], []

    def add(o, a, b):
        s.append(ci._to_world(o, a))
        e.append(ci._to_world(o, b))

    n = len(ob)
    real = [i for i in range(n) if not ob[i]["filling"]]
    targets = sorted({real[(k * 37) % len(real)] for k in range(8)} | {i for i in (T - 1, T) if i < n}) if real else []
    for i in targets:
        o = ob[i]
        h = o["half"]
        add(o, [0.3 * h[0], -0.2 * h[1], 0.1 * h[2]], [h[0] + 0.5, 0.2, 0.1])          # the start inside
        add(o, [-h[0] - 0.4, 0.3, 0.2], [0.0, 0.0, 0.0])                              # the end inside
        add(o, [h[0] + 0.4, 0.01, 0.02], [-h[0] - 0.3, -0.01, 0.0])                   # through, ends outside
        add(o, [-h[0] - 0.5, h[1] + 0.25, 0.1], [h[0] + 0.7, h[1] + 0.25, 0.1])       # parallel to local x
        add(o, [h[0] + 0.15, -h[1] - 0.6, 0.0], [h[0] + 0.15, h[1] + 0.3, 0.0])       # parallel to local y
        add(o, [h[0] + 0.2, h[1] + 0.1, -h[2] - 0.5], [h[0] + 0.2, h[1] + 0.1, h[2] + 0.5])  # parallel to z
        add(o, [h[0], -h[1] - 0.4, 0.1], [h[0], h[1] + 0.6, -0.1])                    # in the face plane x = +h
        add(o, [-h[0] - 0.3, 0.2, h[2]], [h[0] + 0.5, -0.1, h[2]])                    # in the face plane z = +h
        add(o, [h[0] + 0.3, h[1] - 0.3, 0.0], [h[0] - 0.3, h[1] + 0.3, 0.0])          # grazes the corner edge
        add(o, [h[0] + 0.35, h[1] - 0.3, 0.1], [h[0] - 0.3, h[1] + 0.35, 0.2])        # passes 0.035 m off it
        add(o, [h[0] + 0.6, h[1] + 0.2, h[2] + 0.3], [h[0] + 0.1, h[1] + 0.7, h[2] + 0.2])  # beyond a vertex
    for i in targets[:3]:
        o = ob[i]
        add(o, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])                                      # zero length, inside
        p = [o["half"][0] + 0.4, 0.1, 0.0]
        add(o, p, p)                                                                  # zero length, outside
    s, e = [np.asarray(x) for x in s], [np.asarray(x) for x in e]
    far = [([50.0, 50.0, 50.0], [51.0, 50.5, 50.0]), ([-50.0, 3.0, 1.0], [-50.0, 3.0, 2.0]),
           ([0.0, 0.0, -50.0], [0.5, 0.5, -50.0])]
    bad = [([np.nan, 0.0, 1.0], [1.0, 0.0, 1.0]), ([0.0, 0.0, 1.0], [1.0, np.nan, 1.0]),
           ([0.0, 0.0, np.nan], [0.0, 0.0, np.nan]), ([np.inf, 0.0, 1.0], [1.0, 0.0, 1.0]),
           ([0.0, 0.0, 1.0], [1.0, -np.inf, 1.0]), ([0.5, 0.5, 0.5], [np.nan, np.nan, np.nan])]
    assert len(bad) == N_BAD
    for a, b in far + bad:
        s.append(np.array(a))
        e.append(np.array(b))
    return np.array(s), np.array(e)


@functools.lru_cache(maxsize=None)
def edges(name, n):
    """(s1, s2): n edges of the world's set."""
    ob = obbs(name)
    rs = np.random.RandomState(6000 + len(ob))
    cs, ce = _crafted(ob)
    assert len(cs) <= BLOCK + 1 - 32
    r1, r2 = synth.edges(930 + len(ob), 940 + len(ob), *synth.C2_BOUNDS, BLOCK + 1 - len(cs), max_len=1.5)
    p = rs.permutation(BLOCK + 1)
    s1, s2 = np.vstack([cs, r1])[p], np.vstack([ce, r2])[p]
    if n > BLOCK + 1:
        r1, r2 = synth.edges(931 + len(ob), 941 + len(ob), *synth.C2_BOUNDS, n - (BLOCK + 1), max_len=1.5)
        s1, s2 = np.vstack([s1, r1]), np.vstack([s2, r2])
    s1, s2 = np.ascontiguousarray(s1[:n]).reshape(-1, 3), np.ascontiguousarray(s2[:n]).reshape(-1, 3)
    s1.setflags(write=False)
    s2.setflags(write=False)
    return s1, s2


@functools.lru_cache(maxsize=None)
def expected(name, n):
    """The restatement's (d2, t, nearest) of edges(name, n): computed once, shared, read-only."""
    out = er.edges(obbs(name), *edges(name, n))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the hand cases of the CPU test: one axis-aligned box at the origin ------------------------
def unit_box(half=(0.5, 0.25, 1.0), filling=0):
    o = np.zeros(1, capi.OBB_DTYPE)
    o["half"][0] = half
    o["rot"][0] = np.eye(3).ravel()
    o["filling"] = filling
    return o


# ---- tracks --------------------------------------------------------------------------------------
DT = tsi.DT
V = tsi.V
STEP = tsi.STEP
SIDE = 0.3  # the passing tracks fly this far beside the pole's face


def _pole():
    return obbs("1")[0]


def _beside(J, R, n_seg=1, T0=0.0):
    """R rows (one segment, or n_seg of T0 each) along the pole's local x, SIDE beside its +y
    face, at V: rows J and J + 1 lie 0.3 and 0.5 m on either side of the pole's centre plane,
    so chord J passes the pole at SIDE (t = 3/8) and every row stays at least 0.3 m along x
    beyond the face: farther than SIDE."""
    o = _pole()
    c, s = o["rot"][0], o["rot"][3]
    p0 = ci._to_world(o, [-0.3 - J * STEP, o["half"][1] + SIDE, 0.0])
    T = np.array([(R - 0.5) * DT]) if n_seg == 1 else np.full(n_seg, T0)
    return T, ci.line(p0, V * np.array([c, s, 0.0]), n_seg, T0)


def bar_track():
    """A track across the pole ("a bar between two rows"): along the pole's local x through its
    centre line, rows 10 and 11 half a step (0.4 m) before and behind the centre plane.  Chord
    10 passes through the box (distance 0); no row is closer than 0.4 m - half[0]."""
    o = _pole()
    c, s = o["rot"][0], o["rot"][3]
    p0 = ci._to_world(o, [-10.5 * STEP, 0.0, 0.0])
    return np.array([19.5 * DT]), ci.line(p0, V * np.array([c, s, 0.0]))


@functools.lru_cache(maxsize=None)
def edge_tracks():
    """(names, Ts, Cs, want chord): the closest chord at each edge of the walk's bookkeeping
    (64 checking lanes with ceil(cnt / 64) consecutive samples each, kRowChunk = 512 rows per
    half of the double buffer), tracks of one waypoint, exactly one, two and 513 rows, of 1, 2,
    kTcSegLds and kTcSegLds + 1 segments, and the NaN times of a failed fit."""
    seg = 5.5 * DT  # rows 0..5 in segment 0, row 6 half a step into segment 1
    cases = [
        ("chord 0", *_beside(0, 20), 0),
        ("last chord", *_beside(18, 20), 18),
        ("lane group edge 7|8", *_beside(7, 530), 7),
        ("inside a lane's group 3|4", *_beside(3, 530), 3),
        (f"chunk boundary {K_ROW_CHUNK - 1}|{K_ROW_CHUNK}", *_beside(K_ROW_CHUNK - 1, 530), K_ROW_CHUNK - 1),
        ("first chord of the second chunk", *_beside(K_ROW_CHUNK, 530), K_ROW_CHUNK),
        ("chunk boundary 1023|1024", *_beside(1023, 1040), 1023),
        ("one waypoint", np.zeros(0), np.zeros((0, 3, 10)), -1),
        ("1 row", *_beside(0, 1), -1),
        ("2 rows", *_beside(0, 2), 0),
        ("513 rows, last chord", *_beside(K_ROW_CHUNK - 1, K_ROW_CHUNK + 1), K_ROW_CHUNK - 1),
        ("2 segments", *_beside(5, 0, 2, seg), 5),
        (f"{K_SEG_LDS} segments", *_beside(150, 0, K_SEG_LDS, seg), 150),
        (f"{K_SEG_LDS + 1} segments", *_beside(200, 0, K_SEG_LDS + 1, seg), 200),
        ("NaN times", np.full(2, np.nan), np.full((2, 3, 10), np.nan), -1),
        ("across the pole", *bar_track(), 10),
    ]
    return [x[0] for x in cases], [x[1] for x in cases], [x[2] for x in cases], [x[3] for x in cases]
