"""Worlds and states of the point-record tests (test_point_records_cpu.py,
test_gpu_point_records.py).

The plain point test of k_states_v5 reads 128-byte point records whose thresholds
t = filling ? h : h + r are inflated by the host index build, and learns "filling" from bit
15 of the candidate-list id.  The states here sit where a wrong threshold, a wrong flag or a
wrong record would change a flag: exactly on |lx| = tx, |ly| = ty, |dz| = tz and a few ulps
to either side, on and around the AABB bounds, and inside a filling OBB within r of its
faces (invalid only if the filling box were inflated, or valid only if it were skipped).

Everything is input data and oracle output: built once per process, shared, read-only.
"""
import functools

import numpy as np

import oracle as O
from eppamd import capi, config, synth

from conftest import CONFIG
from small_path_inputs import FILLING_CONFIG, adversarial_points, gate_openings

N_EDGES = (3, 4, 255, 256, 257, 4099)
N_MAX = max(N_EDGES)
MIN_DISTANCE = 0.15
ULPS = 3  # states up to this many ulps to either side of a threshold


@functools.lru_cache(maxsize=None)
def setup(name):
    """(geometry, r_gate, r_obst): "filling" = configs/config_filling.json, "c2" = config.json."""
    cfg = config.load(FILLING_CONFIG if name == "filling" else CONFIG)
    return (config.geometry(cfg),) + tuple(config.inflate_radii(cfg))


@functools.lru_cache(maxsize=None)
def poses(name, moved=False):
    """The C2 track (synth.track_world(42)); in the filling world gate 0 and obstacle 0 stand
    unrotated (yaw 0) and every second obstacle is turned, so there is a gate frame, a filling
    opening and an obstacle of either kind.  moved: gate 2 shifted and turned (a gate-pose
    update)."""
    gates, obstacles = synth.track_world(42)
    gates, obstacles = np.array(gates, float), np.array(obstacles, float)
    if name == "filling":
        gates[0, 5] = 0.0
        obstacles[0, 5] = 0.0
        obstacles[1::2, 5] = 0.4 + 0.1 * np.arange(len(obstacles[1::2]))  # (the track's obstacles stand unrotated)
    if moved:
        gates[2, 0] += 0.15
        gates[2, 1] -= 0.1
        gates[2, 5] += 0.2
    gates.setflags(write=False)
    obstacles.setflags(write=False)
    return gates, obstacles


@functools.lru_cache(maxsize=None)
def world(name, moved=False):
    """(OBBs for capi.World, the oracle's world)."""
    geom, rg, ro = setup(name)
    gates, obstacles = poses(name, moved)
    obbs = capi.build_obbs(geom, gates, obstacles)
    ref = O.world_build(geom, gates, obstacles, rg, ro)
    assert len(obbs) == len(ref)
    obbs.setflags(write=False)
    return obbs, ref


def thresholds(obbs, rg, ro):
    """t = filling ? h : h + r, r by the owner (src/World.cpp:89-90, include/OBB.h:54-57)."""
    r = np.where(obbs["is_gate"] != 0, rg, ro)[:, None]
    return np.where((obbs["filling"] != 0)[:, None], obbs["half"], obbs["half"] + r)


def _nudged(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def threshold_points(obbs, rg, ro):
    """Per OBB and face: a state on the face of the (inflated) box and its neighbours within
    ULPS ulps along the world axis that moves the face coordinate most.  Returns (points,
    number of them for which the kernel's own arithmetic gives |l| == t exactly)."""
    t = thresholds(obbs, rg, ro)
    pts, exact = [], 0
    for o, tt in zip(obbs, t):
        c, s = o["rot"][0], o["rot"][3]
        ctr = o["center"]
        for ax in range(3):
            for sign in (-1.0, 1.0):
                l = np.array([0.3, -0.2, 0.25]) * tt
                l[ax] = sign * tt[ax]
                p = ctr + np.array([c * l[0] - s * l[1], s * l[0] + c * l[1], l[2]])
                # the world axis to nudge: z for the z faces, else the one the local axis leans on
                w = 2 if ax == 2 else (ax if abs(c) >= abs(s) else 1 - ax)
                for k in range(-ULPS, ULPS + 1):
                    q = p.copy()
                    q[w] = _nudged(p[w], k)
                    dx, dy, dz = q - ctr
                    loc = (c * dx + s * dy, c * dy - s * dx, dz)  # the kernel's evaluation
                    exact += abs(loc[ax]) == tt[ax]
                    pts.append(q)
    return np.array(pts), int(exact)


def filling_margin_points(obbs, rg, ro):
    """Inside every filling OBB within r of a face, and outside it within r of the face."""
    pts = []
    for o in obbs[obbs["filling"] != 0]:
        c, s = o["rot"][0], o["rot"][3]
        for ax in range(3):
            for sign in (-1.0, 1.0):
                for d in (-0.5 * rg, -1e-9, 1e-9, 0.5 * rg):
                    l = np.array([0.2, -0.3, 0.1]) * o["half"]
                    l[ax] = sign * (o["half"][ax] + d)
                    pts.append(o["center"] + np.array([c * l[0] - s * l[1], s * l[0] + c * l[1], l[2]]))
    return np.array(pts).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def states(name):
    """N_MAX states: threshold, AABB-bound, filling-margin and gate-opening states and uniform
    ones, shuffled, so that every prefix in N_EDGES holds boundary states."""
    geom, rg, ro = setup(name)
    gates, _ = poses(name)
    obbs, ref = world(name)
    rs = np.random.RandomState(11)
    thr, exact = threshold_points(obbs, rg, ro)
    assert exact >= 20, exact  # states exactly on a threshold exist
    parts = [thr[np.sort(rs.choice(len(thr), 1800, replace=False))],
             adversarial_points(ref)[:: 2][:700], gate_openings(gates, geom, 40, seed=9)]
    if name == "filling":
        parts.append(filling_margin_points(obbs, rg, ro))
    n_rand = N_MAX - sum(len(p) for p in parts)
    assert n_rand > 500
    parts.append(synth.sample_states(21, *synth.C2_BOUNDS, n_rand))
    pts = np.ascontiguousarray(np.vstack(parts)[rs.permutation(N_MAX)])
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def expected(name, variant, moved=False):
    """The oracle's flags of states(name); variant 0 / 1 = can_pass_gate, "md" = minDistance."""
    _, rg, ro = setup(name)
    _, ref = world(name, moved)
    pts = states(name)
    exp = (O.check_states_mindist(ref, pts, MIN_DISTANCE) if variant == "md"
           else O.check_states(ref, rg, ro, pts, bool(variant), threads=8))
    exp.setflags(write=False)
    return exp


def point_records(obbs, rg, ro):
    """The host index build's record images: (17-double records, point records in field
    order, list ids as stored, id mask)."""
    import ctypes as C
    f = capi.lib().epp_dbg_point_records
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                  C.c_void_p]
    n = len(obbs)
    obbs = np.ascontiguousarray(obbs)
    recs, pt = np.zeros((n, 17)), np.zeros((n, 16))
    ids = np.zeros(1 << 20, np.uint16)
    out = np.zeros(6, np.int64)
    capi.check(f(obbs.ctypes.data, n, rg, ro, recs.ctypes.data, pt.ctypes.data, ids.ctypes.data, len(ids),
                 out.ctypes.data))
    layout = dict(zip("aos pt lists ids n_ids id_mask".split(), out.tolist()))
    return recs, pt, ids[: layout["n_ids"]].copy(), layout
