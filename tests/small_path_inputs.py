"""Worlds and query sets of the small-path tests (test_gpu_small_path.py) and of the CPU test
of those inputs (test_small_path_inputs_cpu.py).

The brute-force kernels of small.hip answer every call of <= 4096 states / <= 1024 edges on
a world of <= 256 OBBs.  The worlds here have an exact OBB count under
configs/config_filling.json (6 OBBs per gate, one of them the filling "opening"; 1 per
obstacle), chosen around the branches of that code: the register-staged copy covers 150
records and a tail loop the rest, a workgroup splits the list into 1, 2, 4 or 16 slices, and
257 OBBs fall through to the index kernels.

Everything is input data and oracle output: built once per process, shared, read-only.
"""
import functools
import os

import numpy as np

import oracle as O
from eppamd import capi, config, synth

FILLING_CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "configs", "config_filling.json")

SMALL_OBB_COUNTS = (1, 2, 3, 6, 15, 16, 17, 63, 150, 151, 255, 256)  # the small path
INDEX_OBB_COUNT = 257                                                # the index kernels
OBB_COUNTS = SMALL_OBB_COUNTS + (INDEX_OBB_COUNT,)
BOTH_OBB_COUNTS = (72, 256, 257)  # 72: synth.track_world(42), the suite's C2 world

N_STATES = 4096   # kSmallStates; the sets hold one query more (the first past the small path)
N_MOTIONS = 1024  # kSmallMotions
N_BOTH = 16385    # one past World::query's zero-copy limit
STATE_PREFIXES = (1, 63, 64, 65, 128, 129, 257, 4096)  # per = 64, 128, 256; one and many workgroups
MOTION_PREFIXES = (1, 15, 16, 17, 1023, 1024)
BOTH_PREFIXES = (1, 16, 17, 1024, 1025, 16384, 16385)
MIN_DISTANCES = (0.0, 0.2)


def small_per(n):
    """Queries per workgroup of k_states_small (small_body.h, small_per)."""
    return 64 if n <= 64 else (128 if n <= 128 else 256)


def adversarial_points(ref_w):
    """Points exactly on / one ulp around every AABB face and corner."""
    pts = []
    for o in ref_w:
        mid = (o["aabb_lo"] + o["aabb_hi"]) / 2
        for k in range(3):
            for v in (o["aabb_lo"][k], o["aabb_hi"][k]):
                for w in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
                    p = mid.copy()
                    p[k] = w
                    pts.append(p)
        pts += [o["aabb_lo"].copy(), o["aabb_hi"].copy(), np.nextafter(o["aabb_hi"], -np.inf),
                np.nextafter(o["aabb_lo"], np.inf), o["center"].copy()]
        # points on the inflated OBB faces in local coordinates
        c, s = o["rot"][0], o["rot"][3]
        for sx in (-1, 1):
            l = np.array([sx * (o["half"][0] + 0.2), 0.3 * o["half"][1], 0.0])
            pts.append(o["center"] + np.array([c * l[0] - s * l[1], s * l[0] + c * l[1], l[2]]))
    return np.array(pts)


def gate_openings(gates, geom, n_per_gate=400, seed=3):
    """States in and around every gate opening (the filling boxes), in world coordinates."""
    rs = np.random.RandomState(seed)
    out = []
    for g in gates:
        h = geom.gate_height[int(g[6])]
        loc = rs.uniform([-0.3, -0.05, -0.3], [0.3, 0.05, 0.3], size=(n_per_gate, 3))
        c, s = np.cos(g[5]), np.sin(g[5])
        out.append(np.stack([g[0] + c * loc[:, 0] - s * loc[:, 1], g[1] + s * loc[:, 0] + c * loc[:, 1],
                             h + loc[:, 2]], 1))
    return np.vstack(out)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def setup():
    """(geometry, r_gate, r_obstacle) of configs/config_filling.json."""
    cfg = config.load(FILLING_CONFIG)
    fgeom = config.geometry(cfg)
    assert fgeom.gate_desc["filling"].sum() == 2 and len(fgeom.gate_desc) == 12 and len(fgeom.obst_desc) == 1
    rg, ro = config.inflate_radii(cfg)
    return fgeom, rg, ro


def n_gates_for(n_obb):
    """No gate up to 3 OBBs, one from 6 to 17, eight from 63 up: the worlds with gates have
    filling records, so can_pass matters there."""
    return 0 if n_obb <= 3 else (1 if n_obb <= 17 else 8)


@functools.lru_cache(maxsize=None)
def poses(n_obb, moved=False):
    """(gates, obstacles) of the world with exactly n_obb OBBs; moved: the same world with
    every object shifted and every gate turned (a second version for the update tests)."""
    g = n_gates_for(n_obb)
    if n_obb == 72:
        gates, obstacles = synth.track_world(42)
    else:
        gates, obstacles = synth.track_world(100 + n_obb, n_gates=g, n_obstacles=n_obb - 6 * g)
    assert gates.shape == (g, 7) and len(obstacles) == n_obb - 6 * g
    if moved:
        gates, obstacles = gates.copy(), obstacles.copy()
        gates[:, 0] += 0.15
        gates[:, 5] += 0.1
        obstacles[:, 1] -= 0.04  # (within the 0.05 m half-width: the old centre stays inside)
    return _frozen(gates, obstacles)


@functools.lru_cache(maxsize=None)
def world(n_obb, moved=False):
    """(OBBs for capi.World, the oracle's world) of poses(n_obb, moved)."""
    fgeom, rg, ro = setup()
    gates, obstacles = poses(n_obb, moved)
    obbs = capi.build_obbs(fgeom, gates, obstacles)
    ref = O.world_build(fgeom, gates, obstacles, rg, ro)
    assert len(obbs) == n_obb == len(ref)
    assert sum(int(o["filling"]) for o in ref) == len(gates)
    return _frozen(obbs, ref)


def _opening_rays(gates, fgeom, n_per_gate, seed, reach=0.4):
    """Rays through the openings along the gate normal (the way a drone passes a gate)."""
    a = gate_openings(gates, fgeom, n_per_gate, seed=seed)
    yaw = np.repeat(gates[:, 5], n_per_gate)
    nrm = np.stack([-np.sin(yaw), np.cos(yaw), np.zeros_like(yaw)], 1)
    return a - reach * nrm, a + reach * nrm


@functools.lru_cache(maxsize=None)
def state_points(n_obb):
    """N_STATES + 1 points: random in C2_BOUNDS, points on and an ulp around the AABB faces,
    corners and centres (all of them, or 2048 drawn from them), points in and just around the
    last record's AABB, and points in and around the gate openings; shuffled, so that every
    prefix holds some of each.  The last point is past the small path's limit."""
    fgeom, _, _ = setup()
    gates, _ = poses(n_obb)
    _, ref = world(n_obb)
    rs = np.random.RandomState(7000 + n_obb)
    adv = adversarial_points(ref)
    if len(adv) > 2048:
        adv = adv[np.sort(rs.choice(len(adv), 2048, replace=False))]
    # in and just around the last record's AABB: the record a staging or remainder loop loses first
    last = ref[n_obb - 1]
    parts = [adv, rs.uniform(last["aabb_lo"] - 0.05, last["aabb_hi"] + 0.05, size=(64, 3))]
    if len(gates):
        parts.append(gate_openings(gates, fgeom, 512 // len(gates), seed=n_obb))
    n_rand = N_STATES - sum(len(p) for p in parts)
    parts.append(synth.sample_states(300 + n_obb, *synth.C2_BOUNDS, n_rand))
    pts = np.vstack(parts)[rs.permutation(N_STATES)]
    return _frozen(np.ascontiguousarray(np.vstack([pts, synth.sample_states(301 + n_obb, *synth.C2_BOUNDS, 1)])))


@functools.lru_cache(maxsize=None)
def motion_edges(n_obb):
    """N_MOTIONS + 1 edges: random ones (max_len 1.5), rays through the gate openings along
    the gate normal, edges aimed at the OBBs, edges across and beside the last record, and edges
    next to the OBBs that are parallel to an axis within the 1e-6 threshold of src/OBB.cpp:34
    (|d_y| = 9.9e-7 and 1.01e-6); shuffled."""
    fgeom, _, _ = setup()
    gates, _ = poses(n_obb)
    _, ref = world(n_obb)
    rs = np.random.RandomState(8000 + n_obb)
    centers = np.array([o["center"] for o in ref])
    k = 128  # near-parallel
    t1 = centers[np.arange(k) % n_obb] + rs.uniform([-1.0, -0.4, -0.3], [0.2, 0.4, 0.3], size=(k, 3))
    t2 = t1.copy()
    t2[:, 0] += 0.8
    t2[:, 1] += np.where(np.arange(k) % 2, 9.9e-7, 1.01e-6)
    k = 192  # aimed at an OBB from either side
    c = centers[rs.randint(0, n_obb, k)]
    d = rs.normal(size=(2, k, 3)) * [1.0, 1.0, 0.4]
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    a1, a2 = c + d[0] * rs.uniform(0.2, 1.2, (k, 1)), c - d[1] * rs.uniform(0.0, 1.2, (k, 1))
    last = ref[n_obb - 1]  # across and beside the last record (see state_points)
    l1, l2 = rs.uniform(last["aabb_lo"] - 0.4, last["aabb_hi"] + 0.4, size=(2, 64, 3))
    s1, s2 = [t1, a1, l1], [t2, a2, l2]
    if len(gates):
        o1, o2 = _opening_rays(gates, fgeom, 256 // len(gates), seed=n_obb + 1)
        s1.append(o1)
        s2.append(o2)
    n_rand = N_MOTIONS - sum(len(p) for p in s1)
    r1, r2 = synth.edges(400 + n_obb, 500 + n_obb, *synth.C2_BOUNDS, n_rand, max_len=1.5)
    x1, x2 = synth.edges(401 + n_obb, 501 + n_obb, *synth.C2_BOUNDS, 1, max_len=1.5)
    p = rs.permutation(N_MOTIONS)
    return _frozen(np.ascontiguousarray(np.vstack([np.vstack(s1 + [r1])[p], x1])),
                   np.ascontiguousarray(np.vstack([np.vstack(s2 + [r2])[p], x2])))


@functools.lru_cache(maxsize=None)
def both_rays(n_obb):
    """N_BOTH rays for World::checkRaysBoth: through the openings along the normal, from in
    front of an opening through it and on (sideways into the frame, or far beyond it), from an
    opening to an obstacle, and random ones (max_len 1.5); shuffled."""
    fgeom, _, _ = setup()
    gates, obstacles = poses(n_obb)
    rs = np.random.RandomState(9000 + n_obb)
    ng = len(gates)
    o1, o2 = _opening_rays(gates, fgeom, 2048 // ng, seed=n_obb + 2)
    k = 4096 // ng  # through the opening and on
    loc = rs.uniform([-0.3, -0.6, -0.3], [0.3, -0.3, 0.3], size=(ng, k, 3))
    loc2 = loc + np.stack([rs.uniform(-0.6, 0.6, (ng, k)), rs.uniform(0.6, 3.0, (ng, k)),
                           rs.uniform(-0.6, 0.6, (ng, k))], 2)
    h = fgeom.gate_height[gates[:, 6].astype(int)][:, None]
    cs, sn = np.cos(gates[:, 5])[:, None], np.sin(gates[:, 5])[:, None]

    def to_world(l):
        return np.stack([gates[:, :1] + cs * l[..., 0] - sn * l[..., 1], gates[:, 1:2] + sn * l[..., 0] + cs * l[..., 1],
                         h + l[..., 2]], 2).reshape(-1, 3)

    p1, p2 = _opening_rays(gates, fgeom, 2048 // ng, seed=n_obb + 3)  # from an opening to an obstacle
    p2 = obstacles[rs.randint(0, len(obstacles), len(p1)), :3] + np.c_[np.zeros((len(p1), 2)), rs.uniform(0.1, 1.0, len(p1))]
    n_rand = N_BOTH - 1 - (len(o1) + ng * k + len(p1))
    r1, r2 = synth.edges(600 + n_obb, 700 + n_obb, *synth.C2_BOUNDS, n_rand + 1, max_len=1.5)
    p = rs.permutation(N_BOTH - 1)
    s1 = np.vstack([o1, to_world(loc), p1, r1[:-1]])[p]
    s2 = np.vstack([o2, to_world(loc2), p2, r2[:-1]])[p]
    return _frozen(np.ascontiguousarray(np.vstack([s1, r1[-1:]])), np.ascontiguousarray(np.vstack([s2, r2[-1:]])))


@functools.lru_cache(maxsize=None)
def query_points(n_obb):
    """N_BOTH points for World::checkPoints: state_points' first 4096 and random ones."""
    rest = synth.sample_states(800 + n_obb, *synth.C2_BOUNDS, N_BOTH - N_STATES)
    return _frozen(np.ascontiguousarray(np.vstack([state_points(n_obb)[:N_STATES], rest])))


# ---- the oracle's answers (computed once, shared, read-only) ---------------------------------
@functools.lru_cache(maxsize=None)
def exp_states(n_obb, can_pass):
    _, rg, ro = setup()
    return _frozen(O.check_states(world(n_obb)[1], rg, ro, state_points(n_obb), bool(can_pass), threads=8))


@functools.lru_cache(maxsize=None)
def exp_mindist(n_obb, md, moved=False):
    return _frozen(O.check_states_mindist(world(n_obb, moved)[1], state_points(n_obb), md))


@functools.lru_cache(maxsize=None)
def exp_motions(n_obb, can_pass, mode):
    _, rg, ro = setup()
    s1, s2 = motion_edges(n_obb)
    return _frozen(O.check_motions(world(n_obb)[1], rg, ro, s1, s2, bool(can_pass), mode, threads=8))


def both_bits(ref, s1, s2):
    """World::checkRaysBoth's answer from the oracle: bit 0 canPassGate = false, bit 1 true."""
    _, rg, ro = setup()
    e0 = O.check_motions(ref, rg, ro, s1, s2, False, 0, threads=8).astype(np.uint8)
    e1 = O.check_motions(ref, rg, ro, s1, s2, True, 0, threads=8).astype(np.uint8)
    return e0 | (e1 << 1)


@functools.lru_cache(maxsize=None)
def exp_both(n_obb):
    return _frozen(both_bits(world(n_obb)[1], *both_rays(n_obb)))


# ---- the fused check's tracks -----------------------------------------------------------------
FUSED_OBB_COUNTS = (1, 17, 151, 256)
FUSED_N_CHECK = (1, 64, 65, 128, 129, 4096)
FUSED_ARGS = (1.0, 2.0, 0.1, 0.25, (0.3, -0.1, 0.0), (0.0, 0.2, 0.0))  # v_max, a_max, dt, t0, v0, a0


@functools.lru_cache(maxsize=None)
def fused_track(name):
    """Waypoints: "2wp" (one segment: the refit needs less LDS than the records of a large
    world), "12seg" (the C5 track) and "41seg" (past the refit's LDS limit of 40 segments)."""
    if name == "2wp":
        return _frozen(np.array([[-2.0, -1.0, 0.5], [1.5, 2.0, 1.2]]))
    return _frozen(synth.random_track_waypoints(77 if name == "12seg" else 79, {"12seg": 12, "41seg": 41}[name]))


@functools.lru_cache(maxsize=None)
def fused_rows(name):
    v_max, a_max, dt, t0, v0, a0 = FUSED_ARGS
    return _frozen(O.generate_trajectory(fused_track(name), v_max, a_max, dt, t0, v0, a0))
