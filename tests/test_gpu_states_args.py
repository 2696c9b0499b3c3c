"""k_states_v5 takes the world's parameters by value (the staging source pointer and the
scalars its first loads need as leading arguments, the packed LDS offsets and the class
grid in a small struct) instead of reading them through a pointer into device memory.
These tests drive that parameter path where it can go wrong, flags bit-exact against the
oracle:

  - every forced launch shape (EPP_STATES_KERNEL=v5, EPP_V5_BLOCK unset / 256 / 512 / 1024);
  - n = 1, 2, 3 (no full group of four: the lanes' ignored loads read the staging source
    instead of the states), 4, 5, one 512-thread workgroup of groups -1 / 0 / +1 (2047,
    2048, 2049), and one n just over 2 * CUs * 512 * 4, past every single-pass shape (the
    prefetching instantiations);
  - both can_pass_gate values, the minDistance variant and the compacting variant;
  - the C2 world (64 OBBs, sparse byte classes) and a world of 60 clustered OBBs with more
    than 255 candidate lists, whose class table is staged as u16 (the other branch of the
    packed class offsets, and 4 / 8 staging chunks per lane instead of 2);
  - states outside the bounds, far outside, and NaN.

The worlds, the points and the oracle's answers are built once and shared, read-only.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from eppamd import capi, config, synth

from conftest import CONFIG
from small_path_inputs import adversarial_points

pytestmark = pytest.mark.gpu

CUS = 256                                # MI355X
N_MULTI = 2 * CUS * 512 * 4 + 4 * 3 + 1  # three groups and a tail state past the last single-pass shape
N_EDGES = (1, 2, 3, 4, 5, 2047, 2048, 2049)
N_SMALL = 2049
SHAPES = ("", "256", "512", "1024")
MIN_DISTANCE = 0.15


@functools.lru_cache(maxsize=None)
def _setup():
    cfg = config.load(CONFIG)
    return config.geometry(cfg), config.inflate_radii(cfg)


@functools.lru_cache(maxsize=None)
def _poses(name):
    if name == "c2":
        return synth.track_world(42) + (synth.C2_BOUNDS,)
    # 60 single-OBB obstacles within 1.2 m x 1.2 m: few records, many distinct candidate lists
    rs = np.random.RandomState(5)
    obstacles = np.zeros((60, 6))
    obstacles[:, :2] = rs.uniform(-0.6, 0.6, (60, 2))
    return np.zeros((0, 7)), obstacles, (np.array([-1.0, -1.0, 0.0]), np.array([1.0, 1.0, 2.0]))


@functools.lru_cache(maxsize=None)
def _world(name):
    """(OBBs, the oracle's world, class-grid layout of the host index build)."""
    geom, (rg, ro) = _setup()
    gates, obstacles, _ = _poses(name)
    obbs = capi.build_obbs(geom, gates, obstacles)
    f = capi.lib().epp_dbg_class_layout
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    out = np.zeros(12, np.int64)
    capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, out.ctypes.data))
    layout = dict(zip("aos lists ids cls8 bitmap blob nlists cells bnx bny bnz staged".split(), out.tolist()))
    return obbs, O.world_build(geom, gates, obstacles, rg, ro), layout


@functools.lru_cache(maxsize=None)
def _points(name, n):
    """n states: the first five are an OBB centre, a NaN state, a far-away state, a state with
    one NaN coordinate and another OBB centre (so the prefixes 1..5 hold both answers and
    the odd values); then random states from a box 1 m wider than the bounds on every side,
    points on and an ulp around the AABB faces, and far-away and NaN states again in the
    last groups."""
    _, ref, _ = _world(name)
    lo, hi = _poses(name)[2]
    odd = np.array([[1e6, -1e6, 1.0], [np.nan, np.nan, np.nan], [0.1, np.nan, 0.5], [-1e30, 0.0, 1e30],
                    [np.inf, 0.0, 1.0]])
    head = np.array([ref[0]["center"], odd[1], odd[0], odd[2], ref[len(ref) - 1]["center"]])
    adv = adversarial_points(ref)[:1200]
    rnd = synth.sample_states(77, lo - 1.0, hi + 1.0, n - len(head) - len(adv) - len(odd))
    pts = np.ascontiguousarray(np.vstack([head, adv[:600], rnd, adv[600:], odd]))
    assert pts.shape == (n, 3)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _expected(name, n, variant):
    """variant: 0 / 1 = can_pass_gate, "md" = minDistance."""
    _, (rg, ro) = _setup()
    _, ref, _ = _world(name)
    pts = _points(name, n)
    exp = (O.check_states_mindist(ref, pts, MIN_DISTANCE) if variant == "md"
           else O.check_states(ref, rg, ro, pts, bool(variant), threads=8))
    exp.setflags(write=False)
    return exp


@pytest.fixture
def forced(monkeypatch):
    def f(shape):
        monkeypatch.setenv("EPP_STATES_KERNEL", "v5")  # (also keeps n <= 4096 off the brute-force kernel)
        monkeypatch.setenv("EPP_V5_BLOCK", shape)
    return f


def test_worlds_take_both_class_table_branches():
    """Host index build: C2 stages byte classes, the clustered world the u16 table, and
    both fit k_states_v5's staging budget (so neither falls through to k_states_v4)."""
    c2, u16 = _world("c2")[2], _world("u16")[2]
    assert c2["cls8"] != 0 and c2["nlists"] <= 256 and c2["staged"] <= 64 * 1024
    assert u16["cls8"] == 0 and u16["nlists"] > 255 and 48 * 1024 < u16["staged"] <= 64 * 1024
    for name in ("c2", "u16"):  # the points hold both answers
        e = _expected(name, N_SMALL, 0)
        assert 0 < e[:5].sum() < 5 and 0 < e.sum() < len(e)


def _launch_all(w, name, n, n_pts):
    pts = _points(name, n_pts)[:n]
    for can_pass in (0, 1):
        exp = _expected(name, n_pts, can_pass)[:n]
        got = w.check_states(pts, can_pass)
        assert np.array_equal(got, exp), (n, can_pass, np.flatnonzero(got != exp)[:10])
        valid, idx = w.check_states(pts, can_pass, compact=True)
        assert np.array_equal(valid, exp), (n, can_pass, "compact")
        assert len(idx) == int(exp.sum()) and np.array_equal(np.sort(idx), np.flatnonzero(exp)), (n, can_pass)
    got = w.check_states_mindist(pts, MIN_DISTANCE)
    assert np.array_equal(got, _expected(name, n_pts, "md")[:n]), (n, "md")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["c2", "u16"])
def test_forced_shapes_at_group_and_workgroup_edges(name, shape, forced):
    forced(shape)
    _, (rg, ro) = _setup()
    w = capi.World(_world(name)[0], rg, ro)
    for n in N_EDGES:
        _launch_all(w, name, n, N_SMALL)


@pytest.mark.parametrize("shape", SHAPES)
def test_forced_shapes_past_the_single_pass(shape, forced):
    """More than one group per lane: the prefetching instantiations (512- or 1024-thread
    workgroups, one per CU), every variant."""
    forced(shape)
    _, (rg, ro) = _setup()
    w = capi.World(_world("c2")[0], rg, ro)
    _launch_all(w, "c2", N_MULTI, N_MULTI)


def test_multi_pass_u16_classes(forced):
    """The u16 class table on the prefetching shape: the clustered world's 2049 states
    tiled up to N_MULTI (the oracle's answers tiled alike: no second oracle pass)."""
    forced("")
    _, (rg, ro) = _setup()
    w = capi.World(_world("u16")[0], rg, ro)
    reps = -(-N_MULTI // N_SMALL)
    pts = np.tile(_points("u16", N_SMALL), (reps, 1))[:N_MULTI]
    exp = np.tile(_expected("u16", N_SMALL, 0), reps)[:N_MULTI]
    assert np.array_equal(w.check_states(pts, 0), exp)
