"""k_states_v5's chain behind a wave's state data: the batched, branch-free class lookup
and the pair layout that a forward lane permute builds (one permute for up to 64 (state,
candidate) pairs of a queue round, two for up to 128; more than 128 pairs: each queued state
walks its own list; more than 64 queued states: several queue rounds).  Uniform samples sit
near 27 queued states and 44 pairs per wave and never reach those edges, so the states here
are constructed; flags bit-exact against the oracle.

Pair-count thresholds: worlds of k = 1, 2, 3 identical obstacle boxes at one place, so every
state inside the boxes' inflated AABB has a k-long candidate list and every other state
none.  One launch of 10 x 256 states: wave w owns states [256 w, 256 w + 256) and holds M[w]
cluster states at scattered positions, the rest far away.  Per queue round of up to 64
queued states that is 1, 63 and 64 pairs (k = 1: one permute), 126 and 128 (k = 2: two
permutes, exactly 128 included), 129, 189 and 192 (k = 3: the own-list walk), and 65 to
256 queued states (two to four rounds).  About half of the cluster states lie inside the
inflated box (turned 45 degrees in its AABB) and half in the AABB's corners, so a pair
attributed to the wrong state or to the wrong list entry changes a flag.

Class-lookup edges on the C2 world: states below, above and far outside the class grid on
each axis, infinite and NaN coordinates, the first and the last cell of the grid, the top
layer of cells (behind the last occupied cell of the sparse table: the class byte read for
them is the one after the table's last), and states on and an ulp around cell boundaries of
occupied cells; mixed into 5,000 uniform states, ragged n.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from eppamd import capi, config, synth

from conftest import CONFIG

pytestmark = pytest.mark.gpu

SHAPES = ("", "512", "1024")
M = (0, 1, 43, 63, 64, 65, 127, 128, 255, 256)  # cluster states of wave w (43 x 3 = 129 pairs)
WAVE = 256                                   # states per wave: 64 lanes x 4
CLUSTER_XY = (1.0, -0.5)
MIN_DISTANCE = 0.15


@functools.lru_cache(maxsize=None)
def _setup():
    cfg = config.load(CONFIG)
    return config.geometry(cfg), config.inflate_radii(cfg)


@pytest.fixture
def forced(monkeypatch):
    def f(shape):
        monkeypatch.setenv("EPP_STATES_KERNEL", "v5")  # (also keeps n <= 4096 off the brute-force kernel)
        monkeypatch.setenv("EPP_V5_BLOCK", shape)
    return f


# ---- pair-count thresholds ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cluster(k):
    """(OBBs, oracle world, states, is-cluster mask) of k co-located obstacle boxes."""
    geom, (rg, ro) = _setup()
    obstacles = np.zeros((k, 6))
    obstacles[:, :2] = CLUSTER_XY
    obstacles[:, 5] = np.pi / 4  # yaw: the boxes leave the corners of their AABB free
    gates = np.zeros((0, 7))
    obbs = capi.build_obbs(geom, gates, obstacles)
    ref = O.world_build(geom, gates, obstacles, rg, ro)
    assert len(ref) == k
    lo, hi = ref[0]["aabb_lo"], ref[0]["aabb_hi"]
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rs = np.random.RandomState(100 + k)
    n = len(M) * WAVE
    pts = np.empty((n, 3))
    pts[:, :2] = rs.uniform(4.0, 5.0, (n, 2)) * rs.choice([-1.0, 1.0], (n, 2)) + ctr[:2]  # far away
    pts[:, 2] = rs.uniform(0.0, 2.0, n)
    inside = np.zeros(n, bool)
    for w, m in enumerate(M):
        at = WAVE * w + np.sort(rs.permutation(WAVE)[:m])
        inside[at] = True
        # the boxes stand at 45 degrees in the AABB and leave its corners free: most of the
        # states uniform in the AABB (mostly inside the inflated box), a third towards the
        # corners (mostly outside it), many of either kind close to the box's faces
        u = rs.uniform(-0.98, 0.98, (m, 3))
        corner = rs.rand(m) < 0.35
        u[corner, :2] = rs.uniform(0.6, 0.98, (int(corner.sum()), 2)) * rs.choice([-1.0, 1.0], (int(corner.sum()), 2))
        pts[at] = ctr + u * half
    # every cluster state is a candidate of every box (strictly inside the AABB), no other is
    assert np.all((pts[inside] > lo) & (pts[inside] < hi))
    assert not np.any(np.all((pts[~inside] > lo - 1.0) & (pts[~inside] < hi + 1.0), axis=1))
    pts.setflags(write=False)
    return obbs, ref, pts, inside


@functools.lru_cache(maxsize=None)
def _cluster_expected(k, variant):
    _, (rg, ro) = _setup()
    _, ref, pts, _ = _cluster(k)
    exp = (O.check_states_mindist(ref, pts, MIN_DISTANCE) if variant == "md"
           else O.check_states(ref, rg, ro, pts, bool(variant)))
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("k", [1, 2, 3])
def test_cluster_states_hold_both_outcomes(k):
    """(no launch) The constructed states: far-away ones valid, cluster ones about half each."""
    _, _, _, inside = _cluster(k)
    for variant in (0, 1, "md"):
        exp = _cluster_expected(k, variant)
        assert exp[~inside].all()
        frac = exp[inside].mean()
        assert 0.3 < frac < 0.7, (variant, frac)
    for w, m in enumerate(M):
        assert inside[WAVE * w:WAVE * (w + 1)].sum() == m


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_pair_count_thresholds(k, shape, forced):
    forced(shape)
    _, (rg, ro) = _setup()
    obbs, _, pts, inside = _cluster(k)
    w = capi.World(obbs, rg, ro)
    for can_pass in (0, 1):
        exp = _cluster_expected(k, can_pass)
        got = w.check_states(pts, can_pass)
        assert np.array_equal(got, exp), (can_pass, np.flatnonzero(got != exp)[:10])
    exp = _cluster_expected(k, 0)
    valid, idx = w.check_states(pts, 0, compact=True)
    assert np.array_equal(valid, exp)
    assert np.array_equal(np.sort(idx), np.flatnonzero(exp))
    got = w.check_states_mindist(pts, MIN_DISTANCE)
    exp = _cluster_expected(k, "md")
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]


# ---- class-lookup edges on the C2 world --------------------------------------------------

def _class_grid(ref, obbs, rg, ro):
    """The class grid of the host index build (origin, cell size, cells per axis), rebuilt
    from the world's extent and checked against the build's own cell counts."""
    f = capi.lib().epp_dbg_class_layout
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    out = np.zeros(12, np.int64)
    capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, out.ctypes.data))
    dims = out[8:11]
    assert out[3] != 0, "C2 stages sparse byte classes"
    g0, g1 = ref["aabb_lo"].min(axis=0), ref["aabb_hi"].max(axis=0)
    ext = np.maximum(g1 - g0, 1e-3)
    for halvings in range(3):
        h = np.cbrt(ext.prod() / (2.0 ** (14 - halvings)))
        for extra in range(9):
            if np.array_equal(np.ceil(ext / h).astype(np.int64) + 4 + extra, dims):
                return g0 - 1.5 * h, h, dims
    raise AssertionError(("class grid not reconstructed", dims.tolist()))


@functools.lru_cache(maxsize=None)
def _c2():
    geom, (rg, ro) = _setup()
    gates, obstacles = synth.track_world(42)
    obbs = capi.build_obbs(geom, gates, obstacles)
    ref = O.world_build(geom, gates, obstacles, rg, ro)
    org, h, dims = _class_grid(ref, obbs, rg, ro)
    top = org + dims * h
    mid = 0.5 * (org + top)
    rs = np.random.RandomState(8)
    edge = []
    for ax in range(3):
        for v in (org[ax] - 0.5 * h, org[ax] - 1e-9, org[ax] + 0.5 * h, top[ax] - 0.5 * h, top[ax] + 1e-9,
                  top[ax] + 0.5 * h, -1e3, 1e3, -1e6, 1e6, -1e30, 1e30, -np.inf, np.inf, np.nan):
            p = mid + rs.uniform(-1.0, 1.0, 3) * 0.25 * (top - org)
            p[ax] = v
            edge.append(p)
    cell = lambda i: org + (np.asarray(i) + 0.5) * h  # noqa: E731  (a cell's centre)
    edge += [cell((0, 0, 0)), cell(dims - 1), org - 0.5 * h, top + 0.5 * h, np.full(3, np.nan), np.full(3, np.inf),
             np.full(3, -np.inf), cell((dims[0] - 1, 0, 0)), cell((0, dims[1] - 1, dims[2] - 1))]
    # the top layer and the one below it: cells behind the table's last occupied cell
    for z in (dims[2] - 1, dims[2] - 2):
        for _ in range(40):
            edge.append(cell((rs.randint(dims[0]), rs.randint(dims[1]), z)))
    # cell boundaries of occupied cells: the planes of the grid next to AABB faces and OBB
    # centres, on them and an ulp to either side, the other coordinates inside the AABB
    for o in ref:
        for face in (o["aabb_lo"], o["aabb_hi"], o["center"]):
            for ax in range(3):
                p = o["aabb_lo"] + rs.uniform(0.05, 0.95, 3) * (o["aabb_hi"] - o["aabb_lo"])
                b = org[ax] + np.round((face[ax] - org[ax]) / h) * h
                for v in (b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf), np.float64(np.float32(b))):
                    q = p.copy()
                    q[ax] = v
                    edge.append(q)
    edge = np.array(edge)
    rnd = synth.sample_states(15, *synth.C2_BOUNDS, 5000)
    n = len(edge) + len(rnd)
    n -= (n - 3) % 4  # n % 4 == 3
    third = len(edge) // 3
    pts = np.ascontiguousarray(np.vstack([edge[:third], rnd[:2500], edge[third:2 * third], rnd[2500:],
                                          edge[2 * third:]])[-n:])
    pts.setflags(write=False)
    exp = {v: (O.check_states_mindist(ref, pts, MIN_DISTANCE) if v == "md" else O.check_states(ref, rg, ro, pts, bool(v)))
           for v in (0, 1, "md")}
    return obbs, pts, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_class_lookup_edges(shape, forced):
    forced(shape)
    _, (rg, ro) = _setup()
    obbs, pts, exp = _c2()
    assert 0 < exp[0].sum() < len(pts)
    w = capi.World(obbs, rg, ro)
    for n in (len(pts), len(pts) - 1, len(pts) - 2):  # n % 4 = 3, 2, 1: the tail lanes see edge states too
        assert n % 4 in (1, 2, 3)
        for can_pass in (0, 1):
            got = w.check_states(pts[:n], can_pass)
            assert np.array_equal(got, exp[can_pass][:n]), (n, can_pass, np.flatnonzero(got != exp[can_pass][:n])[:10])
    valid, idx = w.check_states(pts, 0, compact=True)
    assert np.array_equal(valid, exp[0]) and np.array_equal(np.sort(idx), np.flatnonzero(exp[0]))
    assert np.array_equal(w.check_states_mindist(pts, MIN_DISTANCE), exp["md"])
