"""GPU: clearance, the Euclidean distance to the nearest collision OBB (include/epp.h):
epp_states_clearance per state and epp_traj_clearance_batch as the closest approach of fitted
tracks' rows, straight from their coefficients; and the Python / PathPlanner layers.

Against the numpy restatement (clearance_ref.py: the same IEEE operations in the same
association, so d2 and its minimum are the same bits) `nearest` and `row` must match exactly
and the distance within 1 ulp of np.sqrt(d2): only the device's square root may round
differently.  By definition the fused call is epp_sample_count + epp_sample_batch +
epp_states_clearance on the rows' columns 0 / 3 / 6 with a per-track minimum that prefers the
earliest row: all four outputs are compared with that composition with ==.

Worlds, state sets and tracks: clearance_inputs.py (its claims are checked on the CPU in
test_clearance_inputs_cpu.py).  T = kClearTile, the LDS tile of both kernels.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import clearance_inputs as ci
import clearance_ref as cr
import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi
from test_gpu_trajsweep import _sample

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _world(name):
    _, rg, ro = spi.setup()
    return capi.World(ci.obbs(name), rg, ro)


@functools.lru_cache(maxsize=None)
def _fit():
    Ts, Cs, st = capi.minsnap_batch(tsi.fit_waypoints(), 1.0, 2.0)
    assert (st == 0).all()
    return Ts, Cs


@functools.lru_cache(maxsize=None)
def _fit_ref_rows():
    """The restatement's rows of the GPU fits at FIT_DT (world-independent: computed once)."""
    Ts, Cs = _fit()
    return [cr.sample_rows(T, Cf, ci.FIT_DT) for T, Cf in zip(Ts, Cs)]


@functools.lru_cache(maxsize=None)
def _state_ref(name, n):
    return cr.states(ci.obbs(name), ci.points(name, n))


def _assert_dist(got, d2_ref, what):
    exp = np.sqrt(d2_ref)
    u = cr.ulps(got, exp)
    print(f"{what}: max |dist - sqrt(d2_ref)| = {u.max() if len(u) else 0.0} ulp, "
          f"equal {int((got == exp).sum())}/{len(exp)}")
    assert not np.isnan(got).any()
    assert (u <= 1.0).all()
    assert np.array_equal(np.isinf(got), np.isinf(exp)) and np.array_equal(got == 0.0, exp == 0.0)


# ---- 1. states against the restatement ------------------------------------------------------
@pytest.mark.parametrize("name", ci.WORLDS)
def test_states_equal_restatement(name):
    world = _world(name)
    counts = ci.STATE_COUNTS + ((ci.MANY,) if name in ci.MANY_WORLDS else ())
    for n in counts:
        pts = ci.points(name, n)
        d2, near = _state_ref(name, n)
        dist, got_near = world.clearance(pts)
        assert dist.dtype == np.float64 and got_near.dtype == np.int32 and len(dist) == n
        assert np.array_equal(got_near, near), n
        _assert_dist(dist, d2, f"{name} OBBs, {n} states")
    if name == "filling":
        assert np.isinf(dist).all() and (got_near == -1).all()


def test_states_nearest_is_optional():
    world = _world("72")
    pts = ci.points("72", 65)
    d_xyz = capi.DeviceBuffer.from_array(pts)
    d_dist = capi.DeviceBuffer(8 * len(pts))
    capi.check(capi.lib().epp_states_clearance(world.handle, d_xyz.ptr, len(pts), d_dist.ptr, None, None))
    capi.sync()
    assert np.array_equal(d_dist.download(np.float64, len(pts)), world.clearance(pts)[0])


# ---- 2. the fused call against the composition and the restatement ---------------------------
def _compose(world, rows, roff):
    """The definition: the rows' positions -> World.clearance -> per track the earliest row of
    the minimum distance.  (sqrt is monotone, so the earliest minimum of the distances is an
    argmin of d2; the CPU test of the inputs keeps distinct d2 from colliding after the root.)"""
    nt = len(roff) - 1
    clr, row = np.full(nt, np.inf), np.full(nt, -1, np.int64)
    time, near = np.full(nt, -1.0), np.full(nt, -1, np.int32)
    if len(rows) == 0:
        return clr, row, time, near
    dist, nr = world.clearance(np.ascontiguousarray(rows[:, [0, 3, 6]]))
    for k in range(nt):
        d = dist[roff[k]:roff[k + 1]]
        if len(d) == 0 or not np.isfinite(d).any():
            continue
        r = int(np.argmin(d))
        clr[k], row[k], time[k], near[k] = d[r], r, rows[roff[k] + r, 9], nr[roff[k] + r]
    return clr, row, time, near


def _assert_equals_composition(world, Ts, Cs, dt):
    rows, roff = _sample(Ts, Cs, dt)
    exp = _compose(world, rows, roff)
    got = world.trajectory_clearance(Ts, Cs, dt)
    assert [g.dtype for g in got] == [np.float64, np.int64, np.float64, np.int32]
    for g, e, what in zip(got, exp, ("clearance", "row", "time", "nearest")):
        assert np.array_equal(g, e), (what, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    assert ((got[1] == -1) == np.isinf(got[0])).all() and (got[1] < np.maximum(np.diff(roff), 1)).all()
    return got, np.diff(roff)


@pytest.mark.parametrize("name", ci.WORLDS)
def test_tracks_equal_composition_and_restatement(name):
    world = _world(name)
    Ts, Cs = _fit()
    assert len(Ts) == 64 and {len(t) for t in Ts} == set(range(1, 13))
    _, cnt = _assert_equals_composition(world, Ts, Cs, 0.01)
    assert cnt.max() > 2 * 512 and cnt.min() < 512  # several chunks, and less than one
    got, _ = _assert_equals_composition(world, Ts, Cs, ci.FIT_DT)
    d2, row, time, near = cr.tracks(ci.obbs(name), Ts, Cs, ci.FIT_DT, _fit_ref_rows())
    print(f"{name}: rows {got[1].tolist()}")
    assert np.array_equal(got[1], row) and np.array_equal(got[3], near) and np.array_equal(got[2], time)
    _assert_dist(got[0], d2, f"{name} OBBs, 64 fitted tracks")
    if name == "filling":
        assert np.isinf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1.0).all() and (got[3] == -1).all()


@pytest.mark.parametrize("name", ["T+1", "1100"])
def test_nearest_past_the_first_tile(name):
    """A track whose closest box is the world's last one: in the T + 1 world the only entry
    past the LDS tile."""
    world = _world(name)
    T, Cf = ci.last_box_track(name)
    d2, row, time, near = cr.tracks(ci.obbs(name), [T], [Cf], ci.DT)
    assert near[0] == len(ci.obbs(name)) - 1 and row[0] == 0
    got = world.trajectory_clearance([T], [Cf], ci.DT)
    assert got[1][0] == 0 and got[3][0] == near[0] and got[2][0] == time[0]
    _assert_dist(got[0], d2, f"{name} OBBs, last box")
    _assert_equals_composition(world, [T], [Cf], ci.DT)


# ---- 3. the edges of the walk ------------------------------------------------------------------
def test_walk_edges():
    """Straight tracks past the pole of the 1-OBB world: one launch, then some in launches of
    their own."""
    names, Ts, Cs, want, zero = ci.edge_tracks()
    world = _world("1")
    d2, row, time, near = cr.tracks(ci.obbs("1"), Ts, Cs, ci.DT)
    assert row.tolist() == want
    got = world.trajectory_clearance(Ts, Cs, ci.DT)
    print("edges:", list(zip(names, got[1].tolist(), got[0].tolist())))
    assert np.array_equal(got[1], row) and np.array_equal(got[2], time) and np.array_equal(got[3], near)
    _assert_dist(got[0], d2, "edge tracks")
    assert np.array_equal(got[0] == 0.0, np.array(zero))
    for k, name in enumerate(names):
        if want[k] < 0:
            assert (got[0][k], got[1][k], got[2][k], got[3][k]) == (np.inf, -1, -1.0, -1), name
    _assert_equals_composition(world, Ts, Cs, ci.DT)
    for k in range(0, len(Ts), 3):
        alone = world.trajectory_clearance(Ts[k:k + 1], Cs[k:k + 1], ci.DT)
        assert all(a[0] == g[k] for a, g in zip(alone, got)), names[k]


# ---- 4. independence, optional outputs, staging -----------------------------------------------
def test_each_track_alone_equals_the_batch():
    world = _world("T+1")
    Ts, Cs = _fit()
    batch = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    for k in range(0, 64, 5):
        alone = world.trajectory_clearance(Ts[k:k + 1], Cs[k:k + 1], ci.FIT_DT)
        assert all(a[0] == b[k] for a, b in zip(alone, batch)), k


def test_optional_outputs_may_be_null():
    world = _world("72")
    Ts, Cs = _fit()
    nt = len(Ts)
    full = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_clr = capi.DeviceBuffer(8 * nt)
    capi.check(capi.lib().epp_traj_clearance_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, ci.FIT_DT, d_clr.ptr,
                                                   None, None, None, None))
    capi.sync()
    assert np.array_equal(d_clr.download(np.float64, nt), full[0])


@pytest.mark.parametrize("name", ["72", "T+1"])
def test_records_through_l2_equal_staged(name, monkeypatch):
    """EPP_TRAJCLEAR_STAGE=0: every record read through L2 instead of the LDS tile."""
    world = _world(name)
    Ts, Cs = _fit()
    staged = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    monkeypatch.setenv("EPP_TRAJCLEAR_STAGE", "0")
    direct = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    assert all(np.array_equal(a, b) for a, b in zip(staged, direct))
    assert np.isfinite(staged[0]).all()


def test_after_world_update():
    fgeom, rg, ro = spi.setup()
    Ts, Cs = _fit()
    pts = ci.points("72", 257)
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    before = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    moved = capi.build_obbs(fgeom, *spi.poses(72, moved=True))
    world.update(moved)  # (no build_index: the calls rebuild it)
    got = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    got_pts = world.clearance(pts)
    fresh = capi.World(moved, rg, ro)
    exp = fresh.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    assert all(np.array_equal(a, b) for a, b in zip(got, exp))
    assert all(np.array_equal(a, b) for a, b in zip(got_pts, fresh.clearance(pts)))
    assert not np.array_equal(got[0], before[0])  # (the move changes answers)


def test_graph_replay():
    fgeom, rg, ro = spi.setup()
    Ts, Cs = _fit()
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    world.build_index()
    direct = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    pts = ci.points("72", 257)
    direct_pts = world.clearance(pts)
    L = capi.lib()
    nt, n = len(Ts), len(pts)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_xyz = capi.DeviceBuffer.from_array(pts)
    outs = [capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(4 * nt),
            capi.DeviceBuffer(8 * n), capi.DeviceBuffer(4 * n)]
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_traj_clearance_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, ci.FIT_DT, outs[0].ptr,
                                          outs[1].ptr, outs[2].ptr, outs[3].ptr, s.value))
    capi.check(L.epp_states_clearance(world.handle, d_xyz.ptr, n, outs[4].ptr, outs[5].ptr, s.value))
    capi.check(L.epp_graph_end(s.value, C.byref(g)))
    for b in outs:
        capi.check(L.epp_memset(b.ptr, 0x5A, b.nbytes, None))  # poison
    capi.sync()
    capi.check(L.epp_graph_launch(g.value, s.value))
    capi.check(L.epp_stream_sync(s.value))
    dts = (np.float64, np.int64, np.float64, np.int32)
    for b, dt, e in zip(outs[:4], dts, direct):
        assert np.array_equal(b.download(dt, nt), e)
    assert np.array_equal(outs[4].download(np.float64, n), direct_pts[0])
    assert np.array_equal(outs[5].download(np.int32, n), direct_pts[1])
    capi.check(L.epp_graph_destroy(g.value))
    L.epp_stream_destroy(s.value)


# ---- 5. consistency with the minDistance check -------------------------------------------------
def test_consistent_with_check_trajectories():
    """inflated box (by md) contains the Euclidean ball of radius md around the box and lies in
    the ball of radius sqrt(3) md: clearance < md implies a failing row at or before row[k]
    -- if the rtree's AABB prefilter (inflated by the world's radii, >= md here) lets the row
    through, which it does for md <= the radii -- and clearance > sqrt(3) md implies none."""
    _, rg, ro = spi.setup()
    md = 0.5 * min(rg, ro)
    world = _world("72")
    Ts, Cs = _fit()
    clr, row, _, _ = world.trajectory_clearance(Ts, Cs, ci.FIT_DT)
    first, _ = world.check_trajectories(Ts, Cs, ci.FIT_DT, md)
    assert (np.abs(clr - md) > 1e-6).all() and (np.abs(clr - np.sqrt(3) * md) > 1e-6).all()
    close, far = clr < md, clr > np.sqrt(3) * md
    assert close.sum() >= 4 and far.sum() >= 4
    assert ((first[close] >= 0) & (first[close] <= row[close])).all()
    assert (first[far] == -1).all()


# ---- 6. C++ / pybind ----------------------------------------------------------------------------
def test_path_planner_candidate_clearances():
    import online_traj_planner as otp
    gates, obstacles = spi.poses(72)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    sets = tsi.fit_waypoints()[:8]
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    exp = _world("72").trajectory_clearance(Ts, Cs, ci.FIT_DT)
    got = pp.candidate_clearances(sets, 1.0, 2.0, ci.FIT_DT)
    assert [g.dtype for g in got] == [np.float64, np.int64, np.float64, np.int32]
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    assert np.isfinite(got[0]).all()
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_clearances([sets[0], sets[1][:1]], 1.0, 2.0, ci.FIT_DT)
    assert [len(r) for r in pp.candidate_clearances([], 1.0, 2.0, ci.FIT_DT)] == [0, 0, 0, 0]


def test_world_clearance_host_arrays():
    """World::clearance through the zero-copy and the staged query path (pybind: clearance)."""
    import online_traj_planner as otp
    gates, obstacles = spi.poses(72)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    world = _world("72")
    for n in (1, 257, 20000):  # one point, zero-copy, staged through HBM
        pts = ci.points("72", n)
        dist, near = pp.clearance(pts)
        exp = world.clearance(pts)
        assert dist.dtype == np.float64 and near.dtype == np.int32
        assert np.array_equal(dist, exp[0]) and np.array_equal(near, exp[1])
