"""GPU: first hit (include/epp.h): epp_motions_first_hit, the entry parameter and OBB at which
each straight edge is first blocked, and epp_traj_first_hit_batch, the same for the first
failing chord of fitted tracks straight from their coefficients; and the Python / PathPlanner
layers.

Against the restatement (firsthit_ref.py: the same IEEE operations in the same association)
t_hit and obb must be equal as values for every edge (np.array_equal: -0.0 == 0.0, inf ==
inf).  obb >= 0 must hold exactly where epp_check_motions (mode 0) gives flag 0.  By definition
the fused call's chord is epp_traj_sweep_batch's, its t_hit and obb are epp_sample_batch
followed by epp_motions_first_hit on rows j, j + 1, and its time is t_j + t_hit * (t_j+1 - t_j)
on the sampled time column: all four outputs are compared with that composition with ==.

Worlds and edge sets: firsthit_inputs.py (its claims are checked on the CPU in
test_firsthit_inputs_cpu.py); tracks and their worlds: trajsweep_inputs.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import firsthit_inputs as fi
import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi
from test_gpu_trajcheck import _world as _fit_world
from test_gpu_trajsweep import _sample

pytestmark = pytest.mark.gpu

K_SEG_LDS = fi.ci.K_SEG_LDS


@functools.lru_cache(maxsize=None)
def _world(name):
    _, rg, ro = spi.setup()
    return capi.World(fi.obbs(name), rg, ro)


@functools.lru_cache(maxsize=None)
def _fit():
    Ts, Cs, st = capi.minsnap_batch(tsi.fit_waypoints(), 1.0, 2.0)
    assert (st == 0).all()
    return Ts, Cs


# ---- 1. edges against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("name", fi.WORLDS)
def test_motions_equal_restatement_and_check_motions(name):
    world = _world(name)
    counts = fi.EDGE_COUNTS + ((fi.MANY,) if name in fi.MANY_WORLDS else ())
    for cp in fi.CAN_PASS:
        for n in counts:
            s1, s2 = fi.edges(name, n)
            exp_t, exp_obb = fi.expected(name, n, cp)
            t, obb = world.first_hits(s1, s2, cp)
            assert t.dtype == np.float64 and obb.dtype == np.int32 and len(t) == n == len(obb)
            bad = np.flatnonzero((t != exp_t) | (obb != exp_obb))
            print(f"{name} OBBs, can_pass {cp}, {n} edges: blocked {int((obb >= 0).sum())}, differing {len(bad)}"
                  f" {bad[:8].tolist()} got {t[bad[:8]].tolist()} {obb[bad[:8]].tolist()}"
                  f" want {exp_t[bad[:8]].tolist()} {exp_obb[bad[:8]].tolist()}")
            assert np.array_equal(t, exp_t) and np.array_equal(obb, exp_obb)
            flags = world.check_motions(s1, s2, cp, 0)
            assert np.array_equal(obb >= 0, flags == 0)
    if name == "filling":
        assert (obb == -1).all() and np.isinf(t).all()  # (can_pass: every OBB is skipped)


def test_motions_obb_is_optional():
    world = _world("72")
    s1, s2 = fi.edges("72", 65)
    d1, d2 = capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
    d_t = capi.DeviceBuffer(8 * len(s1))
    capi.check(capi.lib().epp_motions_first_hit(world.handle, d1.ptr, d2.ptr, len(s1), 0, d_t.ptr, None, None))
    capi.sync()
    assert np.array_equal(d_t.download(np.float64, len(s1)), fi.expected("72", 65, False)[0])


def test_motions_after_world_update():
    fgeom, rg, ro = spi.setup()
    s1, s2 = fi.edges("72", fi.BLOCK + 1)
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    before = world.first_hits(s1, s2, False)
    moved = capi.build_obbs(fgeom, *spi.poses(72, moved=True))
    world.update(moved)  # (a gate moved; no build_index: the call rebuilds it)
    got = world.first_hits(s1, s2, False)
    exp = fi.fr.edges(fi.fr.world(moved, rg, ro), rg, ro, s1, s2, False)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert not np.array_equal(got[0], before[0])  # (the move changes answers)


def test_motions_graph_replay():
    fgeom, rg, ro = spi.setup()
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    world.build_index()
    s1, s2 = fi.edges("72", fi.BLOCK + 1)
    n = len(s1)
    exp = fi.expected("72", n, True)
    L = capi.lib()
    d1, d2 = capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
    d_t, d_obb = capi.DeviceBuffer(8 * n), capi.DeviceBuffer(4 * n)
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_motions_first_hit(world.handle, d1.ptr, d2.ptr, n, 1, d_t.ptr, d_obb.ptr, s.value))
    capi.check(L.epp_graph_end(s.value, C.byref(g)))
    for _ in range(2):
        capi.check(L.epp_memset(d_t.ptr, 0x5A, 8 * n, None))  # poison
        capi.check(L.epp_memset(d_obb.ptr, 0x5A, 4 * n, None))
        capi.sync()
        capi.check(L.epp_graph_launch(g.value, s.value))
        capi.check(L.epp_stream_sync(s.value))
        assert np.array_equal(d_t.download(np.float64, n), exp[0])
        assert np.array_equal(d_obb.download(np.int32, n), exp[1])
    capi.check(L.epp_graph_destroy(g.value))
    L.epp_stream_destroy(s.value)


# ---- 2. the fused call against the composition --------------------------------------------------
def _compose(world, Ts, Cs, dt, cp):
    """The definition: the sweep's chord, then epp_motions_first_hit on its two sampled rows and
    the time formula on the sampled time column (numpy: one subtract, one multiply, one add)."""
    rows, roff = _sample(Ts, Cs, dt)
    chord = world.sweep_trajectories(Ts, Cs, dt, cp)[0]
    nt = len(Ts)
    t, time, obb = np.full(nt, np.inf), np.full(nt, -1.0), np.full(nt, -1, np.int32)
    bad = np.flatnonzero(chord >= 0)
    if len(bad):
        j = roff[bad] + chord[bad]
        assert (chord[bad] + 1 < np.diff(roff)[bad]).all()
        t[bad], obb[bad] = world.first_hits(rows[j][:, [0, 3, 6]], rows[j + 1][:, [0, 3, 6]], cp)
        tj, tj1 = rows[j, 9], rows[j + 1, 9]
        time[bad] = tj + t[bad] * (tj1 - tj)
    return chord, t, time, obb


def _assert_equals_composition(world, Ts, Cs, dt, cp):
    exp = _compose(world, Ts, Cs, dt, cp)
    got = world.trajectory_first_hits(Ts, Cs, dt, cp)
    assert [g.dtype for g in got] == [np.int64, np.float64, np.float64, np.int32]
    for g, e, what in zip(got, exp, ("chord", "t_hit", "time", "obb")):
        assert np.array_equal(g, e), (what, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    chord, t, time, obb = got
    hit = chord >= 0
    assert ((obb >= 0) == hit).all() and ((t >= 0) & (t <= 1))[hit].all()
    assert np.isinf(t[~hit]).all() and (time[~hit] == -1.0).all()
    return got


@pytest.mark.parametrize("n_obb", [3, 72, 300])
def test_tracks_equal_composition(n_obb):
    world, _ = _fit_world(n_obb)
    Ts, Cs = _fit()
    assert len(Ts) == 64 and {len(t) for t in Ts} == set(range(1, 13))
    for dt in (0.01, 0.1):
        for cp in tsi.CAN_PASS:
            chord = _assert_equals_composition(world, Ts, Cs, dt, cp)[0]
            print(f"{n_obb} OBBs dt {dt} can_pass {cp}: chords {chord.tolist()}")
            assert (chord >= 0).sum() >= 8
            if n_obb == 72:
                assert (chord == -1).sum() >= 8


def test_track_edges():
    """trajsweep_inputs' straight tracks through the pole: a failure at chord 0, at the chord
    that spans two chunks (kRowChunk - 1 | kRowChunk), at the last chord, tracks that never
    fail; with them a track of more than kTcSegLds segments and one with the NaN times of a
    failed fit.  One launch, then each failing one in a launch of its own (n_tracks = 1)."""
    names, Ts, Cs, want = tsi.edge_tracks()
    cx, cy = (float(v) for v in tsi.thin_ref()[0]["center"][:2])
    n_seg = K_SEG_LDS + 1  # rows 0..5 in segment 0 (5.5 DT long), the pole between rows 20 and 21
    names = names + [f"{n_seg} segments", "NaN times"]
    Ts = Ts + [np.full(n_seg, 5.5 * tsi.DT), np.full(2, np.nan)]
    Cs = Cs + [tsi.linear(cx - 20.5 * tsi.STEP, tsi.V, cy, tsi.Z, n_seg, 5.5 * tsi.DT), np.full((2, 3, 10), np.nan)]
    want = want + [20, -1]
    _, rg, ro = spi.setup()
    world = capi.World(tsi.thin_obbs(), rg, ro)
    for cp in tsi.CAN_PASS:
        got = _assert_equals_composition(world, Ts, Cs, tsi.DT, cp)
        print("edges:", list(zip(names, got[0].tolist(), got[1].tolist())))
        assert got[0].tolist() == want
        for k, name in enumerate(names):
            if want[k] < 0:
                assert (got[0][k], got[1][k], got[2][k], got[3][k]) == (-1, np.inf, -1.0, -1), name
            else:  # rows 0.4 m before / behind the pole's centre, both outside its inflated box
                assert got[3][k] == 0 and 0.0 < got[1][k] < 0.5, name
    for k in range(len(Ts)):
        if want[k] >= 0:
            alone = world.trajectory_first_hits(Ts[k:k + 1], Cs[k:k + 1], tsi.DT, True)
            assert all(a[0] == g[k] for a, g in zip(alone, got)), names[k]


def test_more_tracks_than_workgroups():
    """2560 tracks: the persistent grid has at most 8 workgroups per CU, so every workgroup
    takes several tracks and keeps no state from one to the next."""
    world, _ = _fit_world(72)
    Ts, Cs = _fit()
    got = _assert_equals_composition(world, Ts * 40, Cs * 40, 0.1, False)
    first = [g[:64] for g in got]
    assert (first[0] >= 0).any() and (first[0] == -1).any()
    for r in range(1, 40):
        assert all(np.array_equal(g[64 * r:64 * (r + 1)], f) for g, f in zip(got, first))


def test_tracks_optional_outputs_may_be_null():
    world, _ = _fit_world(72)
    Ts, Cs = _fit()
    nt = len(Ts)
    full = world.trajectory_first_hits(Ts, Cs, 0.1, False)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_chord, d_t = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt)
    capi.check(capi.lib().epp_traj_first_hit_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, 0.1, 0, d_chord.ptr,
                                                   d_t.ptr, None, None, None))
    capi.sync()
    assert np.array_equal(d_chord.download(np.int64, nt), full[0])
    assert np.array_equal(d_t.download(np.float64, nt), full[1])


# ---- 3. C++ / pybind ----------------------------------------------------------------------------
def test_path_planner_candidate_first_hits():
    import online_traj_planner as otp
    gates, obstacles = spi.poses(72)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    sets = tsi.fit_waypoints()[:16]
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    world, _ = _fit_world(72)
    for cp in tsi.CAN_PASS:
        exp = world.trajectory_first_hits(Ts, Cs, 0.1, cp)
        got = pp.candidate_first_hits(sets, 1.0, 2.0, 0.1, cp)
        assert [g.dtype for g in got] == [np.int64, np.float64, np.float64, np.int32]
        assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    assert (got[0] >= 0).any() and (got[0] == -1).any()
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_first_hits([sets[0], sets[1][:1]], 1.0, 2.0, 0.1, False)
    assert [len(r) for r in pp.candidate_first_hits([], 1.0, 2.0, 0.1, False)] == [0, 0, 0, 0]


def test_world_first_hits_host_arrays():
    """World::firstHits through the zero-copy and the staged query path (pybind: first_hits)."""
    import online_traj_planner as otp
    gates, obstacles = spi.poses(72)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    for n in (1, 257, 20000):  # one edge, zero-copy, staged through HBM
        s1, s2 = fi.edges("72", n)
        for cp in fi.CAN_PASS:
            t, obb = pp.first_hits(s1, s2, cp)
            exp = fi.expected("72", n, cp)
            assert t.dtype == np.float64 and obb.dtype == np.int32
            assert np.array_equal(t, exp[0]) and np.array_equal(obb, exp[1])
