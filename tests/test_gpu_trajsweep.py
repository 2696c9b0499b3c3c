"""GPU: epp_traj_sweep_batch, the first failing chord between consecutive rows of fitted
trajectories straight from their coefficients (World::checkRayValid, src/World.cpp:130-162,
on p_j -> p_j+1), and its Python / PathPlanner layers.

By definition the answer is what the existing pieces give on the same device -- the rows of
epp_sample_count + epp_sample_batch, consecutive rows' columns 0 / 3 / 6 of one track through
epp_check_motions (mode 0), the first zero flag -- so both outputs are compared with that
composition with ==.  The motion check runs per track, so tracks of up to 1025 rows are
served by the small-query kernels on the worlds of <= 256 OBBs and longer ones, and every
track on the larger worlds, by the index kernels.  Against the CPU oracle a track takes part
only if the oracle's flags do not change with the inflation radii moved by -1e-9 and +1e-9
(trajsweep_inputs.oracle_sweep); at least 90 % of the tracks must.

Worlds and fits: test_gpu_trajcheck.py's worlds (3, 72 and 300 OBBs), 64 tracks of 1..12
segments fitted on the GPU with capi.minsnap_batch(tracks, 1.0, 2.0); the straight-line
fixtures of trajsweep_inputs.py against the single pole of a 1-OBB world.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi, synth
from test_gpu_trajcheck import _world

pytestmark = pytest.mark.gpu

DTS = (0.01, 0.1)
OBBS = (3, 72, 300)


@functools.lru_cache(maxsize=None)
def _fit():
    Ts, Cs, st = capi.minsnap_batch(tsi.fit_waypoints(), 1.0, 2.0)
    assert (st == 0).all()
    return Ts, Cs


@functools.lru_cache(maxsize=None)
def _thin_world():
    _, rg, ro = spi.setup()
    return capi.World(tsi.thin_obbs(), rg, ro)


def _sample(Ts, Cs, dt):
    """(rows, row offsets) of epp_sample_count + epp_sample_batch (capi.sample_count /
    capi.sample_batch; the sampler itself is pinned by test_gpu_sample_batch.py)."""
    roff = np.zeros(len(Ts) + 1, np.int64)
    roff[1:] = np.cumsum(capi.sample_count(Ts, dt))
    rows = capi.sample_batch(Ts, Cs, dt)
    assert len(rows) == roff[-1]
    return rows, roff


@functools.lru_cache(maxsize=None)
def _fit_rows(dt):
    return _sample(*_fit(), dt)


def _compose(world, rows, roff, can_pass):
    """The definition: per track, consecutive rows -> mode-0 motion flags -> first zero."""
    nt = len(roff) - 1
    first = np.full(nt, -1, np.int64)
    time = np.full(nt, -1.0)
    for k in range(nt):
        r = rows[roff[k]:roff[k + 1]]
        if len(r) < 2:
            continue
        xyz = np.ascontiguousarray(r[:, [0, 3, 6]])
        bad = np.flatnonzero(world.check_motions(xyz[:-1], xyz[1:], can_pass, 0) == 0)
        if len(bad):
            first[k] = bad[0]
            time[k] = r[bad[0], 9]
    return first, time


def _assert_equals_composition(world, Ts, Cs, dt, can_pass, rows=None, roff=None):
    if rows is None:
        rows, roff = _sample(Ts, Cs, dt)
    exp_first, exp_time = _compose(world, rows, roff, can_pass)
    first, time = world.sweep_trajectories(Ts, Cs, dt, can_pass)
    print(f"dt {dt} can_pass {can_pass}: {len(rows)} rows, first {first.tolist()}")
    assert first.dtype == np.int64 and time.dtype == np.float64
    assert np.array_equal(first, exp_first)
    assert np.array_equal(time, exp_time)
    cnt = np.diff(roff)
    assert ((first == -1) == (time == -1.0)).all() and (first < np.maximum(cnt - 1, 0)).all()
    return first


# ---- 1. equals the composition, exactly --------------------------------------------------
@pytest.mark.parametrize("n_obb", OBBS)
def test_equals_composition(n_obb):
    world, _ = _world(n_obb)
    Ts, Cs = _fit()
    assert len(Ts) == 64 and {len(t) for t in Ts} == set(range(1, 13))
    firsts = []
    for dt in DTS:
        rows, roff = _fit_rows(dt)
        for cp in tsi.CAN_PASS:
            firsts.append(_assert_equals_composition(world, Ts, Cs, dt, cp, rows, roff))
    cnt = np.diff(_fit_rows(0.01)[1])
    assert cnt.max() > 2 * 512 and cnt.min() < 512  # several chunks, and less than one
    assert all((f >= 0).sum() >= 8 for f in firsts)
    if n_obb == 72:  # the inputs take both outcomes, and the gates' openings matter
        assert all((f == -1).sum() >= 8 for f in firsts)
        assert not np.array_equal(firsts[0], firsts[1])


@pytest.mark.parametrize("n_obb", [1, 2, 1100])
def test_tiny_and_large_worlds_equal_composition(n_obb):
    """One and two OBBs, and more than 1024 (past the tile filter of the motion kernels and
    past the LDS copy of the cell lists: the staging falls back to the front or to L2)."""
    fgeom, rg, ro = spi.setup()
    gates, obstacles = synth.track_world(500 + n_obb, n_gates=8 if n_obb > 2 else 0,
                                         n_obstacles=n_obb - 48 if n_obb > 2 else n_obb)
    obbs = capi.build_obbs(fgeom, gates, obstacles)
    assert len(obbs) == n_obb
    world = capi.World(obbs, rg, ro)
    Ts, Cs = _fit()
    Ts, Cs = Ts[:24], Cs[:24]
    rows, roff = _sample(Ts, Cs, 0.1)
    for cp in tsi.CAN_PASS:
        first = _assert_equals_composition(world, Ts, Cs, 0.1, cp, rows, roff)
        if n_obb == 1100:
            assert (first >= 0).sum() >= 8


def test_world_through_l2_equals_composition(monkeypatch):
    """EPP_TRAJSWEEP_STAGE = 1 | 0: only the front in LDS, and the whole world read through L2
    (what worlds too large for the LDS copy take)."""
    world, _ = _world(72)
    Ts, Cs = _fit()
    rows, roff = _fit_rows(0.1)
    staged = world.sweep_trajectories(Ts, Cs, 0.1, False)
    assert (staged[0] >= 0).any()
    for level in ("1", "0"):
        monkeypatch.setenv("EPP_TRAJSWEEP_STAGE", level)
        first = _assert_equals_composition(world, Ts, Cs, 0.1, False, rows, roff)
        assert np.array_equal(first, staged[0])


# ---- 2. equals the CPU oracle -------------------------------------------------------------
@pytest.mark.parametrize("n_obb", OBBS)
def test_equals_oracle(n_obb):
    """Observed on the oracle's own fits of these waypoints (CPU, both dt, both can_pass_gate,
    all three worlds): every track takes part (64 / 64 in all 12 cases)."""
    world, ref = _world(n_obb)
    Ts, Cs = _fit()
    for dt in DTS:
        for cp in tsi.CAN_PASS:
            first, time, robust, _ = tsi.oracle_sweep(ref, Ts, Cs, dt, cp)
            got = world.sweep_trajectories(Ts, Cs, dt, cp)
            print(f"{n_obb} OBBs dt {dt} can_pass {cp}: oracle {first.tolist()}, taking part "
                  f"{int(robust.sum())}/{len(robust)}")
            print(f"         got {got[0].tolist()}")
            assert robust.mean() >= 0.9
            assert np.array_equal(got[0][robust], first[robust])
            assert np.array_equal(got[1][robust], time[robust])


# ---- 3. chunk, lane-group and segment edges -------------------------------------------------
def test_chord_edges():
    """The straight-line fixtures (their claims are checked on the CPU in
    test_trajsweep_cpu.py), one launch; also each in a launch of its own."""
    names, Ts, Cs, want = tsi.edge_tracks()
    world = _thin_world()
    for cp in tsi.CAN_PASS:
        exp_first, exp_time, robust, _ = tsi.oracle_sweep(tsi.thin_ref(), Ts, Cs, tsi.DT, cp)
        assert robust.all() and exp_first.tolist() == want
        first, time = world.sweep_trajectories(Ts, Cs, tsi.DT, cp)
        print("edges:", list(zip(names, first.tolist())))
        assert np.array_equal(first, exp_first)
        assert np.array_equal(time, exp_time)
        _assert_equals_composition(world, Ts, Cs, tsi.DT, cp)
    for k in range(0, len(Ts), 2):
        first, time = world.sweep_trajectories(Ts[k:k + 1], Cs[k:k + 1], tsi.DT, False)
        assert first[0] == exp_first[k] and time[0] == exp_time[k], names[k]


# ---- 4. the feature's reason ----------------------------------------------------------------
def test_sweep_catches_what_sampling_misses():
    Ts, Cs, chord = tsi.thin_track()
    world = _thin_world()
    for md in (0.0, 0.1, 0.2):
        rows, times = world.check_trajectories(Ts, Cs, tsi.DT, md)
        assert rows.tolist() == [-1] and times.tolist() == [-1.0]
    for cp in tsi.CAN_PASS:
        first, time = world.sweep_trajectories(Ts, Cs, tsi.DT, cp)
        assert first.tolist() == [chord]
        assert time[0] == O.sample_traj(Ts[0], Cs[0], tsi.DT)[chord, 9]


# ---- 5. degenerate tracks -------------------------------------------------------------------
def test_degenerate_tracks_beside_ordinary_ones():
    world, ref = _world(72)
    Ts, Cs = _fit()
    ordinary = [1, 5, 11, 23]
    nan_c = np.full((2, 3, 10), np.nan)
    none_T, none_C = np.zeros(0), np.zeros((0, 3, 10))
    # a repeated waypoint with its caller-supplied time: free space, and inside an obstacle's
    # inflated box; and the same two places as hand-made constant polynomials
    free = np.array([0.0, 0.0, 1.9])
    inside = np.array(ref[len(ref) - 1]["center"], float)
    rep_C, st = capi.minsnap_batch_times([np.stack([free, free]), np.stack([inside, inside])], [[1.0], [1.0]])
    print("repeated-waypoint fits: status", st.tolist())

    def const(p):
        c = np.zeros((1, 3, 10))
        c[0, :, 0] = p
        return c

    # (a failed fit leaves NaN times and NaN coefficients: no row, so no chord)
    mixTs = [Ts[1], none_T, Ts[5], np.full(1, np.nan), Ts[11], np.full(2, np.nan), Ts[23], none_T,
             np.array([1.0]), np.array([1.0]), np.array([1.0]), np.array([1.0])]
    mixCs = [Cs[1], none_C, Cs[5], nan_c[:1], Cs[11], nan_c, Cs[23], none_C, rep_C[0], rep_C[1], const(free), const(inside)]
    dt = 0.05
    rows, roff = _sample(mixTs, mixCs, dt)
    cnt = np.diff(roff)
    assert cnt[1] == 0 and cnt[3] == 0 and cnt[5] == 0 and cnt[7] == 0
    r10 = rows[roff[10]:roff[11], [0, 3, 6]]
    assert len(r10) >= 19 and (r10 == r10[0]).all()  # zero-length chords
    for cp in tsi.CAN_PASS:
        first = _assert_equals_composition(world, mixTs, mixCs, dt, cp, rows, roff)
        assert first[1] == first[3] == first[5] == first[7] == -1
        assert first[10] == -1 and first[11] == 0
        alone = world.sweep_trajectories([Ts[k] for k in ordinary], [Cs[k] for k in ordinary], dt, cp)
        assert np.array_equal(first[:8:2], alone[0])
    assert (alone[0] >= 0).any()


# ---- 6. world update ------------------------------------------------------------------------
def test_after_world_update():
    fgeom, rg, ro = spi.setup()
    Ts, Cs = _fit()
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    before = world.sweep_trajectories(Ts, Cs, 0.1, False)
    gates, obstacles = spi.poses(72, moved=True)
    world.update(capi.build_obbs(fgeom, gates, obstacles))  # (no build_index: the call rebuilds it)
    got = world.sweep_trajectories(Ts, Cs, 0.1, False)
    ref = O.world_build(fgeom, gates, obstacles, rg, ro)
    first, time, robust, _ = tsi.oracle_sweep(ref, Ts, Cs, 0.1, False)
    assert robust.mean() >= 0.9
    assert np.array_equal(got[0][robust], first[robust]) and np.array_equal(got[1][robust], time[robust])
    assert not np.array_equal(got[0], before[0])  # (the move changes answers)


# ---- 7. graph replay ------------------------------------------------------------------------
def test_graph_replay():
    fgeom, rg, ro = spi.setup()
    Ts, Cs = _fit()
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    world.build_index()
    direct = world.sweep_trajectories(Ts, Cs, 0.1, False)
    L = capi.lib()
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_row, d_time = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt)
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_traj_sweep_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, 0.1, 0, d_row.ptr, d_time.ptr,
                                      s.value))
    capi.check(L.epp_graph_end(s.value, C.byref(g)))
    for _ in range(2):
        capi.check(L.epp_memset(d_row.ptr, 0x5A, 8 * nt, None))  # poison
        capi.check(L.epp_memset(d_time.ptr, 0x5A, 8 * nt, None))
        capi.sync()
        capi.check(L.epp_graph_launch(g.value, s.value))
        capi.check(L.epp_stream_sync(s.value))
        assert np.array_equal(d_row.download(np.int64, nt), direct[0])
        assert np.array_equal(d_time.download(np.float64, nt), direct[1])
    capi.check(L.epp_graph_destroy(g.value))
    L.epp_stream_destroy(s.value)


def test_first_time_is_optional():
    world, _ = _world(72)
    Ts, Cs = _fit()
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_row = capi.DeviceBuffer(8 * nt)
    capi.check(capi.lib().epp_traj_sweep_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, 0.1, 0, d_row.ptr, None,
                                               None))
    capi.sync()
    assert np.array_equal(d_row.download(np.int64, nt), world.sweep_trajectories(Ts, Cs, 0.1, False)[0])


# ---- 8. API layers --------------------------------------------------------------------------
def test_path_planner_sweep_candidate_trajectories():
    import online_traj_planner as otp
    gates, obstacles = spi.poses(72)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    sets = tsi.fit_waypoints()[:16]
    dt, md = 0.1, 0.05
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    world, _ = _world(72)
    exp_rows, exp_row_times = pp.check_candidate_trajectories(sets, 1.0, 2.0, dt, md)
    for cp in tsi.CAN_PASS:
        rows, chords, times = pp.sweep_candidate_trajectories(sets, 1.0, 2.0, dt, md, cp)
        exp_chords, exp_chord_times = world.sweep_trajectories(Ts, Cs, dt, cp)
        assert rows.dtype == np.int64 and chords.dtype == np.int64 and times.dtype == np.float64
        assert np.array_equal(rows, exp_rows) and np.array_equal(chords, exp_chords)
        # the time of the earlier finding
        row_first = (rows >= 0) & ((chords < 0) | (rows <= chords))
        assert np.array_equal(times, np.where(row_first, exp_row_times, exp_chord_times))
    assert (chords >= 0).any() and (chords == -1).any()
    assert np.array_equal(pp.sweep_candidate_trajectories(sets, 1.0, 2.0, dt, md)[1],
                          world.sweep_trajectories(Ts, Cs, dt, False)[0])  # can_pass_gate defaults to False
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.sweep_candidate_trajectories([sets[0], sets[1][:1]], 1.0, 2.0, dt, md, False)
    assert [len(r) for r in pp.sweep_candidate_trajectories([], 1.0, 2.0, dt, md, False)] == [0, 0, 0]
