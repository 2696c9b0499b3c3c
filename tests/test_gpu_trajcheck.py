"""GPU: epp_traj_check_batch, the first collision of fitted trajectories straight from their
coefficients (PathPlanner::checkTrajectoryValidity, src/PathPlanner.cpp:267-280, per track),
and its Python / PathPlanner layers.

By definition the answer is what the existing pieces give on the same device -- the rows of
epp_sample_count + epp_sample_batch, their columns 0 / 3 / 6 through
epp_check_states_mindist, the first zero flag per track -- so both outputs are compared with
that composition with ==.  Against the CPU oracle a track takes part only if the oracle's
flags at md - 1e-9 and md + 1e-9 agree on every row (the oracle's Horner order differs from
the device's fused one by ~1e-15 in the position); at least 90 % of the tracks must.

Worlds: configs/config_filling.json geometry, 72 OBBs (synth.track_world(42)), 3 OBBs (under
the small-query kernels' limit) and 300 OBBs (above it: the composition's check runs on the
index kernels there).  Tracks: fitted on the GPU with capi.minsnap_batch(tracks, 1.0, 2.0).
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle as O
import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi, synth

from conftest import PKG

pytestmark = pytest.mark.gpu

DT = 0.05
MDS = (0.05, 0.2)
OBBS = (72, 3, 300)
K_ROW_CHUNK = int(re.search(r"kRowChunk = (\d+);", open(os.path.join(PKG, "csrc", "traj_sample.h")).read()).group(1))


@functools.lru_cache(maxsize=None)
def _poses(n_obb):
    if n_obb == 72:
        return synth.track_world(42)
    if n_obb == 3:
        return synth.track_world(103, n_gates=0, n_obstacles=3)
    assert n_obb == 300
    return synth.track_world(7, n_gates=8, n_obstacles=252)


@functools.lru_cache(maxsize=None)
def _world(n_obb):
    """(capi.World, the oracle's world); shared and left unchanged."""
    fgeom, rg, ro = spi.setup()
    gates, obstacles = _poses(n_obb)
    obbs = capi.build_obbs(fgeom, gates, obstacles)
    assert len(obbs) == n_obb
    return capi.World(obbs, rg, ro), O.world_build(fgeom, gates, obstacles, rg, ro)


@functools.lru_cache(maxsize=None)
def _fit(name):
    """"ragged": 24 tracks of 1..30 segments (~28.8k rows at DT); "long": 16 tracks of 41
    segments (past the fit's 40-segment LDS kernel and this kernel's LDS copy of the times)."""
    if name == "ragged":
        tracks = [synth.random_track_waypoints(900 + k, 1 + (k * 7) % 30) for k in range(24)]
    else:
        tracks = [synth.random_track_waypoints(4100 + k, 41) for k in range(16)]
    Ts, Cs, st = capi.minsnap_batch(tracks, 1.0, 2.0)
    assert (st == 0).all()
    return Ts, Cs


def _sample(Ts, Cs, dt):
    """(rows per track, row offsets, all rows) from epp_sample_count + epp_sample_batch
    (capi.sample_count / capi.sample_batch; the sampler itself is pinned by
    test_gpu_sample_batch.py)."""
    cnt = capi.sample_count(Ts, dt)
    roff = np.zeros(len(Ts) + 1, np.int64)
    roff[1:] = np.cumsum(cnt)
    rows = capi.sample_batch(Ts, Cs, dt)
    assert len(rows) == roff[-1]
    return cnt, roff, rows


def _compose(world, Ts, Cs, dt, md):
    """The definition: sample count -> rows -> minDistance flags -> first zero per track."""
    nt = len(Ts)
    cnt, roff, rows = _sample(Ts, Cs, dt)
    total = len(rows)
    flags = world.check_states_mindist(rows[:, [0, 3, 6]], md) if total else np.zeros(0, np.uint8)
    first = np.full(nt, -1, np.int64)
    time = np.full(nt, -1.0)
    for k in range(nt):
        bad = np.flatnonzero(flags[roff[k]:roff[k + 1]] == 0)
        if len(bad):
            first[k] = bad[0]
            time[k] = rows[roff[k] + bad[0], 9]
    return first, time, cnt


def _oracle(ref, Ts, Cs, dt, md):
    """(first row, its time, takes part) per track from the CPU oracle."""
    nt = len(Ts)
    first = np.full(nt, -1, np.int64)
    time = np.full(nt, -1.0)
    robust = np.ones(nt, bool)
    for k in range(nt):
        if len(Ts[k]) == 0:
            continue
        rows = O.sample_traj(Ts[k], Cs[k], dt)
        if len(rows) == 0:
            continue
        xyz = rows[:, [0, 3, 6]]
        f = O.check_states_mindist(ref, xyz, md)
        robust[k] = (np.array_equal(O.check_states_mindist(ref, xyz, md - 1e-9), f)
                     and np.array_equal(O.check_states_mindist(ref, xyz, md + 1e-9), f))
        bad = np.flatnonzero(f == 0)
        if len(bad):
            first[k] = bad[0]
            time[k] = rows[bad[0], 9]
    return first, time, robust


def _assert_equals_oracle(got, ref, Ts, Cs, dt, md, min_part=0.9):
    first, time, robust = _oracle(ref, Ts, Cs, dt, md)
    print(f"md {md}: oracle first rows {first.tolist()}, taking part {int(robust.sum())}/{len(robust)}")
    print(f"         got {got[0].tolist()}")
    assert robust.mean() >= min_part
    assert np.array_equal(got[0][robust], first[robust])
    assert np.array_equal(got[1][robust], time[robust])
    return first


# ---- 1. equals the composition, exactly --------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "long"])
@pytest.mark.parametrize("n_obb", OBBS)
def test_equals_composition(n_obb, name):
    world, _ = _world(n_obb)
    Ts, Cs = _fit(name)
    for md in MDS:
        exp_first, exp_time, cnt = _compose(world, Ts, Cs, DT, md)
        first, time = world.check_trajectories(Ts, Cs, DT, md)
        print(f"{n_obb} OBBs {name} md {md}: {int(cnt.sum())} rows, first {first.tolist()}")
        assert first.dtype == np.int64 and time.dtype == np.float64
        assert np.array_equal(first, exp_first)
        assert np.array_equal(time, exp_time)
        assert ((first == -1) == (time == -1.0)).all() and (first < cnt).all()
    if name == "ragged":
        assert 28000 < cnt.sum() < 30000


def test_front_through_l2_equals_composition(monkeypatch):
    """EPP_TRAJCHECK_STAGE=0: the world's front read through L2 instead of its LDS copy (what a
    world of more than ~1000 OBBs takes)."""
    world, _ = _world(72)
    Ts, Cs = _fit("ragged")
    exp_first, exp_time, _ = _compose(world, Ts, Cs, DT, 0.05)
    monkeypatch.setenv("EPP_TRAJCHECK_STAGE", "0")
    first, time = world.check_trajectories(Ts, Cs, DT, 0.05)
    assert np.array_equal(first, exp_first) and np.array_equal(time, exp_time)


# ---- 2. equals the CPU oracle -------------------------------------------------------------
@pytest.mark.parametrize("n_obb", OBBS)
def test_equals_oracle(n_obb):
    world, ref = _world(n_obb)
    Ts, Cs = _fit("ragged")
    firsts = {}
    for md in MDS:
        firsts[md] = _assert_equals_oracle(world.check_trajectories(Ts, Cs, DT, md), ref, Ts, Cs, DT, md)
    # the inputs exercise every path (what the oracle gives on its own fits)
    if n_obb == 72:
        f = firsts[0.05]
        assert (f == -1).sum() >= 4 and (f >= 0).sum() >= 12
        assert f[f >= 0].min() < K_ROW_CHUNK and f.max() >= 2 * K_ROW_CHUNK  # several chunks
    elif n_obb == 300:
        assert (firsts[0.2] == 0).any()  # fails at row 0
    else:
        assert (firsts[0.05] == -1).sum() >= 18  # mostly valid


# ---- 3. chunk and wave edges --------------------------------------------------------------
def _linear(x0, vx, y, z):
    c = np.zeros((1, 3, 10))
    c[0, 0, :2] = (x0, vx)
    c[0, 1, 0] = y
    c[0, 2, 0] = z
    return c


def _entry_face(ref, md):
    """(x, y, z): where the line (y, z) along +x enters the 3-OBB world's last obstacle at md."""
    ob = ref[2]
    y, z = float(ob["center"][1]), 0.5
    # by bisection on the oracle's predicate
    lo, hi = float(ob["center"][0]) - 1.0, float(ob["center"][0])
    probe = lambda x: O.check_states_mindist(ref, np.array([[x, y, z]]), md)[0]
    assert probe(lo) == 1 and probe(hi) == 0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if probe(mid) else (lo, mid)
    return hi, y, z


def test_chunk_and_wave_edges():
    """One-segment linear tracks x = x0 + v t flying along +x into one obstacle of the 3-OBB
    world, x0 solved on the CPU so that the first failing row is R; tracks that stay valid
    through exactly kRowChunk and kRowChunk + 1 rows; valid neighbours in between; one launch."""
    world, ref = _world(3)
    md, v = 0.05, 0.1
    step = v * DT
    face, y, z = _entry_face(ref, md)
    Rs = [0, 1, 63, 64, K_ROW_CHUNK - 1, K_ROW_CHUNK, K_ROW_CHUNK + 1]
    Ts, Cs, want = [], [], []
    far = _linear(face - 4.0, -v, y, z)  # flies away from the obstacle: valid
    for R in Rs:
        # row R (time ~ R dt) half a step past the face, row R - 1 half a step before it
        Ts += [np.array([(R + 20.5) * DT]), np.array([3.0])]
        Cs += [_linear(face - R * step + 0.5 * step, v, y, z), far]
        want += [R, -1]
    for n_rows in (K_ROW_CHUNK, K_ROW_CHUNK + 1):  # valid through exactly n_rows rows
        Ts += [np.array([(n_rows - 0.5) * DT]), np.array([3.0])]
        Cs += [_linear(face - (n_rows + 1) * step, v, y, z), far]
        want += [-1, -1]
        assert len(O.sample_traj(Ts[-2], Cs[-2], DT)) == n_rows
    first, time, robust = _oracle(ref, Ts, Cs, DT, md)
    assert robust.all() and first.tolist() == want  # (the inputs are what they are meant to be)
    got_first, got_time = world.check_trajectories(Ts, Cs, DT, md)
    print("edges:", got_first.tolist())
    assert np.array_equal(got_first, first)
    assert np.array_equal(got_time, time)


def test_four_consumers_of_the_stepping_loop_agree_at_its_cap_edges():
    """epp_sample_count, epp_sample_batch, epp_traj_check_batch and epp_traj_sweep_batch step
    the recurrence with one loop (traj_sample.h), eight samples at once while eight more fit in
    a chunk: one-segment linear tracks of 1, 8, 9 and kRowChunk + 1 rows flying into an obstacle
    of the 3-OBB world beside a 30-segment fitted track, one batch.  The counts and the time
    column are the oracle's, and a failing row's or chord's time is that column's entry."""
    world, ref = _world(3)
    md, v = 0.05, 0.1
    step = v * DT
    face, y, z = _entry_face(ref, md)
    fit_T, fit_C = _fit("ragged")
    n_rows = [1, 8, 9, K_ROW_CHUNK + 1]
    # the last row half a step past the face (the 1-row track: its only row)
    Ts = [np.array([(n - 0.5) * DT]) for n in n_rows] + [fit_T[17]]
    Cs = [_linear(face - (n - 1) * step + 0.5 * step, v, y, z) for n in n_rows] + [fit_C[17]]
    assert len(Ts[-1]) == 30
    ref_rows = [O.sample_traj(T, Cf, DT) for T, Cf in zip(Ts, Cs)]
    assert [len(r) for r in ref_rows[:4]] == n_rows
    cnt, roff, rows = _sample(Ts, Cs, DT)
    assert cnt.tolist() == [len(r) for r in ref_rows]
    assert np.array_equal(rows[:, 9], np.concatenate([r[:, 9] for r in ref_rows]))
    # (the inputs are what they are meant to be: rows and chords fail, on the oracle alone)
    o_row = _oracle(ref, Ts, Cs, DT, md)[0]
    o_chord = tsi.oracle_sweep(ref, Ts, Cs, DT, False)[0]
    print("oracle rows", o_row.tolist(), "chords", o_chord.tolist())
    assert o_row[:4].tolist() == [n - 1 for n in n_rows] and (o_chord >= 0).any()
    for name, (first, time) in (("check", world.check_trajectories(Ts, Cs, DT, md)),
                                ("sweep", world.sweep_trajectories(Ts, Cs, DT, False))):
        print(name, first.tolist(), time.tolist())
        bad = np.flatnonzero(first >= 0)
        assert len(bad) and (first < cnt).all() and (time[first < 0] == -1.0).all()
        assert np.array_equal(time[bad], rows[roff[bad] + first[bad], 9])


# ---- 4. degenerate tracks -----------------------------------------------------------------
def test_degenerate_tracks_beside_ordinary_ones():
    world, _ = _world(72)
    Ts, Cs = _fit("ragged")
    nan_c = np.full((2, 3, 10), np.nan)
    mixTs = [Ts[0], np.zeros(0), Ts[1], np.array([1.0, 0.5]), Ts[2], np.full(2, np.nan), Ts[4], np.zeros(0)]
    mixCs = [Cs[0], np.zeros((0, 3, 10)), Cs[1], nan_c, Cs[2], nan_c, Cs[4], np.zeros((0, 3, 10))]
    for md in MDS:
        exp_first, exp_time, cnt = _compose(world, mixTs, mixCs, DT, md)
        first, time = world.check_trajectories(mixTs, mixCs, DT, md)
        assert np.array_equal(first, exp_first) and np.array_equal(time, exp_time)
        assert cnt[1] == 0 and cnt[3] > 0 and first[1] == first[3] == first[5] == first[7] == -1
        # the ordinary neighbours: as in a batch of their own
        alone = world.check_trajectories([Ts[0], Ts[1], Ts[2], Ts[4]], [Cs[0], Cs[1], Cs[2], Cs[4]], DT, md)
        assert np.array_equal(first[::2], alone[0]) and np.array_equal(time[::2], alone[1])
        assert (alone[0] >= 0).any()


# ---- 5. world update ----------------------------------------------------------------------
def test_after_world_update():
    fgeom, rg, ro = spi.setup()
    Ts, Cs = _fit("ragged")
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    before = world.check_trajectories(Ts, Cs, DT, 0.05)
    gates, obstacles = spi.poses(72, moved=True)
    world.update(capi.build_obbs(fgeom, gates, obstacles))  # (no build_index: the call rebuilds it)
    got = world.check_trajectories(Ts, Cs, DT, 0.05)
    ref = O.world_build(fgeom, gates, obstacles, rg, ro)
    _assert_equals_oracle(got, ref, Ts, Cs, DT, 0.05)
    assert not np.array_equal(got[0], before[0])  # (the move changes answers)


# ---- 6. graph replay ----------------------------------------------------------------------
def test_graph_replay():
    fgeom, rg, ro = spi.setup()
    Ts, Cs = _fit("ragged")
    world = capi.World(capi.build_obbs(fgeom, *spi.poses(72)), rg, ro)
    world.build_index()
    direct = world.check_trajectories(Ts, Cs, DT, 0.05)
    L = capi.lib()
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_row, d_time = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt)
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_traj_check_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, DT, 0.05, d_row.ptr, d_time.ptr,
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
    Ts, Cs = _fit("ragged")
    nt = len(Ts)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_row = capi.DeviceBuffer(8 * nt)
    capi.check(capi.lib().epp_traj_check_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, DT, 0.05, d_row.ptr, None,
                                               None))
    capi.sync()
    assert np.array_equal(d_row.download(np.int64, nt), world.check_trajectories(Ts, Cs, DT, 0.05)[0])


# ---- 7. API layers ------------------------------------------------------------------------
def test_path_planner_check_candidate_trajectories():
    import online_traj_planner as otp
    fgeom, rg, ro = spi.setup()
    gates, obstacles = spi.poses(72)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    sets = [synth.random_track_waypoints(900 + k, 1 + (k * 7) % 30) for k in range(8)]
    rows, times = pp.check_candidate_trajectories(sets, 1.0, 2.0, DT, 0.05)
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    world, _ = _world(72)
    exp = world.check_trajectories(Ts, Cs, DT, 0.05)
    assert rows.dtype == np.int64 and np.array_equal(rows, exp[0]) and np.array_equal(times, exp[1])
    assert (rows >= 0).any() and (rows == -1).any()
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.check_candidate_trajectories([sets[0], sets[1][:1]], 1.0, 2.0, DT, 0.05)
    assert [len(r) for r in pp.check_candidate_trajectories([], 1.0, 2.0, DT, 0.05)] == [0, 0]
