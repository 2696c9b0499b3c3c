"""GPU: gate passage (include/epp.h): epp_gates_crossed, the gates each straight edge crosses,
and epp_traj_gate_pass_batch, the gates the chords of fitted tracks pass in order, with split
times and offsets, straight from their coefficients; and the Python / PathPlanner /
OnlineTrajGenerator layers.

The edge masks must equal the restatement (gatepass_ref.py: the same IEEE operations in the same
association) with np.array_equal.  By definition the fused call is epp_sample_batch, then
epp_gates_crossed on rows j, j + 1, then the ordered loop, then t_j + u * (t_j+1 - t_j) on the
sampled time column in numpy: every output is compared with that composition with ==.

Tracks, frame tables and edge sets: gatepass_inputs.py (its claims are checked on the CPU in
test_gatepass_inputs_cpu.py).
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import gatepass_inputs as gi
import gatepass_ref as gr
from conftest import CONFIG
from eppamd import capi, synth
from test_gpu_trajsweep import _sample

pytestmark = pytest.mark.gpu


# ---- 1. edges against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("G", gi.GATE_COUNTS)
def test_edges_equal_restatement(G):
    frames = gi.random_frames(G)
    for n in gi.EDGE_COUNTS:
        s1, s2 = gi.random_edges(n, G)
        want = gr.masks(gr.cross(frames, gi.HE, s1, s2)["crossed"])
        got = capi.gates_crossed(frames, gi.HE, s1, s2)
        assert got.dtype == np.uint64 and len(got) == n
        print(f"{G} gates, {n} edges: crossing {int((got != 0).sum())}, differing {int((got != want).sum())}")
        assert np.array_equal(got, want)


def test_edges_exact_cases_no_gates_and_no_edges():
    s1, s2, want = gi.exact_edges()
    got = capi.gates_crossed(gi.FR1, gi.HE, s1, s2)
    assert np.array_equal(got, want.astype(np.uint64)), got
    # n_gates == 0 writes zeros (over poison)
    L = capi.lib()
    n = len(s1)
    d1, d2 = capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
    d_m = capi.DeviceBuffer(8 * n)
    capi.check(L.epp_memset(d_m.ptr, 0x5A, 8 * n, None))
    capi.check(L.epp_gates_crossed(None, 0, gi.HE, d1.ptr, d2.ptr, n, d_m.ptr, None))
    capi.sync()
    assert (d_m.download(np.uint64, n) == 0).all()
    # n == 0 launches nothing
    assert len(capi.gates_crossed(gi.FR1, gi.HE, np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    capi.check(L.epp_memset(d_m.ptr, 0x5A, 8 * n, None))
    capi.check(L.epp_gates_crossed(None, 0, gi.HE, None, None, 0, d_m.ptr, None))
    capi.sync()
    assert (d_m.download(np.uint8, 8 * n) == 0x5A).all()


# ---- 2. the fused call against the composition --------------------------------------------------
def _compose(frames, half_edge, Ts, Cs, dt):
    """The definition: the sampled rows, epp_gates_crossed on every pair of consecutive rows of
    a track (one call for all), the ordered loop per track, u and the offsets by the
    restatement on the chosen rows and the time formula in numpy."""
    rows, roff = _sample(Ts, Cs, dt)
    nt, G = len(Ts), len(frames)
    first = np.concatenate([np.arange(roff[k], max(roff[k + 1] - 1, roff[k])) for k in range(nt)] + [np.zeros(0, int)])
    first = first.astype(np.int64)
    xyz = rows[:, [0, 3, 6]]
    m = capi.gates_crossed(frames, half_edge, xyz[first], xyz[first + 1]) if len(first) else np.zeros(0, np.uint64)
    bits = ((m[:, None] >> np.arange(G, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)
    chord, time = np.full((nt, G), -1, np.int64), np.full((nt, G), -1.0)
    off, n_passed = np.full((nt, G, 2), np.nan), np.zeros(nt, np.int32)
    o = 0
    for k in range(nt):
        nc = max(int(roff[k + 1] - roff[k]) - 1, 0)
        chord[k], time[k], off[k], n_passed[k] = gr.passes(frames, half_edge, rows[roff[k]:roff[k + 1]],
                                                           bits[o:o + nc])
        o += nc
    return chord, time, off, n_passed


def _assert_equals_composition(frames, Ts, Cs, dt, half_edge=gi.HE):
    exp = _compose(frames, half_edge, Ts, Cs, dt)
    got = capi.trajectory_gate_passes(frames, half_edge, Ts, Cs, dt)
    assert [g.dtype for g in got] == [np.int64, np.float64, np.float64, np.int32]
    for g, e, what in zip(got, exp, ("chord", "time", "offset", "n_passed")):
        assert g.shape == e.shape, what
        same = (g == e) | ((g != g) & (e != e))  # (an unpassed gate's offsets are NaN in both)
        assert same.all(), (what, np.argwhere(~same)[:8].tolist(), g[~same][:8], e[~same][:8])
    chord, time, off, n_passed = got
    passed = chord >= 0
    assert np.array_equal(passed.sum(axis=1), n_passed) and (np.diff(passed.astype(int), axis=1) <= 0).all()
    assert (time[~passed] == -1.0).all() and np.isnan(off[~passed]).all() and np.isfinite(off[passed]).all()
    assert (np.abs(off[passed]) <= half_edge).all()
    return got


def test_single_gate_track_edges():
    """Every bookkeeping edge of the walk against one gate, in one launch, then each track in a
    launch of its own (n_tracks = 1)."""
    names, Ts, Cs, want = gi.single_gate_tracks()
    got = _assert_equals_composition(gi.FR1, Ts, Cs, gi.DT)
    print("edges:", list(zip(names, got[0][:, 0].tolist(), got[1][:, 0].tolist())))
    assert got[0][:, 0].tolist() == want.tolist()
    hit = want >= 0
    # rows J, J + 1 half a step before / behind the plane: the split time is (J + 0.5) DT exactly
    assert np.array_equal(got[1][hit, 0], (want[hit] + 0.5) * gi.DT)
    for k, name in enumerate(names):
        alone = capi.trajectory_gate_passes(gi.FR1, gi.HE, Ts[k:k + 1], Cs[k:k + 1], gi.DT)
        for a, g in zip(alone, got):
            assert np.array_equal(a[0], g[k], equal_nan=True), name


@pytest.mark.parametrize("case", gi.multi_gate_cases(), ids=lambda c: c[0])
def test_multi_gate_cases(case):
    name, frames, Ts, Cs, want = case
    got = _assert_equals_composition(frames, Ts, Cs, gi.DT)
    assert np.array_equal(got[0], want), got[0]
    assert np.array_equal(got[3], (want >= 0).sum(axis=1))


def test_optional_outputs_may_be_null():
    names, Ts, Cs, want = gi.single_gate_tracks()
    nt = len(Ts)
    full = capi.trajectory_gate_passes(gi.FR1, gi.HE, Ts, Cs, gi.DT)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_f = capi.DeviceBuffer.from_array(gi.FR1)
    d_chord, d_np = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(4 * nt)
    capi.check(capi.lib().epp_traj_gate_pass_batch(d_f.ptr, 1, gi.HE, d_T.ptr, d_C.ptr, d_off.ptr, nt, gi.DT,
                                                   d_chord.ptr, None, None, d_np.ptr, None))
    capi.sync()
    assert np.array_equal(d_chord.download(np.int64, nt), full[0][:, 0])
    assert np.array_equal(d_np.download(np.int32, nt), full[3])
    # no gates: nothing to pass, n_passed = 0 (over poison)
    capi.check(capi.lib().epp_memset(d_np.ptr, 0x5A, 4 * nt, None))
    capi.check(capi.lib().epp_traj_gate_pass_batch(None, 0, gi.HE, d_T.ptr, d_C.ptr, d_off.ptr, nt, gi.DT,
                                                   None, None, None, d_np.ptr, None))
    capi.sync()
    assert (d_np.download(np.int32, nt) == 0).all()


def test_more_tracks_than_workgroups():
    """2560 two-row tracks: the persistent grid has at most 8 workgroups per CU, so every
    workgroup takes several tracks and keeps no state from one to the next."""
    Ts, Cs, want = gi.short_tracks(2560)
    got = capi.trajectory_gate_passes(gi.FR1, gi.HE, Ts, Cs, gi.DT)
    assert np.array_equal(got[0][:, 0], want) and np.array_equal(got[3], (want >= 0).astype(np.int32))
    for k in (0, 1):  # the two distinct tracks, each alone, against every copy in the batch
        alone = _assert_equals_composition(gi.FR1, Ts[k:k + 1], Cs[k:k + 1], gi.DT)
        for a, g in zip(alone, got):
            assert (np.array_equal(g[k::2], np.broadcast_to(a[0], g[k::2].shape), equal_nan=True))


# ---- 3. fitted tracks ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit():
    Ts, Cs, st = capi.minsnap_batch(gi.fit_waypoints(), 1.0, 2.0)
    assert (st == 0).all()
    return Ts, Cs


@pytest.mark.parametrize("dt", [0.01, 0.1])
def test_fitted_tracks_equal_composition(dt):
    Ts, Cs = _fit()
    assert len(Ts) == 64 and len(Ts[gi.FIT_ON]) == 12
    rows, _ = _sample(Ts[gi.FIT_ON:gi.FIT_ON + 1], Cs[gi.FIT_ON:gi.FIT_ON + 1], dt)
    frames, at = gi.gates_on_rows(rows)
    chord, time, off, n_passed = _assert_equals_composition(frames, Ts, Cs, dt)
    print(f"dt {dt}: n_passed {n_passed.tolist()}")
    # the track the gates stand on passes all of them, each at (or before) the chord it stands on
    assert n_passed[gi.FIT_ON] == gi.N_FIT_GATES and (chord[gi.FIT_ON] <= at).all()
    assert (np.diff(chord[gi.FIT_ON]) >= 0).all() and (np.diff(time[gi.FIT_ON]) >= 0).all()
    assert (n_passed < gi.N_FIT_GATES).any()


# ---- 4. graph capture, argument errors ----------------------------------------------------------
def test_graph_replay():
    names, Ts, Cs, want = gi.single_gate_tracks()
    nt = len(Ts)
    exp = capi.trajectory_gate_passes(gi.FR1, gi.HE, Ts, Cs, gi.DT)
    s1, s2, crossed = gi.exact_edges()
    n = len(s1)
    L = capi.lib()
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_f, d1, d2 = capi.DeviceBuffer.from_array(gi.FR1), capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
    outs = [capi.DeviceBuffer(b) for b in (8 * nt, 8 * nt, 16 * nt, 4 * nt, 8 * n)]
    d_chord, d_time, d_o, d_np, d_m = outs
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_traj_gate_pass_batch(d_f.ptr, 1, gi.HE, d_T.ptr, d_C.ptr, d_off.ptr, nt, gi.DT, d_chord.ptr,
                                          d_time.ptr, d_o.ptr, d_np.ptr, s.value))
    capi.check(L.epp_gates_crossed(d_f.ptr, 1, gi.HE, d1.ptr, d2.ptr, n, d_m.ptr, s.value))
    capi.check(L.epp_graph_end(s.value, C.byref(g)))
    for _ in range(2):
        for b in outs:
            capi.check(L.epp_memset(b.ptr, 0x5A, b.nbytes, None))  # poison
        capi.sync()
        capi.check(L.epp_graph_launch(g.value, s.value))
        capi.check(L.epp_stream_sync(s.value))
        assert np.array_equal(d_chord.download(np.int64, nt), exp[0][:, 0])
        assert np.array_equal(d_time.download(np.float64, nt), exp[1][:, 0])
        assert np.array_equal(d_o.download(np.float64, 2 * nt), exp[2].ravel(), equal_nan=True)
        assert np.array_equal(d_np.download(np.int32, nt), exp[3])
        assert np.array_equal(d_m.download(np.uint64, n), crossed.astype(np.uint64))
    capi.check(L.epp_graph_destroy(g.value))
    L.epp_stream_destroy(s.value)


def test_argument_errors_leave_outputs_untouched():
    names, Ts, Cs, want = gi.single_gate_tracks()
    Ts, Cs = Ts[:4], Cs[:4]
    nt = 4
    s1, s2, _ = gi.exact_edges()
    n = len(s1)
    L = capi.lib()
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_f, d1, d2 = capi.DeviceBuffer.from_array(gi.FR1), capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
    out = capi.DeviceBuffer(4096)  # every output of every call below lies in here
    capi.check(L.epp_memset(out.ptr, 0x5A, 4096, None))
    capi.sync()
    o = [out.ptr + 1024 * k for k in range(4)]
    nan, inf = float("nan"), float("inf")
    edges = {
        "n_gates < 0": (d_f.ptr, -1, gi.HE, d1.ptr, d2.ptr, n, o[0]),
        "n_gates 65": (d_f.ptr, 65, gi.HE, d1.ptr, d2.ptr, n, o[0]),
        "half_edge < 0": (d_f.ptr, 1, -0.1, d1.ptr, d2.ptr, n, o[0]),
        "half_edge NaN": (d_f.ptr, 1, nan, d1.ptr, d2.ptr, n, o[0]),
        "half_edge inf": (d_f.ptr, 1, inf, d1.ptr, d2.ptr, n, o[0]),
        "n < 0": (d_f.ptr, 1, gi.HE, d1.ptr, d2.ptr, -1, o[0]),
        "NULL gates": (None, 1, gi.HE, d1.ptr, d2.ptr, n, o[0]),
        "NULL s1": (d_f.ptr, 1, gi.HE, None, d2.ptr, n, o[0]),
        "NULL s2": (d_f.ptr, 1, gi.HE, d1.ptr, None, n, o[0]),
    }
    for name, a in edges.items():
        assert L.epp_gates_crossed(*a, None) == capi.EPP_ERR_INVALID_ARGUMENT, name
    assert L.epp_gates_crossed(d_f.ptr, 1, gi.HE, d1.ptr, d2.ptr, n, None, None) == capi.EPP_ERR_INVALID_ARGUMENT
    t = (d_T.ptr, d_C.ptr, d_off.ptr)
    tracks = {
        "n_gates < 0": (d_f.ptr, -1, gi.HE, *t, nt, gi.DT, *o),
        "n_gates 65": (d_f.ptr, 65, gi.HE, *t, nt, gi.DT, *o),
        "half_edge < 0": (d_f.ptr, 1, -0.1, *t, nt, gi.DT, *o),
        "half_edge NaN": (d_f.ptr, 1, nan, *t, nt, gi.DT, *o),
        "half_edge inf": (d_f.ptr, 1, inf, *t, nt, gi.DT, *o),
        "n_tracks < 0": (d_f.ptr, 1, gi.HE, *t, -1, gi.DT, *o),
        "dt == 0": (d_f.ptr, 1, gi.HE, *t, nt, 0.0, *o),
        "dt < 0": (d_f.ptr, 1, gi.HE, *t, nt, -gi.DT, *o),
        "dt NaN": (d_f.ptr, 1, gi.HE, *t, nt, nan, *o),
        "dt inf": (d_f.ptr, 1, gi.HE, *t, nt, inf, *o),
        "NULL gates": (None, 1, gi.HE, *t, nt, gi.DT, *o),
        "NULL seg_times": (d_f.ptr, 1, gi.HE, None, d_C.ptr, d_off.ptr, nt, gi.DT, *o),
        "NULL coeffs": (d_f.ptr, 1, gi.HE, d_T.ptr, None, d_off.ptr, nt, gi.DT, *o),
        "NULL wp_offsets": (d_f.ptr, 1, gi.HE, d_T.ptr, d_C.ptr, None, nt, gi.DT, *o),
        "NULL chord": (d_f.ptr, 1, gi.HE, *t, nt, gi.DT, None, o[1], o[2], o[3]),
        "NULL n_passed": (d_f.ptr, 1, gi.HE, *t, nt, gi.DT, o[0], o[1], o[2], None),
    }
    for name, a in tracks.items():
        assert L.epp_traj_gate_pass_batch(*a, None) == capi.EPP_ERR_INVALID_ARGUMENT, name
    capi.sync()
    assert (out.download(np.uint8, 4096) == 0x5A).all()


# ---- 5. C++ / pybind ----------------------------------------------------------------------------
def test_path_planner_candidate_gate_passes(geom):
    import online_traj_planner as otp
    gates, obstacles = synth.track_world(42)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), CONFIG)
    frames = pp.gate_frames(gates)
    heights = np.array([float(geom.gate_height[int(t)]) for t in gates[:, 6]])
    want = np.column_stack([gates[:, 0], gates[:, 1], gates[:, 2] + heights, np.cos(gates[:, 5]), np.sin(gates[:, 5])])
    assert frames.shape == (len(gates), 5) and np.array_equal(frames[:, :3], want[:, :3])
    assert np.abs(frames[:, 3:] - want[:, 3:]).max() <= 2.0 ** -52  # (std::cos / std::sin against numpy's)
    bad = np.array(gates[:1])
    bad[0, 3] = 0.1
    with pytest.raises(ValueError, match="rotation around z"):
        pp.gate_frames(bad)
    # candidates through the gates: 0.55 m before every gate, its centre, 0.55 m behind it; shifted
    # copies (the last one 3 m above every opening); a short one; the whole lap the wrong way round
    cps = synth.gate_checkpoints(gates, np.array([float(h) for h in geom.gate_height]), 0.55)
    lap = np.concatenate([[cps[2 * g], (cps[2 * g] + cps[2 * g + 1]) / 2, cps[2 * g + 1]] for g in range(len(gates))])
    sets = [lap + [dx, 0.0, dz] for dx, dz in ((0.0, 0.0), (0.05, 0.02), (0.3, -0.1), (0.0, 3.0))] + [lap[:4], lap[::-1]]
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    for he in (gi.HE, 0.2):
        exp = capi.trajectory_gate_passes(frames, he, Ts, Cs, 0.05)
        got = pp.candidate_gate_passes(sets, 1.0, 2.0, 0.05, frames, he)
        assert [g.dtype for g in got] == [np.int64, np.float64, np.float64, np.int32]
        assert [g.shape for g in got] == [(6, 8), (6, 8), (6, 8, 2), (6,)]
        assert all(np.array_equal(g, e, equal_nan=True) for g, e in zip(got, exp))
    print("n_passed:", got[3].tolist())
    # through gate 0's centre along its normal (yaw within 0.3 of 0: see test_online_get_gate_passes);
    # 3 m above every gate
    assert got[3][0] >= 1 and got[3][3] == 0
    assert np.array_equal(pp.candidate_gate_passes(sets, 1.0, 2.0, 0.05, frames)[0],
                          capi.trajectory_gate_passes(frames, gi.HE, Ts, Cs, 0.05)[0])  # half_edge defaults to 0.425
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_gate_passes([sets[0], sets[1][:1]], 1.0, 2.0, 0.05, frames)
    assert [r.shape for r in pp.candidate_gate_passes([], 1.0, 2.0, 0.05, frames)] == [(0, 8), (0, 8), (0, 8, 2), (0,)]


def test_online_get_gate_passes(tmp_path, geom):
    """The planned trajectory of the 8-gate track world: get_gate_passes equals the restatement
    on get_planned_traj().  Gate 0 (yaw within 0.3 of 0) is passed: the trajectory runs from
    0.55 m before its centre through the centre to 0.55 m behind it along the gate normal n, and
    for a point lambda * n from the centre checkGatePassed's frame gives y = lambda cos(2 yaw),
    x = -lambda sin(2 yaw): the sign of lambda, and at the crossing step |x| far below 0.425."""
    import online_traj_planner as otp
    c = json.load(open(CONFIG))
    c["world_properties"]["lower_bound"] = [-6, -6, 0]
    c["world_properties"]["upper_bound"] = [6, 6, 2]
    path = tmp_path / "config.json"
    path.write_text(json.dumps(c))
    gates, obstacles = synth.track_world(42)
    assert abs(gates[0, 5]) < 0.3
    cps = synth.gate_checkpoints(gates, np.array([float(h) for h in geom.gate_height]), 0.55)
    otg = otp.OnlineTrajGenerator(cps[0], cps[-1], gates, obstacles, str(path))
    otg.pre_compute_traj(1.5)
    traj = otg.get_planned_traj()
    rows, times = otg.get_gate_passes()
    assert rows.dtype == np.int64 and times.dtype == np.float64 and len(rows) == len(times) == len(gates)
    frames = otp.PathPlanner(np.array(gates), np.array(obstacles), str(path)).gate_frames(gates)
    chord, time, _, n_passed = gr.passes(frames, gi.HE, traj)
    print("rows", rows.tolist(), "times", times.tolist())
    assert np.array_equal(rows, chord) and np.array_equal(times, time)
    assert rows[0] >= 0 and n_passed >= 1 and traj[rows[0], 9] <= times[0] <= traj[rows[0] + 1, 9]
