"""GPU: the min-snap fits at the track lengths where their memory layout changes
(fit_limits_inputs.py): the largest track every entry point takes (the only launches near
kLdsBudget of dynamic LDS), the first it refuses, short tracks beside the largest, the
single-track refit on both sides of its `big` layout with v0 / a0 read from host memory, and the
refit's row slicing at its edges.

What each quantity is held to, and where the numbers come from:
  batch fit    _norm_err(gpu) <= max(_norm_err(oracle), FLOOR) per track against
               minsnap_np.track_batch_refined (the rule of test_batch_vs_truth_short_segment_sweep).
               FLOOR is twice the oracle's own worst distance from that truth over the tracks of
               this module, computed in the test (CPU).  Measured on the CPU: 4.8e-8 at worst
               (41 segments, caller times; 1.4e-8 at 670), so FLOOR = 9.5e-8.  Measured on an
               MI355X: the device's own distance is 3.5e-13 at worst (41 and 670 segments alike),
               and the short tracks of the mixed batch are bit-equal to a short-only batch.
               Continuity of derivatives 0..4 and the end constraints at 1e-6 (the oracle's
               poly_eval).
  refit rows   M <= 276 and the row-slicing cases: sample_batch_ref's bound against the exact
               truth on the batch fit's coefficients; the single-track rows with the existing
               allowance 1e-9 max(1, T_total)^2 more (test_gpu_sample_batch.py section 6).
               Measured on an MI355X, worst error / bound: the batch's rows 0.055; the
               single-track rows before the allowance 19,390 (41 segments), 64,846 (275), 49,651
               (276) and up to 1,008 on the 12-segment row-slicing track (the refit runs
               without the refinement step); the allowances there are 1.1e-5, 4.7e-4, 4.8e-4
               and 1.8e-6, and every row is within bound + allowance.
               M = 4280 (the dense truth is out of reach): every row within 1e-6 of the
               oracle's rows, time column exact, first row the start vertex.  The oracle's
               sparse solve of 4280 segments takes a quarter of an hour on a CPU, so its rows
               for this fixed track are recorded under tests/golden/ and the CPU test holds
               the record to the track.  The issue's position continuity between rows
               (|v| dt + 1e-6) is not asserted: at a few thousand rows over 4280 segments dt
               is longer than a segment, a sampled |v| bounds nothing between two rows, and
               the oracle's own rows break it at 234 of 2500 steps; the 1e-6 against the
               oracle holds every interior row instead (measured on an MI355X: 1.7e-7 at worst).
  gradient, descent   the bounds of test_gpu_time_alloc.py: J within 2 D S of the truth cost
               (time_alloc_ref, S = sum |c Q c|), a gradient entry within 2 (2 D S) / h.  D is
               the reference-arithmetic solve's distance from the truth on these tracks (CPU):
               over every variant of the short tracks, and over the variants of
               fit_limits_inputs.kkt_entries for the largest gradient track / the given times
               for the largest descent track (a dense KKT solve of ~10,000 unknowns each).  A
               truth solve of one variant at 647 segments takes 2.3 s on a CPU and there are
               648, so the largest track's gradient is held at every 16th entry plus the first
               and last two (fit_limits_inputs.held_entries, 44 entries); status and finiteness
               are checked on all.  The descent's step is tr.step_from_grad from the device's
               own gradient at 1e-12 with whichever of the rule's 0..8 halvings the device
               accepted (the CPU's own descent would need all 587 variants' truths), sum T to
               1e-12, coefficients bit for bit epp_minsnap_batch_times at the returned times.
               The largest tracks give the same bits alone and beside short tracks, and the
               short tracks beside them the bits of a short-only batch: asserted (MI355X).
               Measured: D = 0.127 eps of S over the gradient's batch and 0.091 eps over the
               descent's (CPU); on an MI355X the worst |J - truth| / bound 0.21 and
               |g - truth| / bound 0.22 (gradient), |cost0 - truth| / bound 0.30 and
               |cost1 - truth| / bound 0.55 (descent).  The gradient test's CPU truths take
               about 40 s.
test_fit_limits_inputs_cpu.py shows on the CPU that the coefficient rule, the row bound with its
allowance, the 1e-6 of the oracle's rows and the J / g bounds each reject a swapped v0, a dropped
a0 and shifted coefficients.
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import fit_limits_inputs as FI
import minsnap_np as MN
import oracle as O
import sample_batch_ref as SR
import time_alloc_ref as tr
from eppamd import capi

pytestmark = pytest.mark.gpu

LIM = FI.limits()
NAN_WORD = 0x7FF8DEADBEEF0001  # a quiet NaN with a payload no arithmetic produces


def _norm_err(C_, truth, T):
    Tn = np.asarray(T)[:, None, None] ** np.arange(10)[None, None, :]
    return float((np.abs(C_ - truth) * Tn).max() / (np.abs(truth) * Tn).max())


@functools.lru_cache(maxsize=None)
def _case(M, k, caller_times):
    """(wp, T, v0, a0, truth, oracle's distance from it) of track M as case k; shared, unchanged."""
    wp, Tn, Tc = FI.track(M)
    T = Tc if caller_times else Tn
    v0, a0 = FI.v0a0(k)
    truth = MN.track_batch_refined(wp[None], T[None], v0, a0)[0]
    eo = _norm_err(FI.oracle_fit(wp, T, v0, a0), truth, T)
    return wp, T, v0, a0, truth, eo


def _mixed(caller_times):
    return [_case(M, k, caller_times) for k, M in enumerate(FI.mixed_batch_segments())]


@functools.lru_cache(maxsize=None)
def _floor():
    """Twice the oracle's worst distance from the truth over the batch-fit tracks of this module."""
    worst = max(c[5] for ct in (False, True) for c in _mixed(ct))
    print("oracle's worst _norm_err over the module's tracks", worst)
    return 2.0 * worst


def _check_path(T, Cf, wp, v0, a0):
    M = len(T)
    for d in range(3):
        for k in range(5):
            beg = np.array([O.poly_eval(Cf[i, d], 0.0, k) for i in range(M)])
            end = np.array([O.poly_eval(Cf[i, d], T[i], k) for i in range(M)])
            assert np.abs(beg[1:] - end[:-1]).max(initial=0.0) < 1e-6, (d, k)
            if k == 0:
                assert np.abs(beg - wp[:-1, d]).max() < 1e-6 and np.abs(end - wp[1:, d]).max() < 1e-6
            else:
                assert abs(beg[0] - (v0[d] if k == 1 else a0[d] if k == 2 else 0.0)) < 1e-6 and abs(end[-1]) < 1e-6


def _fit(cases, caller_times):
    wps, Ts = [c[0] for c in cases], [c[1] for c in cases]
    v0, a0 = np.array([c[2] for c in cases]), np.array([c[3] for c in cases])
    if caller_times:
        Cs, st = capi.minsnap_batch_times(wps, Ts, v0, a0)
    else:
        Tg, Cs, st = capi.minsnap_batch(wps, FI.V_MAX, FI.A_MAX, v0, a0)
        for T, want in zip(Tg, Ts):
            np.testing.assert_allclose(T, want, rtol=1e-12, atol=0)
    assert (st == 0).all(), st
    return Cs


def _assert_fit(cases, Cs, what):
    for (wp, T, v0, a0, truth, eo), Cf in zip(cases, Cs):
        eg = _norm_err(Cf, truth, T)
        print(what, len(T), "segments: _norm_err gpu", eg, "oracle", eo, "floor", _floor())
        assert np.isfinite(Cf).all()
        assert eg <= max(eo, _floor()), (what, len(T), eg, eo)
        _check_path(T, Cf, wp, v0, a0)


# ---- batch fit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("caller_times", [False, True], ids=["nfabian", "times"])
@pytest.mark.parametrize("M", [FI.K_MAX_LDS_SEG + 1, LIM["batch"][0]])
def test_batch_fit_alone(M, caller_times):
    k = FI.mixed_batch_segments().index(M)
    cases = [_case(M, k, caller_times)]
    _assert_fit(cases, _fit(cases, caller_times), "alone")


@pytest.mark.parametrize("caller_times", [False, True], ids=["nfabian", "times"])
def test_batch_fit_short_tracks_beside_the_largest(caller_times):
    cases = _mixed(caller_times)
    Cs = _fit(cases, caller_times)
    _assert_fit(cases, Cs, "mixed")
    short = [i for i, c in enumerate(cases) if len(c[1]) <= FI.K_MAX_LDS_SEG]
    Cshort = _fit([cases[i] for i in short], caller_times)
    for i, Cf in zip(short, Cshort):
        print(len(cases[i][1]), "segments: mixed batch bit-equal to the short-only batch:",
              Cs[i].tobytes() == Cf.tobytes(), "max difference", float(np.abs(Cs[i] - Cf).max()))


def _raw_batch(wps, stream, times=None):
    """epp_minsnap_batch (times None) or epp_minsnap_batch_times on buffers prefilled with
    NAN_WORD: (rc, error text, times, coefficients, statuses) as 64-bit words.  The caller's
    times are that call's input, in the times buffer."""
    wp = np.ascontiguousarray(np.concatenate(wps))
    off = np.zeros(len(wps) + 1, np.int32)
    off[1:] = np.cumsum([len(w) for w in wps])
    nseg = int(off[-1]) - len(wps)
    d_wp, d_off = capi.DeviceBuffer.from_array(wp), capi.DeviceBuffer.from_array(off)
    outs = [capi.DeviceBuffer.from_array(np.full(n, NAN_WORD, np.uint64)) for n in (nseg, nseg * 30, len(wps))]
    if times is not None:
        outs[0].upload(np.ascontiguousarray(np.concatenate(times)))
    capi.sync()
    if times is not None:
        rc = capi.lib().epp_minsnap_batch_times(d_wp.ptr, d_off.ptr, len(wps), None, None, outs[0].ptr, outs[1].ptr,
                                                outs[2].ptr, stream)
    else:
        rc = capi.lib().epp_minsnap_batch(d_wp.ptr, d_off.ptr, len(wps), FI.V_MAX, FI.A_MAX, None, None, outs[0].ptr,
                                          outs[1].ptr, outs[2].ptr, stream)
    err = capi.lib().epp_last_error().decode()
    capi.sync()
    return (rc, err) + tuple(o.download(np.uint64, n) for o, n in zip(outs, (nseg, nseg * 30, len(wps))))


def _untouched(*arrays):
    return all((a == np.uint64(NAN_WORD)).all() for a in arrays)


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside valid tracks"])
def test_batch_fit_refusal(beside):
    taken, refused = LIM["batch"]
    wps = [FI.track(refused)[0]]
    if beside:
        wps = [FI.track(12)[0], wps[0], FI.track(41)[0]]
    with pytest.raises(capi.EppError) as e:
        capi.minsnap_batch(wps, FI.V_MAX, FI.A_MAX)
    assert e.value.code == capi.EPP_ERR_UNSUPPORTED and "too many waypoints" in str(e.value)
    with pytest.raises(capi.EppError) as e:
        capi.minsnap_batch_times(wps, [FI.track(len(w) - 1)[2] for w in wps])
    assert e.value.code == capi.EPP_ERR_UNSUPPORTED and "too many waypoints" in str(e.value)
    s = C.c_void_p()
    capi.check(capi.lib().epp_stream_create(C.byref(s)))
    rc, err, T, Cf, st = _raw_batch(wps, s.value)
    assert rc == capi.EPP_ERR_UNSUPPORTED and "too many waypoints" in err
    assert _untouched(T, Cf, st)
    Tin = [FI.track(len(w) - 1)[2] for w in wps]
    rc, err, T, Cf, st = _raw_batch(wps, s.value, Tin)
    assert rc == capi.EPP_ERR_UNSUPPORTED and "too many waypoints" in err
    assert _untouched(Cf, st) and T.tobytes() == np.concatenate(Tin).tobytes()
    # the next valid call on the same stream: the largest track
    wp, Tn, _ = FI.track(taken)
    rc, err, T, Cf, st = _raw_batch([wp], s.value)
    assert rc == capi.EPP_OK, err
    assert st.view(np.int32)[0] == 0
    np.testing.assert_allclose(T.view(np.float64), Tn, rtol=1e-12, atol=0)
    Cf = Cf.view(np.float64).reshape(-1, 3, 10)
    assert np.isfinite(Cf).all()
    _check_path(Tn, Cf, wp, np.zeros(3), np.zeros(3))
    capi.lib().epp_stream_destroy(s.value)


# ---- time gradient and descent --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _alloc_ref(entry):
    """(group, D, {track name: {variant: (truth J, scale S)}}) of the entry's batch -- its largest
    track between the two short ones.  Short tracks: every variant, D over all of them (as
    tr.reference_distance).  The largest gradient track: the held entries' variants, D over
    FI.kkt_entries; the largest descent track: the times themselves."""
    M = LIM[entry][0]
    group = FI.alloc_group(M)
    D, per = 0.0, {}
    for t in group:
        m = len(t.T)
        if m <= FI.K_MAX_LDS_SEG:
            every = list(range(m + 1 if m > 1 else 1))
            per[t.name], d = FI.alloc_reference(t, every, every)
        elif entry == "gradient":
            per[t.name], d = FI.alloc_reference(t, [0] + [n + 1 for n in FI.held_entries(m)], FI.kkt_entries(m))
        else:
            per[t.name], d = FI.alloc_reference(t, [0], [0])
        D = max(D, d)
    print(f"{entry}: reference-arithmetic distance D = {D / tr.EPS:.3f} eps of sum |c Q c|")
    assert 0.0 < D < 64 * tr.EPS  # (as test_gpu_time_alloc.test_reference_distance)
    return group, D, per


def _args(group):
    return ([t.wp for t in group], [t.T for t in group], np.array([t.v0 for t in group]),
            np.array([t.a0 for t in group]))


def test_gradient_largest_alone_and_beside_short_tracks():
    """J within 2 D S of the truth and the gradient entries within 2 (2 D S) / h: every entry of
    the short tracks, FI.held_entries (every 16th, the first and last two) of the largest; status
    and finiteness on all of them."""
    group, D, per = _alloc_ref("gradient")
    M = LIM["gradient"][0]
    wps, Ts, v0, a0 = _args(group)
    J, G, st = capi.time_gradient(wps, Ts, FI.H, FI.T_MIN, v0, a0)
    assert (st == 0).all() and np.isfinite(J).all() and all(np.isfinite(g).all() for g in G)
    assert G[1].shape == (M,)
    worst_j = worst_g = 0.0
    for t, j, g in zip(group, J, G):
        p, m = per[t.name], len(t.T)
        J0, S0 = p[0]
        worst_j = max(worst_j, abs(j - J0) / (2 * D * S0))
        assert abs(j - J0) <= 2 * D * S0, (t.name, j, J0, abs(j - J0) / (tr.EPS * S0))
        if m == 1:
            assert (g == 0.0).all()
            continue
        for n in (range(m) if m <= FI.K_MAX_LDS_SEG else FI.held_entries(m)):
            Jn, Sn = p[n + 1]
            gt, bg = (Jn - J0) / FI.H, 2 * (2 * D * max(Sn, S0)) / FI.H
            worst_g = max(worst_g, abs(g[n] - gt) / bg)
            assert abs(g[n] - gt) <= bg, (t.name, n, g[n], gt, abs(g[n] - gt) / bg)
    print("largest |J - truth| / bound", worst_j, "largest |g - truth| / bound", worst_g)
    # the same bits whatever the batch: the largest alone, the short ones in a short-only batch
    J1, G1, st1 = capi.time_gradient(wps[1:2], Ts[1:2], FI.H, FI.T_MIN, v0[1:2], a0[1:2])
    assert st1[0] == 0 and J1[0] == J[1] and G1[0].tobytes() == G[1].tobytes()
    Js, Gs, ss = capi.time_gradient(wps[::2], Ts[::2], FI.H, FI.T_MIN, v0[::2], a0[::2])
    for i in range(2):
        assert ss[i] == 0 and Js[i] == J[2 * i] and Gs[i].tobytes() == G[2 * i].tobytes(), i


def test_descent_largest_alone_and_beside_short_tracks():
    """One step (max_iter = 1): cost0 and cost1 within 2 D S of the truth cost at the given and
    at the returned times; the step tr.step_from_grad's from the device's own gradient (1e-12
    relative; the halvings are the rule's 0..8, whichever the device accepted: the CPU's own
    descent would need all 587 variants' truths), sum T kept to 1e-12, coefficients bit for bit
    epp_minsnap_batch_times at the returned times."""
    group, D, per = _alloc_ref("descent")
    wps, Ts, v0, a0 = _args(group)
    prm = capi.TimeoptParams(max_iter=1)
    _, G, gs = capi.time_gradient(wps, Ts, FI.H, FI.T_MIN, v0, a0)
    Tn, Cn, J0, J1, iters, st = capi.optimize_times(wps, Ts, prm, v0, a0)
    assert (gs == 0).all() and (st >= 0).all(), (gs, st)
    Cb, sb = capi.minsnap_batch_times(wps, Tn, v0, a0)
    assert (sb == 0).all()
    for k, (t, T1) in enumerate(zip(group, Tn)):
        T = t.T
        assert Cn[k].tobytes() == Cb[k].tobytes(), k
        s0, s1 = tr.seq_sum(T), tr.seq_sum(T1)
        assert abs(s1 - s0) <= 1e-12 * s0 and (T1 >= FI.T_MIN).all()
        want0, S0 = per[t.name][0]
        Ct = tr.solve(t.wp, T1, t.v0, t.a0)[0]
        want1, S1 = tr.cost(T1, Ct), tr.cost_abs(T1, Ct)
        print(t.name, "cost", J0[k], "->", J1[k], "|cost0 - truth| / bound", abs(J0[k] - want0) / (2 * D * S0),
              "|cost1 - truth| / bound", abs(J1[k] - want1) / (2 * D * S1))
        assert abs(J0[k] - want0) <= 2 * D * S0 and abs(J1[k] - want1) <= 2 * D * S1, t.name
        if len(T) == 1:
            assert iters[k] == 0 and T1.tobytes() == T.tobytes()
            continue
        assert iters[k] == 1 and J1[k] < J0[k], (k, iters[k], J0[k], J1[k])
        rel = [float(np.max(np.abs(T1 - w) / w)) for w in (tr.step_from_grad(T, G[k], h, 0.5) for h in range(9))]
        print(t.name, "halvings", int(np.argmin(rel)), "largest relative difference", min(rel))
        assert min(rel) <= 1e-12, (k, rel)
    alone = capi.optimize_times(wps[1:2], Ts[1:2], prm, v0[1:2], a0[1:2])
    assert alone[0][0].tobytes() == Tn[1].tobytes() and alone[1][0].tobytes() == Cn[1].tobytes()


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside a valid track"])
@pytest.mark.parametrize("entry", ["gradient", "descent"])
def test_gradient_and_descent_refusal(entry, beside):
    taken, refused = LIM[entry]
    wps, Ts = [FI.track(refused)[0]], [FI.track(refused)[2]]
    if beside:
        wps, Ts = [FI.track(3)[0]] + wps, [FI.track(3)[2]] + Ts
    nt = len(wps)
    prm = capi.TimeoptParams(max_iter=1)
    with pytest.raises(capi.EppError) as e:
        if entry == "gradient":
            capi.time_gradient(wps, Ts, FI.H, FI.T_MIN)
        else:
            capi.optimize_times(wps, Ts, prm)
    assert e.value.code == capi.EPP_ERR_UNSUPPORTED and "too many waypoints" in str(e.value)
    # the C call on prefilled outputs, on a stream of its own: untouched
    d_wp, d_off, d_T, _, _, off, nseg = capi._upload_fit_inputs(wps, Ts, None, None)
    sizes = (nt, nseg, nt) if entry == "gradient" else (nseg * 30, nt, nt, nt, nt)
    outs = [capi.DeviceBuffer.from_array(np.full(n, NAN_WORD, np.uint64)) for n in sizes]
    capi.sync()
    L = capi.lib()
    s = C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    if entry == "gradient":
        rc = L.epp_minsnap_time_gradient(d_wp.ptr, d_off.ptr, nt, None, None, d_T.ptr, FI.H, FI.T_MIN, outs[0].ptr,
                                         outs[1].ptr, outs[2].ptr, s.value)
    else:
        rc = L.epp_minsnap_optimize_times(d_wp.ptr, d_off.ptr, nt, None, None, d_T.ptr, outs[0].ptr, prm, outs[1].ptr,
                                          outs[2].ptr, outs[3].ptr, outs[4].ptr, s.value)
    assert rc == capi.EPP_ERR_UNSUPPORTED and b"too many waypoints" in L.epp_last_error()
    capi.sync()
    assert _untouched(*(o.download(np.uint64, n) for o, n in zip(outs, sizes)))
    assert d_T.download(np.float64, nseg).tobytes() == np.concatenate(Ts).tobytes()
    # the next valid call of the same entry point on that stream: the three-segment track
    wp3, T3 = FI.track(3)[0], FI.track(3)[2]
    d_wp, d_off, d_T, _, _, off, nseg = capi._upload_fit_inputs([wp3], [T3], None, None)
    outs = [capi.DeviceBuffer(8 * n) for n in (90, 3, 3, 3, 3)]
    if entry == "gradient":
        capi.check(L.epp_minsnap_time_gradient(d_wp.ptr, d_off.ptr, 1, None, None, d_T.ptr, FI.H, FI.T_MIN,
                                               outs[1].ptr, outs[2].ptr, outs[3].ptr, s.value))
        capi.sync()
        want = capi.time_gradient([wp3], [T3], FI.H, FI.T_MIN)
        assert want[2][0] == 0 and outs[3].download(np.int32, 1)[0] == 0
        assert outs[1].download(np.float64, 1)[0] == want[0][0]
        assert outs[2].download(np.float64, 3).tobytes() == want[1][0].tobytes()
    else:
        capi.check(L.epp_minsnap_optimize_times(d_wp.ptr, d_off.ptr, 1, None, None, d_T.ptr, outs[0].ptr, prm,
                                                outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, s.value))
        capi.sync()
        want = capi.optimize_times([wp3], [T3], prm)
        assert want[4][0] == 1 and outs[3].download(np.int32, 1)[0] == 1
        assert d_T.download(np.float64, 3).tobytes() == want[0][0].tobytes()
        assert outs[0].download(np.float64, 90).tobytes() == want[1][0].tobytes()
    L.epp_stream_destroy(s.value)


# ---- the single-track refit -----------------------------------------------------------------
def _extra(T):
    return Fraction(1e-9) * Fraction(max(1.0, float(np.sum(T)))) ** 2


def _refit_against_truth(wp, T, dt, v0, a0, what):
    single = capi.generate_trajectory_times(wp, T, dt, FI.T0, v0, a0)
    Cb, st = capi.minsnap_batch_times([wp], [T], v0[None], a0[None])
    assert st[0] == 0
    batch = capi.sample_batch([T], Cb, dt, t0=[FI.T0])
    truth = SR.Truth(T, Cb[0], dt)
    assert len(single) == len(truth) and single[-1, 9] == truth.time(FI.T0)[-1]
    wb = SR.assert_rows(batch, truth, FI.T0, (what, "batch"))
    ws = SR.assert_rows(single, truth, FI.T0, (what, "single"), extra=_extra(T), positions=False)
    print(f"{what}: {len(truth)} rows, worst error / bound: batch {wb.tolist()}, single (before the allowance) "
          f"{ws.tolist()}, allowance {float(_extra(T))}")
    assert (wb <= 1.0).all()
    np.testing.assert_allclose(single[0, [0, 3, 6]], wp[0], atol=1e-9)
    np.testing.assert_allclose(single[0, [1, 4, 7]], v0, atol=1e-9)
    np.testing.assert_allclose(single[0, [2, 5, 8]], a0, atol=1e-9)
    return single


@pytest.mark.parametrize("M", FI.refit_segments()[:3])
def test_refit_on_both_sides_of_its_layouts(M):
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    rows = _refit_against_truth(wp, Tc, FI.refit_dt(M), v0, a0, f"{M} segments")
    assert len(rows) > 2048


def test_refit_largest():
    """4280 segments, the largest refit launch (`big` layout, v0 / a0 from host memory): every
    row within 1e-6 of the oracle's (oracle.sample_traj of oracle.minsnap_solve at these times,
    recorded in tests/golden/fit_limits_refit_4280_rows.npy: that solve takes a quarter of an
    hour; test_fit_limits_inputs_cpu.py holds the file to this track), time column exact, the
    first row the start vertex."""
    M = LIM["refit"][0]
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    dt = FI.refit_dt(M)
    want = FI.refit_largest_rows()
    rows = capi.generate_trajectory_times(wp, Tc, dt, FI.T0, v0, a0)
    assert rows.shape == want.shape and len(rows) > 2048
    assert rows[:, 9].tobytes() == want[:, 9].tobytes()
    d = np.abs(rows[:, :9] - want[:, :9])
    print("largest |row - oracle's|", float(d.max()), "in column", int(d.max(axis=0).argmax()))
    assert d.max() < 1e-6
    np.testing.assert_allclose(rows[0, [0, 3, 6]], wp[0], atol=1e-9)
    np.testing.assert_allclose(rows[0, [1, 4, 7]], v0, atol=1e-9)
    np.testing.assert_allclose(rows[0, [2, 5, 8]], a0, atol=1e-9)


def test_refit_refusal_and_next_call():
    M = LIM["refit"][1]
    wp, _, Tc = FI.track(M)
    with pytest.raises(capi.EppError) as e:
        capi.generate_trajectory_times(wp, Tc, 1.0, FI.T0, *FI.v0a0(0))
    assert e.value.code == capi.EPP_ERR_UNSUPPORTED and "too many waypoints" in str(e.value)
    wp, _, Tc = FI.track(12)
    v0, a0 = FI.v0a0(3)
    got = capi.generate_trajectory_times(wp, Tc, 0.1, FI.T0, v0, a0)
    exp = O.sample_traj(Tc, FI.oracle_fit(wp, Tc, v0, a0), 0.1, FI.T0)
    assert got.shape == exp.shape and np.array_equal(got[:, 9], exp[:, 9])
    assert np.abs(got[:, :9] - exp[:, :9]).max() < 1e-6


def test_fused_check_on_the_big_layout(cfg, geom):
    from eppamd import config, synth
    rg, ro = config.inflate_radii(cfg)
    gates, obstacles = synth.track_world(42)
    md = float(cfg["path_planner_properties"]["min_dist_check_traj_collision"])
    M = LIM["refit big"][1]
    wp = FI.track(M)[0]
    v0, a0 = FI.v0a0(M)
    pts = synth.sample_states(300 + M, [-6, -6, 0], [6, 6, 2], 300)
    w = capi.World(capi.build_obbs(geom, gates, obstacles), rg, ro)
    flags, rows = capi.check_and_generate_trajectory(w, pts, md, wp, FI.V_MAX, FI.A_MAX, 0.5, FI.T0, v0, a0)
    ref = O.world_build(geom, gates, obstacles, rg, ro)
    assert np.array_equal(flags, O.check_states_mindist(ref, pts, md))
    print("valid check points", int(flags.sum()), "of", len(flags))
    sep = capi.generate_trajectory(wp, FI.V_MAX, FI.A_MAX, 0.5, FI.T0, v0, a0)
    assert rows.tobytes() == sep.tobytes() and len(rows) > 128
    w.close()


# ---- the refit's row slicing ----------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(FI.ROW_COUNTS)))
def test_refit_row_slices(case):
    R, dt = FI.row_cases()[case]
    wp, _, Tc = FI.track(FI.ROW_TRACK)
    v0, a0 = FI.v0a0(case)
    rows = _refit_against_truth(wp, Tc, dt, v0, a0, f"{R} rows")
    assert len(rows) == R
