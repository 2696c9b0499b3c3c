"""GPU: time scaling of fitted tracks to thrust, body-rate and tilt limits
(epp_traj_thrust_grid_batch, epp_traj_scale_to_thrust_limits, csrc/thrust_scale.hip).

1. the fused search equals the composition -- the same bracketing and bisection driven from
   Python over epp_traj_thrust_grid_batch(scale_in = s), one call per step -- in scale, status
   and violated, and its scaled tracks equal the restatement's apply of that scale, all ==;
2. the hand-built tracks give their exact answers (1.5, 1.0, status 1, status -1, violated);
3. thrust_grid against the restatement (thrust_rates_ref's ulps; times where separated);
4. the fused scales against the restatement, == wherever no decision of the restatement's
   search lay within 4 ulp of its limit (at most 2 % left out; the inputs leave out none);
5. the rows of the scaled tracks at dt = 0.01 against the limits -- a REPORT: the search
   guarantees the grid points, the rows are other points, so what is printed is the largest
   excess of the rows over the grid extremes and over the limits (DESIGN.md records it); what is
   asserted is the grid-point guarantee itself on the scaled tracks;
6. the call inside a captured graph; 7. the Python and C++ layers.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import thrust_rates_ref as tr
import thrust_scale_inputs as si
import thrust_scale_ref as sr
from conftest import CONFIG
from eppamd import capi, synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def fitted():
    fT, fC, _ = O.minsnap_batch(list(si.fit_waypoints()), si.V_MAX, si.A_MAX, threads=8)
    return list(fT), list(fC)


@functools.lru_cache(maxsize=None)
def short():
    """(Ts, Cs of the 1025 tracks, the index of each one's distinct fit)."""
    sT, sC, _ = O.minsnap_batch(list(si.short_waypoints()), si.V_MAX, si.A_MAX, threads=8)
    idx = [k % len(sT) for k in range(si.N_SHORT)]
    return [sT[i] for i in idx], [sC[i] for i in idx], idx


@functools.lru_cache(maxsize=None)
def fitted_ref():
    return sr.scale_tracks(*fitted(), si.L_FIT)


def fused(Ts, Cs, L):
    Tn, Cn, scale, status, viol = capi.scale_to_thrust_limits(Ts, Cs, *L)
    return [(scale[k], int(status[k]), int(viol[k]), Tn[k], Cn[k]) for k in range(len(Ts))]


def composed(Ts, Cs, L):
    """The search driven from the host, the tracks uploaded once: [(scale, status, violated, T,
    C)] with the restatement's apply of the scale found, and the number of grid calls."""
    nt = len(Ts)
    lib = capi.lib()
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_s, d_out = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(64 * nt)

    def grid_call(s):
        d_s.upload(np.ascontiguousarray(s, np.float64))
        capi.check(lib.epp_traj_thrust_grid_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, d_s.ptr, L.g, d_out.ptr, None))
        capi.sync()
        return d_out.download(np.float64, 8 * nt).reshape(nt, 8)

    valid = [not sr.track_invalid(T, Cf) for T, Cf in zip(Ts, Cs)]
    scale, status, viol, calls = sr.composition(grid_call, valid, L)
    out = []
    for k in range(nt):
        T, Cf = np.asarray(Ts[k], np.float64).ravel(), np.asarray(Cs[k], np.float64).reshape(-1, 3, 10)
        if status[k] == 0 and scale[k] != 1.0:
            T, Cf = sr.apply(T, Cf, scale[k])
        out.append((scale[k], int(status[k]), int(viol[k]), T, Cf))
    return out, calls


# ---- 1. fused == composition -------------------------------------------------------------------
@pytest.mark.parametrize("group", range(len(si.hand_groups())), ids=[g.name for g in si.hand_groups()])
def test_hand_tracks_equal_composition(group):
    g = si.hand_groups()[group]
    got = fused(g.Ts, g.Cs, g.limits)
    exp, calls = composed(g.Ts, g.Cs, g.limits)
    assert calls <= 1 + sr.MAX_DOUBLINGS + sr.BISECT_ROUNDS
    assert sr.compare_results(got, exp) == []
    for k in range(len(g.Ts)):  # alone
        one = fused(g.Ts[k:k + 1], g.Cs[k:k + 1], g.limits)
        assert sr.compare_results(one, exp[k:k + 1]) == [], g.names[k]


def test_fitted_tracks_equal_composition():
    fT, fC = fitted()
    got = fused(fT, fC, si.L_FIT)
    exp, calls = composed(fT, fC, si.L_FIT)
    scales = np.array([r[0] for r in got])
    print("calls", calls, "scales: min %.3f median %.3f max %.3f" % (scales.min(), np.median(scales), scales.max()))
    assert sr.compare_results(got, exp) == []
    assert ((scales > 1.0) & (scales < 4.0)).mean() > 0.5 and got[-1][0] > 1.0  # (the 44 segments too)


def test_1025_short_tracks_equal_composition():
    sT, sC, _ = short()
    got = fused(sT, sC, si.L_FIT)
    exp, _ = composed(sT, sC, si.L_FIT)
    assert len(got) == si.N_SHORT and sr.compare_results(got, exp) == []
    assert sum(r[0] > 1.0 for r in got) > si.N_SHORT // 2


# ---- 2. the exact answers ----------------------------------------------------------------------
def test_hand_tracks_exact_answers():
    for g in si.hand_groups():
        got = fused(g.Ts, g.Cs, g.limits)
        grid = capi.thrust_grid(g.Ts, g.Cs, g.limits.g)
        for k, (name, want, r) in enumerate(zip(g.names, g.wants, got)):
            what = (g.name, name)
            assert (r[1], r[2]) == (want.status, want.violated), what
            if want.scale is not None:
                assert r[0] == want.scale, (what, r[0])
            else:
                assert si.FREE_FALL_SCALE[0] < r[0] < si.FREE_FALL_SCALE[1], (what, r[0])
            T0, C0 = np.asarray(g.Ts[k], np.float64), np.asarray(g.Cs[k], np.float64).reshape(-1, 3, 10)
            if r[0] == 1.0:  # untouched, bit for bit (NaN times included)
                assert r[3].tobytes() == T0.tobytes() and r[4].tobytes() == C0.tobytes(), what
            else:
                Tn, Cn = sr.apply(T0, C0, r[0])
                assert r[3].tobytes() == Tn.tobytes() and r[4].tobytes() == Cn.tobytes(), what
            if want.t_fmax is not None:
                assert grid[k, 3] == want.t_fmax, (what, grid[k, 3])
            if want.status == -1:
                assert grid[k].tobytes() == sr.IDENTITY.tobytes(), what


# ---- 3. thrust_grid against the restatement ----------------------------------------------------
def _grid_reference(Ts, Cs, s, g):
    outs, sep = [], []
    for T, Cf, sk in zip(Ts, Cs, s):
        out, idx, q = sr.grid_extremes(T, Cf, sk, g)
        outs.append(out)
        sep.append([True] * 4 if q is None else
                   [tr.separated(v, is_min, int(i)) for (v, is_min), i in
                    zip(((q[0], True), (q[0], False), (q[1], False), (q[2], True)), idx)])
    return np.array(outs), sep


@pytest.mark.parametrize("scale", [None, 1.5, "per track"])
def test_thrust_grid_equals_restatement(scale):
    fT, fC = fitted()
    g0 = si.hand_groups()[0]
    Ts, Cs = list(g0.Ts) + fT[:24] + fT[-1:], list(g0.Cs) + fC[:24] + fC[-1:]
    n = len(Ts)
    s = np.ones(n) if scale is None else np.full(n, 1.5) if scale == 1.5 else 1.0 + (np.arange(n) % 7) * 0.375
    got = capi.thrust_grid(Ts, Cs, si.GRAVITY, None if scale is None else s)
    exp, sep = _grid_reference(Ts, Cs, s, si.GRAVITY)
    bad = sr.compare_grid(got, exp, sep)
    print("times compared:", sum(map(sum, sep)), "of", 4 * n)
    assert bad == [], bad[:8]
    assert sum(map(sum, sep)) > 2 * n


# ---- 4. the fused scales against the restatement -----------------------------------------------
def test_fused_scales_equal_restatement():
    fT, fC = fitted()
    exp = fitted_ref()
    got = fused(fT, fC, si.L_FIT)
    skip = {k for k, r in enumerate(exp) if r.marginal}
    print("left out:", sorted(skip))
    assert len(skip) <= 0.02 * len(exp)
    assert sr.compare_results(got, exp, skip) == []
    sT, sC, idx = short()
    ref = sr.scale_tracks(sT[:41], sC[:41], si.L_FIT)
    got = fused(sT, sC, si.L_FIT)
    skip = {k for k in range(si.N_SHORT) if ref[idx[k]].marginal}
    assert len(skip) <= 0.02 * si.N_SHORT
    assert sr.compare_results(got, [ref[i] for i in idx], skip) == []


# ---- 5. the rows of the scaled tracks: a report ------------------------------------------------
def test_rows_after_scaling_report():
    fT, fC = fitted()
    L = si.L_FIT
    Tn, Cn, scale, status, _ = capi.scale_to_thrust_limits(fT, fC, *L)
    assert (status == 0).all()
    grid = capi.thrust_grid(Tn, Cn, L.g)
    rows, _ = capi.trajectory_thrust_rates(Tn, Cn, si.FIT_DT, L.g)
    # the guarantee: no grid point of the scaled track violates.  The scaled track's own a and j
    # are those of the search (a / s2, j / s3) up to the rounding of the apply -- ten products
    # per polynomial, each within a few ulp -- so 1e-9 relative is far above it and far below
    # anything the grid's spacing could hide.
    tol = 1e-9
    assert (grid[:, 0] >= L.f_min * (1 - tol)).all() and (grid[:, 2] <= L.f_max * (1 + tol)).all()
    assert (grid[:, 4] <= L.rate_max * (1 + tol)).all() and (grid[:, 6] >= L.cos_tilt_min * (1 - tol)).all()
    assert np.isfinite(rows[:, ::2]).all()
    # the report: how far the rows (other points than the grid) go beyond the grid extremes and
    # beyond the limits, relative to the limit
    over_grid = np.array([(grid[:, 0] - rows[:, 0]) / L.f_min, (rows[:, 2] - grid[:, 2]) / L.f_max,
                          (rows[:, 4] - grid[:, 4]) / L.rate_max, (grid[:, 6] - rows[:, 6]) / L.cos_tilt_min])
    over_limit = np.array([(L.f_min - rows[:, 0]) / L.f_min, (rows[:, 2] - L.f_max) / L.f_max,
                           (rows[:, 4] - L.rate_max) / L.rate_max, (L.cos_tilt_min - rows[:, 6]) / L.cos_tilt_min])
    for q, name in enumerate(("f_min", "f_max", "rate_max", "cos_tilt_min")):
        print("%-12s rows beyond the grid extreme: %.3e   rows beyond the limit: %.3e (relative, largest over %d tracks)"
              % (name, over_grid[q].max(), over_limit[q].max(), len(fT)))


# ---- 6. graph capture --------------------------------------------------------------------------
def test_graph_replay():
    fT, fC = fitted()
    A = (fT[:16], fC[:16])
    B = (A[0], [c * 1.25 for c in A[1]])  # the same times, other coefficients
    nt = 16
    L = capi.lib()
    lim = si.L_FIT
    d_T, d_C, d_off, _, nseg = capi._upload_tracks(*A)
    outs = [capi.DeviceBuffer(b) for b in (8 * nt, 4 * nt, 4 * nt, 64 * nt)]
    d_sc, d_st, d_vi, d_grid = outs
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_traj_scale_to_thrust_limits(d_T.ptr, d_C.ptr, d_off.ptr, nt, *lim, d_sc.ptr, d_st.ptr, d_vi.ptr,
                                                 s.value))
    capi.check(L.epp_traj_thrust_grid_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, None, lim.g, d_grid.ptr, s.value))
    capi.check(L.epp_graph_end(s.value, C.byref(g)))
    scales = []
    for Tk, Ck in (A, B):
        Tn, Cn, scale, status, viol = capi.scale_to_thrust_limits(Tk, Ck, *lim)  # the direct call
        exp_grid = capi.thrust_grid(Tn, Cn, lim.g)
        d_T.upload(np.concatenate(Tk))
        d_C.upload(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3, 10) for c in Ck]))
        for b in outs:
            capi.check(L.epp_memset(b.ptr, 0x5A, b.nbytes, None))  # poison
        capi.sync()
        capi.check(L.epp_graph_launch(g.value, s.value))
        capi.check(L.epp_stream_sync(s.value))
        assert d_sc.download(np.float64, nt).tobytes() == scale.tobytes()
        assert np.array_equal(d_st.download(np.int32, nt), status) and np.array_equal(d_vi.download(np.int32, nt), viol)
        assert d_T.download(np.float64, nseg).tobytes() == np.concatenate(Tn).tobytes()
        assert d_C.download(np.float64, nseg * 30).tobytes() == np.concatenate(Cn).tobytes()
        assert d_grid.download(np.float64, 8 * nt).tobytes() == exp_grid.tobytes()
        scales.append(scale)
    assert scales[0].tobytes() != scales[1].tobytes()  # (the replay saw the changed coefficients)
    capi.check(L.epp_graph_destroy(g.value))
    L.epp_stream_destroy(s.value)


def test_violated_may_be_null():
    fT, fC = fitted()
    nt = 8
    d_T, d_C, d_off, _, _ = capi._upload_tracks(fT[:nt], fC[:nt])
    d_sc, d_st = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(4 * nt)
    capi.check(capi.lib().epp_traj_scale_to_thrust_limits(d_T.ptr, d_C.ptr, d_off.ptr, nt, *si.L_FIT, d_sc.ptr,
                                                          d_st.ptr, None, None))
    capi.sync()
    exp = fused(fT[:nt], fC[:nt], si.L_FIT)
    assert d_sc.download(np.float64, nt).tolist() == [r[0] for r in exp]
    assert d_st.download(np.int32, nt).tolist() == [r[1] for r in exp]


# ---- 7. the Python and C++ layers --------------------------------------------------------------
def test_generate_trajectory_thrust_limits():
    import polynomial_trajectory as pt
    lim = tuple(si.L_FIT)
    for k in (0, 5, 12):
        wp = np.asarray(si.fit_waypoints()[k])
        for enforce in (False, True):
            rows = pt.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05, enforceLimits=enforce, thrustLimits=lim)
            exp, s_va, s_th = capi.generate_trajectory_flyable(wp, si.V_MAX, si.A_MAX, 0.05, lim, enforce_va=enforce,
                                                               return_scales=True)
            assert rows.shape == exp.shape and rows.tobytes() == exp.tobytes(), (k, enforce)
            assert s_th >= 1.0 and (enforce or s_va == 1.0)
        # the rows are those of the batch calls: fit, (v / a scaling,) thrust scaling, sampling
        Ts, Cs, st = capi.minsnap_batch([wp], si.V_MAX, si.A_MAX)
        Tn, Cn, scale, status, _ = capi.scale_to_thrust_limits(Ts, Cs, *lim)
        got, _, s_th = capi.generate_trajectory_flyable(wp, si.V_MAX, si.A_MAX, 0.05, lim, return_scales=True)
        assert s_th == scale[0] and status[0] == 0
        assert got.tobytes() == capi.sample_batch(Tn, Cn, 0.05).tobytes(), k
        # thrustLimits=None: today's rows, bit for bit
        assert pt.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05, thrustLimits=None).tobytes() == \
            pt.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05).tobytes() == \
            capi.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05).tobytes()
        assert pt.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05, enforceLimits=True).tobytes() == \
            capi.generate_trajectory_limited(wp, si.V_MAX, si.A_MAX, 0.05).tobytes()
    with pytest.raises(ValueError):
        pt.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05, thrustLimits=(9.81, 0.0, 5.0, 1.0, 0.5))
    with pytest.raises(ValueError):
        pt.generate_trajectory(wp, si.V_MAX, si.A_MAX, 0.05, thrustLimits=(9.81, 0.0, 20.0))


def test_path_planner_candidate_flyable_scales():
    import online_traj_planner as otp
    gates, obstacles = synth.track_world(42)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), CONFIG)
    sets = [np.asarray(w) for w in si.fit_waypoints()[:12]]
    lim = tuple(si.L_FIT)
    Ts, Cs, st = capi.minsnap_batch(sets, si.V_MAX, si.A_MAX)
    assert (st == 0).all()
    Tn, Cn, exp_scale, exp_status, exp_viol = capi.scale_to_thrust_limits(Ts, Cs, *lim)
    scale, duration, status, viol = pp.candidate_flyable_scales(sets, si.V_MAX, si.A_MAX, lim)
    assert scale.dtype == np.float64 and duration.dtype == np.float64 and scale.shape == duration.shape == (12,)
    assert scale.tobytes() == exp_scale.tobytes()
    assert np.array_equal(status, exp_status) and np.array_equal(viol, exp_viol)
    assert duration.tolist() == [functools.reduce(lambda a, b: a + b, T.tolist(), 0.0) for T in Tn]
    print("scale", scale.round(3).tolist(), "duration", duration.round(2).tolist())
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_flyable_scales([sets[0], sets[1][:1]], si.V_MAX, si.A_MAX, lim)
    with pytest.raises(ValueError, match="f_min < g < f_max"):
        pp.candidate_flyable_scales(sets, si.V_MAX, si.A_MAX, (9.81, 0.0, 5.0, 1.0, 0.5))
    assert [r.shape for r in pp.candidate_flyable_scales([], si.V_MAX, si.A_MAX, lim)] == [(0,)] * 4
