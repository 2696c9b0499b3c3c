"""GPU: the segment-time allocation (epp_traj_snap_cost, epp_minsnap_time_gradient,
epp_minsnap_optimize_times, csrc/time_alloc.hip) against the truth of time_alloc_ref.py, and
the layers above it.

Bounds (none is tuned to the device's answers):
  cost from given coefficients   |J_gpu - J_np| <= 64 eps sum |c_a Q_ab c_b|: both sum 36
      products per polynomial.
  cost and gradient through the solve   the distance D of the reference-arithmetic solve
      (oracle/minsnap_np.track_batch, cost summed in doubles as the reference sums it) from
      the truth in J is measured on the CPU over every variant of every track used here, in
      units of S = sum |c_a Q_ab c_b| (the sum cancels to ~1e-6 of S, so S is what a cost's
      rounding scales with); it is printed by test_reference_distance (~0.12 eps).  The GPU's
      J may be 2 D S from the truth, a gradient entry 2 * (2 D S) / h (its two costs; S the
      larger of the two).
  one step   the device's times against the restated step built from the device's own gradient
      with the accepted alpha of the CPU run: 1e-12 relative; iters and status equal.
  run to the end   sum T kept to 1e-12, T >= t_min, cost1 <= cost0, cost1 the truth cost at
      the returned times within 2 D S, coefficients bit for bit epp_minsnap_batch_times there;
      M = 3, 4 at max_iter = 200, ftol = 0: no farther from SLSQP's optimum than twice the
      restatement's gap plus 2 D S."""
import functools

import numpy as np
import pytest

import time_alloc_inputs as ti
import time_alloc_ref as tr
from eppamd import capi, synth

from conftest import CONFIG

pytestmark = pytest.mark.gpu

TRACKS = ti.tracks()
BATCHES = ti.batches()
EPS = tr.EPS


@functools.lru_cache(maxsize=None)
def _reference():
    """(D, {name: (variants, truth costs, scales)}) over every track of every batch."""
    every = {t.name: t for g in BATCHES.values() for t in g}
    every.update(TRACKS)
    return tr.reference_distance(list(every.values()), ti.H, ti.T_MIN)


def _wps(group):
    return [t.wp for t in group]


def _times(group):
    return [t.T for t in group]


def test_reference_distance():
    D, per = _reference()
    print(f"reference-arithmetic distance D = {D / EPS:.3f} eps of sum |c Q c| over {sum(len(v[1]) for v in per.values())} solves")
    assert 0.0 < D < 64 * EPS  # (the reference's own rounding cannot exceed the derived 36-product bound)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_cost_from_given_coefficients(batch):
    group = BATCHES[batch]
    v0, a0 = ti.v0a0(group)
    Cs, st = capi.minsnap_batch_times(_wps(group), _times(group), v0, a0)
    assert (st == 0).all()
    J, js = capi.snap_cost(_times(group), Cs)
    assert (js == 0).all()
    for t, C, j in zip(group, Cs, J):
        want, S = tr.cost(t.T, C), tr.cost_abs(t.T, C)
        print(batch, t.name, j, want, abs(j - want) / (EPS * S))
        assert abs(j - want) <= 64 * EPS * S, t.name


def test_cost_of_invalid_tracks_and_their_neighbours():
    group = [TRACKS["m3"], TRACKS["m12"], TRACKS["m2"]]
    Cs, _ = capi.minsnap_batch_times(_wps(group), _times(group))
    good, _ = capi.snap_cost(_times(group), Cs)
    Ts = [t.T.copy() for t in group]
    Ts2 = [Ts[0], np.array([1.0, 0.0, 2.0]), Ts[1], np.array([1.0, np.nan]), Ts[2], np.zeros(0), Ts[0]]
    Cn = Cs[0].copy()
    Cn[1, 2, 5] = np.inf
    Cs2 = [Cs[0], Cs[0], Cs[1], Cs[2], Cs[2], np.zeros((0, 3, 10)), Cn]
    J, st = capi.snap_cost(Ts2, Cs2)
    assert st.tolist() == [0, -1, 0, -1, 0, -1, -1]
    assert np.isnan(J[[1, 3, 5, 6]]).all()
    assert J[[0, 2, 4]].tobytes() == good.tobytes()


@pytest.mark.parametrize("batch", list(BATCHES))
def test_cost_and_gradient_through_the_solve(batch):
    D, per = _reference()
    group = BATCHES[batch]
    v0, a0 = ti.v0a0(group)
    J, G, st = capi.time_gradient(_wps(group), _times(group), ti.H, ti.T_MIN, v0, a0)
    assert (st == 0).all()
    worst_j = worst_g = 0.0
    for t, j, g in zip(group, J, G):
        V, Jt, S = per[t.name]
        M = len(t.T)
        bj = 2 * D * S[0]
        worst_j = max(worst_j, abs(j - Jt[0]) / bj)
        assert abs(j - Jt[0]) <= bj, (t.name, j, Jt[0], abs(j - Jt[0]) / (EPS * S[0]))
        assert g.shape == (M,)
        if M == 1:
            assert (g == 0.0).all()
            continue
        gt = (Jt[1:] - Jt[0]) / ti.H
        bg = 2 * (2 * D * np.maximum(S[1:], S[0])) / ti.H
        worst_g = max(worst_g, float(np.max(np.abs(g - gt) / bg)))
        assert (np.abs(g - gt) <= bg).all(), (t.name, np.abs(g - gt) / bg)
    print(batch, "largest |J - truth| / bound", worst_j, "largest |g - truth| / bound", worst_g)


def test_gradient_of_invalid_tracks_and_their_neighbours():
    a, b = TRACKS["m3"], TRACKS["m2"]
    alone = capi.time_gradient([a.wp, b.wp, a.wp], [a.T, b.T, a.T], ti.H, ti.T_MIN)
    wn = a.wp.copy()
    wn[2, 1] = np.nan
    J, G, st = capi.time_gradient([a.wp, a.wp, b.wp, wn, a.wp], [a.T, np.array([1.0, -0.5, 1.0]), b.T, a.T, a.T],
                                  ti.H, ti.T_MIN)
    assert st.tolist() == [0, -2, 0, 0, 0]
    assert np.isnan(J[1]) and np.isnan(G[1]).all() and np.isnan(J[3])
    assert J[[0, 2, 4]].tobytes() == alone[0].tobytes()
    for k, m in ((0, 0), (2, 1), (4, 2)):
        assert G[k].tobytes() == alone[1][m].tobytes()


@functools.lru_cache(maxsize=None)
def _cpu_step(name, step0):
    t = TRACKS[name]
    return tr.descent(t.wp, t.T, tr.DEFAULTS._replace(max_iter=1, step0=step0), t.v0, t.a0)


@pytest.mark.parametrize("which", ["lds 0.5", "lds 1.0", "long 0.5"])
def test_one_step(which):
    kind, step0 = which.split()
    step0 = float(step0)
    group = [t for t, s in ti.one_step_cases() if s == step0 and (len(t.T) > 40) == (kind == "long")]
    assert group
    v0, a0 = ti.v0a0(group)
    _, G, gs = capi.time_gradient(_wps(group), _times(group), ti.H, ti.T_MIN, v0, a0)
    Tn, Cn, J0, J1, iters, st = capi.optimize_times(_wps(group), _times(group),
                                                    capi.TimeoptParams(max_iter=1, step0=step0), v0, a0)
    assert (gs == 0).all()
    for t, g, T1, it, s, j0, j1 in zip(group, G, Tn, iters, st, J0, J1):
        r = _cpu_step(t.name, step0)
        want = tr.step_from_grad(t.T, g, r.trace[0].halvings, step0)
        print(which, t.name, "halvings", r.trace[0].halvings, "status", s, r.status,
              "largest relative difference", np.max(np.abs(T1 - want) / want))
        assert (it, s) == (r.iters, r.status)
        assert (np.abs(T1 - want) <= 1e-12 * want).all(), t.name
        assert j1 < j0


@functools.lru_cache(maxsize=None)
def _to_the_end(batch):
    group = BATCHES[batch]
    v0, a0 = ti.v0a0(group)
    return capi.optimize_times(_wps(group), _times(group), None, v0, a0)


@pytest.mark.parametrize("batch", list(BATCHES))
def test_run_to_the_end(batch):
    D, _ = _reference()
    group = BATCHES[batch]
    v0, a0 = ti.v0a0(group)
    Tn, Cn, J0, J1, iters, st = _to_the_end(batch)
    Cb, sb = capi.minsnap_batch_times(_wps(group), Tn, v0, a0)
    assert (sb == 0).all()
    for t, T1, C1, j0, j1, it, s, C2 in zip(group, Tn, Cn, J0, J1, iters, st, Cb):
        M = len(t.T)
        s0, s1 = tr.seq_sum(t.T), tr.seq_sum(T1)
        assert abs(s1 - s0) <= 1e-12 * s0 and (T1 >= ti.T_MIN).all(), t.name
        assert j1 <= j0 and s in (0, 1, 2), t.name
        Ct = tr.solve(t.wp, T1, t.v0, t.a0)[0]
        want, S = tr.cost(T1, Ct), tr.cost_abs(T1, Ct)
        print(batch, t.name, "iters", it, "status", s, "cost", j0, "->", j1, "|cost1 - truth| / bound",
              abs(j1 - want) / (2 * D * S))
        assert abs(j1 - want) <= 2 * D * S, t.name
        assert C1.tobytes() == C2.tobytes(), t.name
        if M == 1:
            assert (it, s) == (0, 0) and j1 == j0 and T1.tobytes() == t.T.tobytes()
        else:
            assert it >= 1, t.name


def test_max_iter_zero_is_the_plain_fit():
    group = BATCHES["two"]
    v0, a0 = ti.v0a0(group)
    Tn, Cn, J0, J1, iters, st = capi.optimize_times(_wps(group), _times(group), capi.TimeoptParams(max_iter=0), v0, a0)
    Cb, _ = capi.minsnap_batch_times(_wps(group), _times(group), v0, a0)
    Jg, _, _ = capi.time_gradient(_wps(group), _times(group), ti.H, ti.T_MIN, v0, a0)
    assert iters.tolist() == [0, 0] and st.tolist() == [0, 0] and J1.tobytes() == J0.tobytes() == Jg.tobytes()
    for t, T1, C1, C2 in zip(group, Tn, Cn, Cb):
        assert T1.tobytes() == t.T.tobytes() and C1.tobytes() == C2.tobytes()


def test_descent_of_invalid_tracks_and_their_neighbours():
    a, b = TRACKS["m3"], TRACKS["m2"]
    alone = capi.optimize_times([a.wp, b.wp, a.wp], [a.T, b.T, a.T])
    wn = a.wp.copy()
    wn[2, 1] = np.nan
    bad_T = np.array([1.0, -0.5, 1.0])
    Tn, Cn, J0, J1, iters, st = capi.optimize_times([a.wp, a.wp, b.wp, wn, a.wp], [a.T, bad_T, b.T, a.T, a.T])
    assert st[1] == -2 and iters[1] == 0 and np.isnan(J0[1]) and np.isnan(J1[1]) and Tn[1].tobytes() == bad_T.tobytes()
    assert st[3] == 0 and iters[3] == 0 and np.isnan(J0[3]) and np.isnan(J1[3]) and Tn[3].tobytes() == a.T.tobytes()
    for k, m in ((0, 0), (2, 1), (4, 2)):
        assert Tn[k].tobytes() == alone[0][m].tobytes() and Cn[k].tobytes() == alone[1][m].tobytes()
        assert (J0[k], J1[k], iters[k], st[k]) == (alone[2][m], alone[3][m], alone[4][m], alone[5][m])


@pytest.mark.parametrize("name", ["m3", "m4"])
def test_long_run_against_scipy(name):
    D, _ = _reference()
    t = TRACKS[name]
    prm = tr.DEFAULTS._replace(max_iter=200, ftol=0.0)
    r = tr.descent(t.wp, t.T, prm)
    Ts, Js = tr.scipy_optimum(t.wp, t.T, ti.T_MIN)
    gap = r.cost1 - Js
    Tn, Cn, J0, J1, iters, st = capi.optimize_times([t.wp], [t.T], capi.TimeoptParams(max_iter=200, ftol=0.0))
    S = tr.cost_abs(Tn[0], Cn[0])
    print(name, "SLSQP", Js, "restatement", r.cost1, f"({r.iters} steps, status {r.status})", "device", J1[0],
          f"({iters[0]} steps, status {st[0]})", "gap", gap / Js, (J1[0] - Js) / Js)
    assert gap >= 0.0
    assert J1[0] - Js <= 2 * gap + 2 * D * S
    assert abs(tr.seq_sum(Tn[0]) - tr.seq_sum(t.T)) <= 1e-12 * tr.seq_sum(t.T) and (Tn[0] >= ti.T_MIN).all()


# ---- upper layers ------------------------------------------------------------------------------
V_MAX, A_MAX = 1.0, 2.0


def test_generate_trajectory_optimize_times():
    import polynomial_trajectory as pt
    wp = TRACKS["m4"].wp
    (T0,), (C0,), _ = capi.minsnap_batch([wp], V_MAX, A_MAX)
    total = tr.seq_sum(T0)
    dt = total / 37.5  # (the last sample is half a step before the end: a rounding of the total adds no row)
    plain = pt.generate_trajectory(wp, V_MAX, A_MAX, dt)
    rows = pt.generate_trajectory(wp, V_MAX, A_MAX, dt, optimizeTimes=True)
    (T1,), (C1,), J0, J1, iters, st = capi.optimize_times([wp], [T0])
    assert iters[0] >= 1 and J1[0] < J0[0]
    want = capi.generate_trajectory_times(wp, T1, dt)  # the row count rule: evaluateRange on the optimised times
    assert rows.shape == want.shape == plain.shape and len(rows) >= 38
    assert rows[:, 9].tobytes() == want[:, 9].tobytes()
    assert np.abs(rows - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    assert abs(rows[-1, 9] - plain[-1, 9]) <= 1e-12 * plain[-1, 9]
    assert np.abs(rows - plain).max() > 1e-3  # it is another trajectory
    # the C call reports the descent's outputs
    r2, j0, j1, it = capi.generate_trajectory_timeopt(wp, V_MAX, A_MAX, dt, return_costs=True)
    assert r2.tobytes() == rows.tobytes() and (j0, j1, it) == (J0[0], J1[0], iters[0])
    # (max_iter, h, t_min); max_iter = 0 is the plain trajectory
    same = pt.generate_trajectory(wp, V_MAX, A_MAX, dt, optimizeTimes=(0, 0.1, 0.1))
    assert same.shape == plain.shape and np.abs(same - plain).max() <= 1e-9 * max(1.0, np.abs(plain).max())
    assert pt.generate_trajectory(wp, V_MAX, A_MAX, dt, optimizeTimes=False).tobytes() == plain.tobytes()
    # optimise, then scale: with the limits enforced the peaks are within them
    lim = pt.generate_trajectory(wp, V_MAX, A_MAX, dt, enforceLimits=True, optimizeTimes=True)
    v = np.linalg.norm(lim[:, [1, 4, 7]], axis=1).max()
    assert v <= V_MAX * (1 + 2e-3) and lim[-1, 9] >= rows[-1, 9]
    for bad in ((5, 0.0, 0.1), (5, 0.1, 0.0), (5, -0.1, 0.1), (-1, 0.1, 0.1)):
        with pytest.raises(ValueError):
            pt.generate_trajectory(wp, V_MAX, A_MAX, dt, optimizeTimes=bad)


def test_argument_errors():
    t = TRACKS["m3"]
    for kw in (dict(h=0.0), dict(t_min=0.0), dict(t_min=-1.0), dict(step0=0.0), dict(step0=1.5)):
        with pytest.raises(capi.EppError):
            capi.optimize_times([t.wp], [t.T], capi.TimeoptParams(**kw))
    for h, t_min in ((0.0, 0.1), (0.1, 0.0), (-1.0, 0.1)):
        with pytest.raises(capi.EppError):
            capi.time_gradient([t.wp], [t.T], h, t_min)


def test_path_planner_candidate_snap_costs():
    import online_traj_planner as otp
    gates, obstacles = synth.track_world(42)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), CONFIG)
    sets = [TRACKS[n].wp for n in ("m2", "m3", "m4", "m12", "m1")]
    Ts, Cs, st = capi.minsnap_batch(sets, V_MAX, A_MAX)
    assert (st == 0).all()
    want, _ = capi.snap_cost(Ts, Cs)
    costs, times = pp.candidate_snap_costs(sets, V_MAX, A_MAX)
    assert costs.dtype == np.float64 and costs.tobytes() == want.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(times, Ts))
    Tn, Cn, J0, J1, iters, so = capi.optimize_times(sets, Ts)
    costs, times = pp.candidate_snap_costs(sets, V_MAX, A_MAX, optimize=True)
    assert costs.tobytes() == J1.tobytes() and (costs <= want).all() and (costs[:4] < want[:4]).all()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(times, Tn))
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_snap_costs([sets[0], sets[1][:1]], V_MAX, A_MAX)
    c, ts = pp.candidate_snap_costs([], V_MAX, A_MAX)
    assert c.shape == (0,) and len(ts) == 0
