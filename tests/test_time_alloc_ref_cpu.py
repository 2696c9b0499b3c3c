"""CPU: the truth of the segment-time allocation (time_alloc_ref.py) against what it must
satisfy on its own -- the closed-form cost against quadrature, the descent's invariants, its
distance from scipy's constrained optimum -- and the inputs of the GPU test: no decision of a
one-step case is a coin-flip, the clamp and a rejected first step are exercised.  Also the
presence of the new surface."""
import functools
import os

import numpy as np
import pytest

import time_alloc_inputs as ti
import time_alloc_ref as tr

from conftest import PKG, ROOT

TRACKS = ti.tracks()


@pytest.mark.parametrize("name", list(TRACKS))
def test_closed_form_cost_is_the_integral_of_snap_squared(name):
    t = TRACKS[name]
    C = tr.solve(t.wp, t.T, t.v0, t.a0)[0]
    J, Jq = tr.cost(t.T, C), tr.cost_by_quadrature(t.T, C)
    print(name, J, Jq, abs(J - Jq) / Jq)
    # 6-point Gauss-Legendre is exact for the degree-10 integrand: rounding only
    assert abs(J - Jq) <= 1e-12 * Jq
    # a random polynomial too (not a minimiser)
    rs = np.random.RandomState(len(name))
    T, C = rs.uniform(0.3, 2.5, 3), rs.uniform(-1, 1, (3, 3, 10))
    assert abs(tr.cost(T, C) - tr.cost_by_quadrature(T, C)) <= 1e-12 * tr.cost_by_quadrature(T, C)


def test_variants_are_mellingers():
    T = np.array([0.5, 1.0, 2.0])
    V = tr.variants(T, 0.1, 0.1)
    assert V.shape == (4, 3) and (V[0] == T).all()
    assert (V[1] == [0.5 + 0.1, 1.0 - 0.1 / 2.0, 2.0 - 0.1 / 2.0]).all()
    assert (V[3] == [0.5 - 0.1 / 2.0, 1.0 - 0.1 / 2.0, 2.0 + 0.1]).all()
    assert tr.variants([1.0], 0.1, 0.1).shape == (1, 1)  # M == 1: no gradient
    assert (tr.gradient(TRACKS["m1"].wp, TRACKS["m1"].T, 0.1, 0.1)[1] == 0.0).all()
    # M == 2: the other segment gives up all of h
    assert (tr.variants([1.0, 2.0], 0.1, 0.1)[1] == [1.0 + 0.1, 2.0 - 0.1]).all()
    # every direction sums to zero: the total is kept
    d = tr.direction([3.0, -1.0, 0.5, 7.0])
    assert abs(d.sum()) < 1e-15 and d[0] == 3.0 - (-1.0 + 0.5 + 7.0) / 3.0


def test_clamp_is_exercised():
    t = TRACKS["clamp"]
    V = tr.variants(t.T, ti.H, ti.T_MIN)
    assert (V[2:, 0] == ti.T_MIN).all() and V[1, 0] == t.T[0] + ti.H
    # the clamp changes the total of those variants; the quotient divides by h all the same
    assert abs(V[2].sum() - t.T.sum()) > 0.03


@functools.lru_cache(maxsize=None)
def _run(name, **kw):
    t = TRACKS[name]
    return tr.descent(t.wp, t.T, tr.DEFAULTS._replace(**kw), t.v0, t.a0)


@pytest.mark.parametrize("name", ["m2", "m3", "m4", "va", "clamp", "m12"])
def test_descent_invariants(name):
    t, r = TRACKS[name], _run(name)
    costs = [it.costs[0] for it in r.trace] + ([r.trace[-1].costs[-1]] if r.trace and r.trace[-1].halvings >= 0 else [])
    print(name, r.iters, r.status, r.cost0, r.cost1, costs)
    assert r.iters >= 1 and all(b < a for a, b in zip(costs, costs[1:]))  # monotone
    assert r.cost1 <= r.cost0
    assert abs(tr.seq_sum(r.T) - tr.seq_sum(t.T)) <= 1e-12 * tr.seq_sum(t.T)
    assert (r.T >= ti.T_MIN).all()


def test_degenerate_runs_return_the_plain_fit():
    t = TRACKS["m1"]
    r = tr.descent(t.wp, t.T)
    assert (r.iters, r.status) == (0, 0) and r.cost1 == r.cost0 and (r.T == t.T).all()
    r = _run("m3", max_iter=0)
    assert (r.iters, r.status) == (0, 0) and r.cost1 == r.cost0 and (r.T == TRACKS["m3"].T).all()


@pytest.mark.parametrize("name", ["m3", "m4"])
def test_gap_to_scipy(name):
    t = TRACKS[name]
    r = _run(name, max_iter=200, ftol=0.0)
    Ts, Js = tr.scipy_optimum(t.wp, t.T, ti.T_MIN)
    gap = (r.cost1 - Js) / Js
    print(f"{name}: descent {r.cost1!r} after {r.iters} steps (status {r.status}), SLSQP {Js!r}, relative gap {gap:.3e}")
    assert abs(Ts.sum() - t.T.sum()) <= 1e-9 * t.T.sum() and (Ts >= ti.T_MIN - 1e-12).all()
    # SLSQP works on the cost itself; the descent follows a forward difference of width h, so
    # it may stop short of the optimum but not below it
    assert -1e-9 <= gap <= 0.05
    assert Js < r.cost0


def test_one_step_cases_hold_no_coin_flip():
    seen_bound = seen_cost = 0
    for t, step0 in ti.one_step_cases():
        r = tr.descent(t.wp, t.T, tr.DEFAULTS._replace(max_iter=1, step0=step0), t.v0, t.a0)
        it = r.trace[0]
        print(t.name, step0, r.iters, r.status, it.halvings, it.cost_margin, it.tmin_margin, it.refused_bound,
              it.refused_cost)
        assert r.iters == 1 and it.halvings >= 0
        assert it.cost_margin > 1e-6 and it.tmin_margin > 1e-9
        seen_bound += it.refused_bound > 0
        seen_cost += it.refused_cost > 0
        # the step the GPU test rebuilds from a gradient is this step
        g = tr.gradient(t.wp, t.T, ti.H, ti.T_MIN, t.v0, t.a0)[1]
        assert np.abs(tr.step_from_grad(t.T, g, it.halvings, step0) - r.T).max() <= 1e-15 * r.T.max()
    assert seen_bound >= 1 and seen_cost >= 1  # a first alpha refused by t_min, and one by the cost


NEW = ("epp_traj_snap_cost", "epp_minsnap_time_gradient", "epp_minsnap_optimize_times",
       "epp_generate_trajectory_timeopt_host")


def test_surface():
    from eppamd import capi
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.snap_cost) and callable(capi.time_gradient) and callable(capi.optimize_times)
    import online_traj_planner as otp
    import polynomial_trajectory as pt
    assert hasattr(otp.PathPlanner, "candidate_snap_costs")
    assert "optimizeTimes" in pt.generate_trajectory.__doc__
    assert os.path.exists(os.path.join(PKG, "csrc", "time_alloc.h"))
    header = open(os.path.join(ROOT, "include", "epp.h")).read()
    assert all(name + "(" in header for name in NEW) and "EPP_TIMEOPT_DEFAULTS {0.1, 0.1, 0.5, 8, 1e-4, 20}" in header
    p = capi.TimeoptParams()
    assert (p.h, p.t_min, p.step0, p.max_halvings, p.ftol, p.max_iter) == tuple(tr.DEFAULTS)


def test_argument_checks():
    """They precede every device call, so they run without a GPU."""
    from eppamd import capi
    L, bad, p = capi.lib(), capi.EPP_ERR_INVALID_ARGUMENT, 0x1000
    for h, t_min in ((0.0, 0.1), (-0.1, 0.1), (0.1, 0.0), (0.1, -1.0), (float("nan"), 0.1), (0.1, float("nan"))):
        assert L.epp_minsnap_time_gradient(p, p, 1, None, None, p, h, t_min, p, p, p, None) == bad
        assert b"epp_minsnap_time_gradient" in L.epp_last_error()
    for kw in (dict(h=0.0), dict(h=-1.0), dict(t_min=0.0), dict(t_min=-0.1), dict(step0=0.0), dict(step0=-0.5),
               dict(step0=1.0 + 1e-9), dict(step0=float("nan")), dict(ftol=-1e-9), dict(max_halvings=-1),
               dict(max_iter=-1)):
        prm = capi.TimeoptParams(**kw)
        assert L.epp_minsnap_optimize_times(p, p, 1, None, None, p, p, prm, p, p, p, p, None) == bad, kw
        assert b"epp_minsnap_optimize_times" in L.epp_last_error()
        assert L.epp_minsnap_optimize_times(None, None, 0, None, None, None, None, prm, None, None, None, None,
                                            None) == bad, kw
    ok = capi.TimeoptParams(step0=1.0)
    assert L.epp_minsnap_optimize_times(None, None, 0, None, None, None, None, ok, None, None, None, None,
                                        None) == capi.EPP_OK
    assert L.epp_traj_snap_cost(None, None, None, 0, None, None, None) == capi.EPP_OK
    assert L.epp_traj_snap_cost(None, None, None, 1, None, None, None) == bad
    assert L.epp_minsnap_time_gradient(None, None, 0, None, None, None, 0.1, 0.1, None, None, None, None) == capi.EPP_OK
