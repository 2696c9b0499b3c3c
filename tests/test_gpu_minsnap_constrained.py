"""GPU parity: the min-snap fit with end states and derivatives pinned at waypoints
(epp_minsnap_batch_constrained, k_minsnap_constrained) vs the CPU oracle's general solve.

Tolerances: coefficients within the project's 1e-6 of oracle.minsnap_solve at the same times
(the oracle itself is within 1e-7 of a refined truth on every input here:
test_constrained_fit_inputs_cpu.py); segment times to 1e-12 relative; a pinned derivative
within 1e-9 absolute of its value on both sides of the waypoint (the tolerance
test_generate_trajectory_vs_oracle uses for the start state); free derivatives continuous to
1e-6 (as test_large_batch_property checks).
"""
import ctypes as C
from math import factorial

import numpy as np
import pytest

import constrained_fit_inputs as CI
import oracle as O
from eppamd import capi, synth

gpu = pytest.mark.gpu

COEF_TOL = 1e-6
PIN_TOL = 1e-9
CONT_TOL = 1e-6
EPP_ERR_INVALID_ARGUMENT = -1


def _fit(cases, caller_times=False):
    return capi.minsnap_batch_constrained([c.wp for c in cases], CI.V_MAX, CI.A_MAX, [c.mask for c in cases],
                                          [c.values for c in cases], [c.T for c in cases] if caller_times else None)


def _check_vs_oracle(cases, Ts, Cs, st, label):
    assert (st == 0).all(), st
    worst = 0.0
    for c, T, Cf in zip(cases, Ts, Cs):
        np.testing.assert_allclose(T, c.T, rtol=1e-12, atol=0, err_msg=c.what)
        err = np.abs(Cf - c.oracle_coeffs()).max()
        worst = max(worst, err)
        assert err < COEF_TOL, (c.what, err)
    print(f"{label}: worst coefficient difference from the oracle {worst:.3e}")


def _deriv(c, t, k):
    """derivative k of the polynomial c (increasing powers) at t"""
    return sum(factorial(j) // factorial(j - k) * c[j] * t ** (j - k) for j in range(k, 10))


def _vertex_sides(T, Cf, v, k):
    """derivative k (3-vector) at vertex v from the segment before (None at the start) and
    from the segment after (None at the end)"""
    M = len(T)
    before = np.array([_deriv(Cf[v - 1, d], T[v - 1], k) for d in range(3)]) if v > 0 else None
    after = np.array([_deriv(Cf[v, d], 0.0, k) for d in range(3)]) if v < M else None
    return before, after


# ---- 1. against the oracle --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_seg", CI.SEGMENTS)
def test_batch_vs_oracle(n_seg):
    """1 segment: no system, only the two end states; 2: one inner vertex, the middle step
    only; 3: the bottom sweep has one step and the top none; 40 / 41: LDS against global
    segment scratch.  Each batch mixes random {velocity, acceleration} pins, velocity pinned at
    every inner waypoint, and full end states (end velocity / acceleration, start jerk / snap)."""
    cases = CI.batch(n_seg)
    Ts, Cs, st = _fit(cases)
    _check_vs_oracle(cases, Ts, Cs, st, f"{n_seg} segments")


@gpu
def test_ragged_batch_with_caller_times():
    cases = CI.ragged_batch()
    Ts, Cs, st = _fit(cases, caller_times=True)
    for c, T in zip(cases, Ts):
        assert T.tobytes() == c.T.tobytes()  # the caller's times come back as they went in
    _check_vs_oracle(cases, Ts, Cs, st, "ragged, caller times")


# ---- 2. where the elimination changes shape ---------------------------------------------------
@gpu
def test_single_pin_at_each_place_of_the_elimination():
    """9 segments: a single pin at inner vertex 1 (the top sweep's start), at the last (the
    bottom's start), at the meeting vertex m = 4 and at both its neighbours (each sweep's last
    step), and all four derivatives pinned at m (the system decouples there)."""
    cases = CI.shape_batch()
    Ts, Cs, st = _fit(cases)
    _check_vs_oracle(cases, Ts, Cs, st, "elimination shapes")


# ---- 3. the constraints hold ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", ["5", "12", "41", "ragged", "shapes"])
def test_constraints_hold(which):
    cases = {"ragged": CI.ragged_batch, "shapes": CI.shape_batch}.get(which, lambda: CI.batch(int(which)))()
    Ts, Cs, st = _fit(cases, caller_times=which == "ragged")
    assert (st == 0).all()
    worst_pin = worst_free = 0.0
    for c, T, Cf in zip(cases, Ts, Cs):
        used = c.used()
        W = len(c.wp)
        for v in range(W):
            for k in range(1, 5):
                before, after = _vertex_sides(T, Cf, v, k)
                if used[v, k - 1]:  # (the end vertex carries the given end state: used there)
                    for side in (before, after):
                        if side is not None:
                            err = np.abs(side - c.values[v, k - 1]).max()
                            worst_pin = max(worst_pin, err)
                            assert err <= PIN_TOL, (c.what, v, k, err)
                else:
                    err = np.abs(before - after).max()
                    worst_free = max(worst_free, err)
                    assert err <= CONT_TOL, (c.what, v, k, err)
            before, after = _vertex_sides(T, Cf, v, 0)  # and the positions
            for side in (before, after):
                if side is not None:
                    assert np.abs(side - c.wp[v]).max() <= PIN_TOL, (c.what, v)
    print(f"{which}: pinned values off by at most {worst_pin:.3e}, free derivatives by {worst_free:.3e}")


# ---- 4. reduces to the plain fit --------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_seg", [1, 12, 41])
def test_reduces_to_the_plain_fit(n_seg):
    """Mask 0 inside and ends [v0, a0, 0, 0] / 0 is epp_minsnap_batch's fit: the same segment
    times bit for bit, coefficients within 1e-6 (bit equality is expected -- the policy adds
    only predicated terms -- but depends on the compiler's scheduling, so the largest
    difference is printed, not asserted to be 0).  NaN in every unused inner slot gives the same
    bits as zeros there."""
    tracks = [synth.random_track_waypoints(8000 + 13 * n_seg + k, n_seg) for k in range(CI.N_TRACKS)]
    rs = np.random.RandomState(n_seg)
    v0, a0 = rs.uniform(-0.5, 0.5, (CI.N_TRACKS, 3)), rs.uniform(-0.5, 0.5, (CI.N_TRACKS, 3))
    Tp, Cp, stp = capi.minsnap_batch(tracks, CI.V_MAX, CI.A_MAX, v0, a0)
    masks = [np.zeros(n_seg + 1, np.uint8) for _ in tracks]
    zeros, nans = [], []
    for k in range(CI.N_TRACKS):
        val = np.zeros((n_seg + 1, 4, 3))
        val[0, 0], val[0, 1] = v0[k], a0[k]
        zeros.append(val)
        val = val.copy()
        val[1:-1] = np.nan
        nans.append(val)
    Tz, Cz, stz = capi.minsnap_batch_constrained(tracks, CI.V_MAX, CI.A_MAX, masks, zeros)
    Tn, Cn, stn = capi.minsnap_batch_constrained(tracks, CI.V_MAX, CI.A_MAX, masks, nans)
    assert (stp == 0).all() and (stz == 0).all() and (stn == 0).all()
    worst = 0.0
    for k in range(CI.N_TRACKS):
        assert Tz[k].tobytes() == Tp[k].tobytes()
        worst = max(worst, np.abs(Cz[k] - Cp[k]).max())
        assert Tn[k].tobytes() == Tz[k].tobytes() and Cn[k].tobytes() == Cz[k].tobytes()
    print(f"{n_seg} segments: constrained fit with no pins vs epp_minsnap_batch: largest difference {worst:.3e}")
    assert worst < COEF_TOL


# ---- 5. self-consistency without the oracle ---------------------------------------------------
@gpu
@pytest.mark.parametrize("n_seg", [2, 12, 41])
def test_pinning_a_fits_own_derivatives_gives_the_fit_back(n_seg):
    cases = CI.batch(n_seg)[2::3]  # free inside, full end states
    Ts, Cs, st = _fit(cases)
    assert (st == 0).all()
    masks, values = [], []
    for c, Cf in zip(cases, Cs):
        mask, val = c.mask.copy(), c.values.copy()
        mask[1:-1] = 3
        for v in range(1, n_seg):
            val[v, 0] = Cf[v, :, 1]
            val[v, 1] = 2.0 * Cf[v, :, 2]
        masks.append(mask)
        values.append(val)
    T2, C2, st2 = capi.minsnap_batch_constrained([c.wp for c in cases], CI.V_MAX, CI.A_MAX, masks, values)
    assert (st2 == 0).all()
    worst = max(np.abs(a - b).max() for a, b in zip(Cs, C2))
    print(f"{n_seg} segments: refit with the fit's own velocities and accelerations pinned: {worst:.3e}")
    assert worst < COEF_TOL


# ---- 6. statuses ------------------------------------------------------------------------------
@gpu
def test_statuses_in_one_mixed_launch():
    good = list(CI.batch(5)[:4])
    c = good[1]
    one = CI.Case(np.zeros((1, 3)), np.zeros(1, np.uint8), np.zeros((1, 4, 3)), "one waypoint", np.zeros(0))
    t_bad = c.T.copy()
    t_bad[2] = 0.0
    bad_time = CI.Case(c.wp, c.mask, c.values, "a caller time of 0", t_bad)
    m_bad = good[0].mask.copy()
    m_bad[2] |= 0x10
    bad_bit = CI.Case(good[0].wp, m_bad, good[0].values, "bit 4 set")
    v_bad = good[1].values.copy()
    assert good[1].mask[3] & 1  # (velocity is pinned at every inner waypoint of this track)
    v_bad[3, 0, 1] = np.nan
    bad_nan = CI.Case(good[1].wp, good[1].mask, v_bad, "NaN in a used slot")
    v_inf = good[2].values.copy()
    v_inf[-1, 3, 0] = np.inf  # the end vertex's snap: used whatever the mask says
    bad_inf = CI.Case(good[2].wp, good[2].mask, v_inf, "inf in the end state")
    cases = [good[0], one, good[1], bad_time, bad_bit, good[2], bad_nan, bad_inf, good[3]]
    Ts, Cs, st = _fit(cases, caller_times=True)
    assert st.tolist() == [0, -1, 0, -2, -4, 0, -4, -4, 0]
    for k in (4, 6, 7):  # -4: the track is left unwritten (the wrapper zeroed the outputs)
        assert not Ts[k].any() and not Cs[k].any()
    assert not Cs[3].any()
    # the good tracks beside them: what they are in a launch of their own
    Tg, Cg, stg = _fit(good, caller_times=True)
    assert (stg == 0).all()
    for k, j in zip((0, 2, 5, 8), range(4)):
        assert Ts[k].tobytes() == Tg[j].tobytes() and Cs[k].tobytes() == Cg[j].tobytes()
        assert np.abs(Cs[k] - good[j].oracle_coeffs()).max() < COEF_TOL


def test_null_tables_and_empty_batch():
    """Both are answered before any device call, so this runs without a GPU."""
    L = capi.lib()
    p = np.zeros(64).ctypes.data  # a stand-in for device pointers: rejected before anything is read
    assert L.epp_minsnap_batch_constrained(p, p, 1, 1.0, 2.0, None, None, p, p, p, p, None) == EPP_ERR_INVALID_ARGUMENT
    assert L.epp_minsnap_batch_constrained(p, p, 1, 1.0, 2.0, None, p, None, p, p, p, None) == EPP_ERR_INVALID_ARGUMENT
    assert b"epp_minsnap_batch_constrained" in L.epp_last_error()
    assert L.epp_minsnap_batch_constrained(p, p, -1, 1.0, 2.0, None, p, p, p, p, p, None) == EPP_ERR_INVALID_ARGUMENT
    # an empty batch launches nothing: every pointer may be NULL
    assert L.epp_minsnap_batch_constrained(None, None, 0, 1.0, 2.0, None, None, None, None, None, None, None) == 0
    assert capi.minsnap_batch_constrained([], 1.0, 2.0, [], [])[2].shape == (0,)
    rows, n = C.POINTER(C.c_double)(), C.c_int64(0)
    wp = np.zeros((3, 3))
    assert L.epp_generate_trajectory_constrained_host(wp.ctypes.data, 3, 1.0, 2.0, None, 0.1, 0.0, None, p,
                                                      C.byref(rows), C.byref(n)) == EPP_ERR_INVALID_ARGUMENT
    assert L.epp_generate_trajectory_constrained_host(wp.ctypes.data, 1, 1.0, 2.0, None, 0.1, 0.0, p, p,
                                                      C.byref(rows), C.byref(n)) == EPP_ERR_INVALID_ARGUMENT
    assert b"At least two waypoints" in L.epp_last_error()


# ---- 7. host and Python layers ----------------------------------------------------------------
@gpu
def test_generate_trajectory_keywords_are_the_constrained_fit_sampled():
    import polynomial_trajectory as pt
    n_seg = 7
    wp = synth.random_track_waypoints(8500, n_seg)
    v0, a0, vf, af = (0.3, -0.2, 0.1), (0.0, 0.4, -0.1), (0.2, 0.1, -0.3), (-0.1, 0.0, 0.2)
    j0, s0 = (0.1, -0.3, 0.2), (0.2, 0.2, -0.1)
    wvel = [None] * (n_seg + 1)
    wacc = [None] * (n_seg + 1)
    wvel[2], wvel[5], wacc[5] = (0.4, -0.1, 0.0), (-0.2, 0.3, 0.1), (0.1, 0.1, -0.2)
    got = pt.generate_trajectory(wp, CI.V_MAX, CI.A_MAX, 0.1, 3.25, v0, a0, finalVel=vf, finalAcc=af,
                                 initialJerk=j0, initialSnap=s0, waypointVel=wvel, waypointAcc=wacc)
    mask = np.zeros(n_seg + 1, np.uint8)
    val = np.zeros((n_seg + 1, 4, 3))
    val[0] = [v0, a0, j0, s0]
    val[-1, :2] = [vf, af]
    mask[2], mask[5] = 1, 3
    val[2, 0], val[5, 0], val[5, 1] = wvel[2], wvel[5], wacc[5]
    Ts, Cs, st = capi.minsnap_batch_constrained([wp], CI.V_MAX, CI.A_MAX, [mask], [val])
    assert st[0] == 0
    exp = capi.sample_batch(Ts, Cs, 0.1, [3.25])
    assert got.shape == exp.shape and len(got) > 10
    assert np.array_equal(got[:, 9], exp[:, 9])  # time column exact
    assert np.abs(got[:, :9] - exp[:, :9]).max() < 1e-6
    # the same rows from the ctypes wrapper of the host call, and against the oracle
    got2 = capi.generate_trajectory_constrained(wp, CI.V_MAX, CI.A_MAX, 0.1, mask, val, t0=3.25)
    assert got2.tobytes() == got.tobytes()
    c = CI.Case(wp, mask, val, "keywords")
    ref = O.sample_traj(c.T, c.oracle_coeffs(), 0.1, 3.25)
    assert ref.shape == got.shape and np.abs(got[:, :9] - ref[:, :9]).max() < 1e-6
    # starts and ends in the given states
    np.testing.assert_allclose(got[0, [1, 4, 7]], v0, atol=PIN_TOL)
    np.testing.assert_allclose(got[0, [2, 5, 8]], a0, atol=PIN_TOL)
    # with none of the keywords: today's path, today's rows
    plain = pt.generate_trajectory(wp, CI.V_MAX, CI.A_MAX, 0.1, 3.25, v0, a0)
    assert plain.tobytes() == capi.generate_trajectory(wp, CI.V_MAX, CI.A_MAX, 0.1, 3.25, v0, a0).tobytes()
    # caller times through the host call
    T = c.T * 1.1
    got3 = capi.generate_trajectory_constrained(wp, 0.0, 0.0, 0.1, mask, val, seg_times=T)
    Ts3, Cs3, st3 = capi.minsnap_batch_constrained([wp], 0.0, 0.0, [mask], [val], [T])
    exp3 = capi.sample_batch(Ts3, Cs3, 0.1)
    assert st3[0] == 0 and got3.shape == exp3.shape and np.array_equal(got3[:, 9], exp3[:, 9])
    assert np.abs(got3[:, :9] - exp3[:, :9]).max() < 1e-6
    # a bad table is an invalid argument of the host call
    bad = val.copy()
    bad[2, 0, 0] = np.nan
    with pytest.raises(capi.EppError) as e:
        capi.generate_trajectory_constrained(wp, CI.V_MAX, CI.A_MAX, 0.1, mask, bad)
    assert e.value.code == EPP_ERR_INVALID_ARGUMENT


def test_generate_trajectory_keyword_combinations_raise():
    """Refused before any device call, so this runs without a GPU."""
    import polynomial_trajectory as pt
    wp = synth.random_track_waypoints(8501, 4)
    pins = [dict(finalVel=(0.1, 0, 0)), dict(finalAcc=(0.1, 0, 0)), dict(initialJerk=(0.1, 0, 0)),
            dict(initialSnap=(0.1, 0, 0)), dict(waypointVel=[None, (0.1, 0, 0), None, None, None]),
            dict(waypointAcc=[None, None, (0.1, 0, 0), None, None])]
    others = [dict(enforceLimits=True), dict(thrustLimits=(9.81, 1.0, 30.0, 10.0, 0.2)), dict(optimizeTimes=True),
              dict(optimizeTimes=(5, 0.1, 0.1))]
    for p in pins:
        for o in others:
            with pytest.raises(ValueError):
                pt.generate_trajectory(wp, 1.0, 2.0, 0.1, **p, **o)
    with pytest.raises(ValueError):  # one entry per waypoint
        pt.generate_trajectory(wp, 1.0, 2.0, 0.1, waypointVel=[None, (0.1, 0, 0)])
    with pytest.raises(ValueError):  # the end states have their own keywords
        pt.generate_trajectory(wp, 1.0, 2.0, 0.1, waypointVel=[(0.1, 0, 0), None, None, None, None])
    with pytest.raises(TypeError):  # keyword-only
        pt.generate_trajectory(wp, 1.0, 2.0, 0.1, 0.0, None, None, False, None, None, (0.1, 0, 0))


def test_gate_velocity_pins():
    """Host code: the gate frame's y axis (sin yaw, cos yaw, 0) -- gate_pass.h: a crossing goes
    from negative to positive gate-frame y -- times the speed, with the sign of the direction
    of travel."""
    yaws = np.array([0.0, np.pi / 2, 0.3])
    centres = np.array([[0.0, 1.0, 1.0], [2.0, 2.0, 1.2], [4.0, 1.0, 0.9]])
    frames = capi.gate_frames(centres, yaws)
    # start, gate 0 flown along +y, a free waypoint, gate 1 flown along +x (its normal at yaw pi/2),
    # gate 2 flown against its normal, end (at a gate: left alone)
    wp = np.array([[0.0, 0.0, 1.0], centres[0], [1.0, 2.0, 1.1], centres[1], centres[2], [4.0, -1.0, 1.0]])
    mask, val = capi.gate_velocity_pins(frames, wp, [-1, 0, -1, 1, 2, 2], 2.5)
    assert mask.dtype == np.uint8 and mask.tolist() == [0, 1, 0, 1, 1, 0]
    assert val.shape == (6, 4, 3) and not val[[0, 2, 5]].any() and not val[:, 1:].any()
    np.testing.assert_allclose(val[1, 0], [0.0, 2.5, 0.0], atol=1e-15)
    np.testing.assert_allclose(val[3, 0], [2.5, 0.0, 0.0], atol=1e-15)
    n2 = np.array([np.sin(0.3), np.cos(0.3), 0.0])
    np.testing.assert_allclose(val[4, 0], -2.5 * n2, atol=1e-15)  # travelling towards -y: the normal flipped
    for w in (1, 3, 4):
        assert np.dot(val[w, 0], wp[w + 1] - wp[w - 1]) >= 0.0
        assert abs(np.linalg.norm(val[w, 0]) - 2.5) < 1e-12
    with pytest.raises(ValueError):
        capi.gate_velocity_pins(frames, wp, [-1, 0], 1.0)
    with pytest.raises(ValueError):
        capi.gate_velocity_pins(frames, wp, [-1, 3, -1, -1, -1, -1], 1.0)
