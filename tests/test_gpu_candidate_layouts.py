"""GPU: PathPlanner's candidate calls where their device block is smallest and ragged.  Each
call lays out its own block (csrc/candidate_batch.h: the waypoints, times, coefficients,
offsets and statuses of the fit, then the call's outputs, every part 256-byte aligned), so a
wrong part size or offset shows where the parts are far from multiples of 256 bytes: one
single-segment set alone (n = 1), and it beside one longer set, either way round (n = 2).

By definition a candidate call is epp_minsnap_batch followed by the call's own stage on the
same tracks: every output equals, with == and the same dtype, the composition of
capi.minsnap_batch and the matching capi / World call.  The world, limits, dt and gate frames
are those of the call's own test (test_path_planner_candidate_* and the two *_candidate_trajectories
tests); the long set is one of that test's fit inputs and the short set its first two
waypoints.  A fit that fails is never handed to a stage: the fit's status is asserted first.
"""
import functools

import numpy as np
import pytest

import clearance_inputs as ci
import gatepass_inputs as gi
import small_path_inputs as spi
import thrust_rates_inputs as ti
import thrust_scale_inputs as si
import time_alloc_inputs as tai
import trajsweep_inputs as tsi
from conftest import CONFIG
from eppamd import capi, config, synth
from test_gpu_clearance import _world as _clearance_world
from test_gpu_trajcheck import DT, _world as _fit_world

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _planner(kind):
    import online_traj_planner as otp
    if kind == "obbs":  # the 72-OBB world of the check, sweep, clearance and first-hit tests
        gates, obstacles = spi.poses(72)
        return otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)
    gates, obstacles = synth.track_world(42)
    return otp.PathPlanner(np.array(gates), np.array(obstacles), CONFIG)


@functools.lru_cache(maxsize=None)
def _gates():
    """(frames, a lap through the gates): test_path_planner_candidate_gate_passes' inputs."""
    gates, _ = synth.track_world(42)
    geom = config.geometry(config.load(CONFIG))
    frames = _planner("track").gate_frames(gates)
    cps = synth.gate_checkpoints(gates, np.array([float(h) for h in geom.gate_height]), 0.55)
    lap = np.concatenate([[cps[2 * g], (cps[2 * g] + cps[2 * g + 1]) / 2, cps[2 * g + 1]] for g in range(len(gates))])
    return frames, lap


def _sweep_expected(Ts, Cs, cp):
    world, _ = _fit_world(72)
    rows, row_times = world.check_trajectories(Ts, Cs, 0.1, 0.05)
    chords, chord_times = world.sweep_trajectories(Ts, Cs, 0.1, cp)
    row_first = (rows >= 0) & ((chords < 0) | (rows <= chords))
    found = (rows >= 0) | (chords >= 0)
    return rows, chords, np.where(found, np.where(row_first, row_times, chord_times), -1.0)


def _flyable_expected(Ts, Cs):
    Tn, _, scale, status, viol = capi.scale_to_thrust_limits(Ts, Cs, *si.L_FIT)
    assert (status >= 0).all()
    duration = np.array([functools.reduce(lambda a, b: a + b, T.tolist(), 0.0) for T in Tn])
    return scale, duration, status, viol


def _snap_expected(sets, Ts, Cs, optimize):
    if not optimize:
        cost, st = capi.snap_cost(Ts, Cs)
        assert (st >= 0).all()
        return cost, Ts
    Tn, _, _, J1, _, st = capi.optimize_times(sets, Ts)
    assert (st >= 0).all()
    return J1, Tn


def _snap_got(sets, optimize):
    costs, times = _planner("track").candidate_snap_costs(sets, 1.0, 2.0, optimize=optimize)
    return costs, times


# name -> (the long set, v_max, a_max, the call on sets, the composition on (sets, Ts, Cs), the
# dtypes of the outputs)
CALLS = {
    "check_candidate_trajectories": (
        lambda: synth.random_track_waypoints(903, 22), 1.0, 2.0,
        lambda sets: _planner("obbs").check_candidate_trajectories(sets, 1.0, 2.0, DT, 0.05),
        lambda sets, Ts, Cs: _fit_world(72)[0].check_trajectories(Ts, Cs, DT, 0.05),
        [np.int64, np.float64]),
    "sweep_candidate_trajectories": (
        lambda: tsi.fit_waypoints()[3], 1.0, 2.0,
        lambda sets: _planner("obbs").sweep_candidate_trajectories(sets, 1.0, 2.0, 0.1, 0.05, False),
        lambda sets, Ts, Cs: _sweep_expected(Ts, Cs, False),
        [np.int64, np.int64, np.float64]),
    "sweep_candidate_trajectories-can_pass": (
        lambda: tsi.fit_waypoints()[3], 1.0, 2.0,
        lambda sets: _planner("obbs").sweep_candidate_trajectories(sets, 1.0, 2.0, 0.1, 0.05, True),
        lambda sets, Ts, Cs: _sweep_expected(Ts, Cs, True),
        [np.int64, np.int64, np.float64]),
    "candidate_clearances": (
        lambda: tsi.fit_waypoints()[3], 1.0, 2.0,
        lambda sets: _planner("obbs").candidate_clearances(sets, 1.0, 2.0, ci.FIT_DT),
        lambda sets, Ts, Cs: _clearance_world("72").trajectory_clearance(Ts, Cs, ci.FIT_DT),
        [np.float64, np.int64, np.float64, np.int32]),
    "candidate_first_hits": (
        lambda: tsi.fit_waypoints()[3], 1.0, 2.0,
        lambda sets: _planner("obbs").candidate_first_hits(sets, 1.0, 2.0, 0.1, False),
        lambda sets, Ts, Cs: _fit_world(72)[0].trajectory_first_hits(Ts, Cs, 0.1, False),
        [np.int64, np.float64, np.float64, np.int32]),
    "candidate_gate_passes": (
        lambda: _gates()[1], 1.0, 2.0,
        lambda sets: _planner("track").candidate_gate_passes(sets, 1.0, 2.0, 0.05, _gates()[0], gi.HE),
        lambda sets, Ts, Cs: capi.trajectory_gate_passes(_gates()[0], gi.HE, Ts, Cs, 0.05),
        [np.int64, np.float64, np.float64, np.int32]),
    "candidate_thrust_rates": (
        lambda: np.asarray(ti.fit_waypoints()[3]), 1.0, 2.0,
        lambda sets: _planner("track").candidate_thrust_rates(sets, 1.0, 2.0, 0.05, 9.81),
        lambda sets, Ts, Cs: capi.trajectory_thrust_rates(Ts, Cs, 0.05, 9.81),
        [np.float64, np.int64]),
    "candidate_flyable_scales": (
        lambda: np.asarray(si.fit_waypoints()[3]), si.V_MAX, si.A_MAX,
        lambda sets: _planner("track").candidate_flyable_scales(sets, si.V_MAX, si.A_MAX, tuple(si.L_FIT)),
        lambda sets, Ts, Cs: _flyable_expected(Ts, Cs),
        [np.float64, np.float64, np.int32, np.int32]),
    "candidate_snap_costs": (
        lambda: tai.tracks()["m12"].wp, 1.0, 2.0,
        lambda sets: _snap_got(sets, False),
        lambda sets, Ts, Cs: _snap_expected(sets, Ts, Cs, False),
        [np.float64]),
    "candidate_snap_costs-optimize": (
        lambda: tai.tracks()["m12"].wp, 1.0, 2.0,
        lambda sets: _snap_got(sets, True),
        lambda sets, Ts, Cs: _snap_expected(sets, Ts, Cs, True),
        [np.float64]),
}
ORDERS = {"short,long": lambda s, l: [s, l], "long,short": lambda s, l: [l, s], "short": lambda s, l: [s]}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", list(CALLS))
def test_candidate_call_equals_fit_then_stage(name, order):
    long_set, v_max, a_max, call, composition, dtypes = CALLS[name]
    long = np.asarray(long_set(), np.float64)
    assert len(long) > 2
    sets = ORDERS[order](long[:2], long)
    Ts, Cs, st = capi.minsnap_batch(sets, v_max, a_max)
    assert (st == 0).all()  # (before any stage runs on the tracks)
    assert sorted(len(T) for T in Ts) == sorted(len(s) - 1 for s in sets) and min(len(T) for T in Ts) == 1
    exp = composition(sets, Ts, Cs)
    got = call(sets)
    if name.startswith("candidate_snap_costs"):  # (costs, the list of each set's segment times)
        assert len(got[1]) == len(exp[1]) == len(sets)
        for a, b in zip(got[1], exp[1]):
            assert a.dtype == np.float64 and np.array_equal(a, b)
        got, exp = got[:1], exp[:1]
    assert len(got) == len(exp) == len(dtypes)
    for g, e, dt in zip(got, exp, dtypes):
        assert g.dtype == e.dtype == dt, (g.dtype, e.dtype, dt)
        assert g.shape == e.shape and np.array_equal(g, e, equal_nan=(dt == np.float64)), (g, e)


@pytest.mark.parametrize("name", list(CALLS))
def test_candidate_call_edges(name):
    """A one-waypoint set is refused; an empty list gives empty arrays of the call's dtypes."""
    long_set, _, _, call, _, dtypes = CALLS[name]
    long = np.asarray(long_set(), np.float64)
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        call([long, long[:1]])
    got = call([])
    if name.startswith("candidate_snap_costs"):
        assert isinstance(got[1], list) and len(got[1]) == 0
        got = got[:1]
    assert len(got) == len(dtypes)
    for g, dt in zip(got, dtypes):
        assert g.dtype == dt and g.shape[0] == 0 and g.size == 0
