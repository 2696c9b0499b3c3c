"""Inputs of the thrust / body-rate tests (test_gpu_thrust_rates.py) and of the CPU test of
those inputs (test_thrust_rates_inputs_cpu.py): fitted waypoint sets and hand-built coefficient
tracks, with the outcome each one claims.

The hand-built tracks are sampled at DT = 2^-6 s and every coefficient, row time and
acceleration of theirs is an exact double, so the rows on which their extremes fall hold
whatever the rounding of a square root.  G = 9.8125 is exactly representable.

Everything is input data: built once per process, shared, read-only.
"""
import functools
import os
import re

import numpy as np

from eppamd import synth

DT = 2.0 ** -6
G = 9.8125
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "efficient-path-planner_amd", "csrc")
K_SEG_LDS = int(re.search(r"kTcSegLds = (\d+);", open(os.path.join(_CSRC, "traj_walk.h")).read()).group(1))
ROW_CHUNK = int(re.search(r"kRowChunk = (\d+);", open(os.path.join(_CSRC, "traj_sample.h")).read()).group(1))
assert ROW_CHUNK == 512  # (the chunk-boundary tracks below are written for it)

R_LONG = 1100  # rows of the long hand-built tracks: more than two chunks
LAST = R_LONG - 1
MIN_ROWS = (0, 63, 64, 511, 512, 513, 1023, 1024, LAST)
SLOPE = 0.75  # m/s^3: 6 * 2^-3, so c3 = SLOPE / 6 = 2^-3 is exact

IDENTITY = [np.inf, -1.0, -np.inf, -1.0, -np.inf, -1.0, np.inf, -1.0]


def one_segment(R, coeffs):
    """(T, C) of one segment of R rows at DT; coeffs: {(axis, power): value}."""
    c = np.zeros((1, 3, 10))
    for (d, p), v in coeffs.items():
        c[0, d, p] = v
    return np.array([(R - 0.5) * DT]), c


def thrust_min_at(r, R=R_LONG):
    """a_x = SLOPE (t - r DT), a_y = a_z = 0: |F|^2 = a_x^2 + G^2 is smallest exactly on row r,
    the rate G SLOPE / |F|^2 largest there; the thrust is largest and cos_tilt smallest on the
    end farther from r."""
    return one_segment(R, {(0, 3): SLOPE / 6.0, (0, 2): -SLOPE * (r * DT) / 2.0})


def rate_inf_at(r, R=R_LONG):
    """Free fall with a sideways jerk: a_z = -G, a_x = 2^-560 (its square underflows to 0, so
    f2 == 0 wherever a_y == 0), a_y = J (t - r DT) with J = 6 * 2^400: on row r, and only
    there, thrust = 0, cos_tilt = 0 / 0 = NaN and rate = sqrt(36 * 2^-320) / 0 = +inf."""
    c3 = 2.0 ** 400
    return one_segment(R, {(2, 2): -G / 2.0, (0, 2): 2.0 ** -561, (1, 3): c3, (1, 2): -6.0 * c3 * (r * DT) / 2.0})


assert K_SEG_LDS == 40  # (MANY_ROW below is counted for 41 segments)
MANY_ROW = 222


def many_segments():
    """kTcSegLds + 1 segments of 5.5 DT each, so the segment times come through L2: the rows'
    times in their segments run 0..5 DT (segment 0), 0.5..5.5 DT (odd segments) and 1..5 DT
    (the other even ones: 6 + 6 + 19 * (5 + 6) = 221 rows before the last).  In every segment
    but the last the thrust minimum lies at 2.25 DT (segment 0: 5.75 DT), which no row has; in
    the last one at 2 DT: row 222.  The thrust is largest where a row is farthest from its
    segment's minimum: row 0, 5.75 DT from it (3.25 DT at most elsewhere)."""
    n = K_SEG_LDS + 1
    c = np.tile(one_segment(8, {(0, 3): SLOPE / 6.0, (0, 2): -SLOPE * (2.25 * DT) / 2.0})[1], (n, 1, 1))
    c[0] = one_segment(8, {(0, 3): SLOPE / 6.0, (0, 2): -SLOPE * (5.75 * DT) / 2.0})[1][0]
    c[-1] = thrust_min_at(2, 8)[1][0]
    return np.full(n, 5.5 * DT), c


@functools.lru_cache(maxsize=None)
def hand_tracks():
    """(names, Ts, Cs, want_out (K, 8) with NaN where nothing is claimed, want_rows (K, 4) with
    -2 where nothing is claimed)."""
    nan = np.nan
    t_last = LAST * DT
    cases = [
        # (a) every row the same bits: all four extremes answer row 0 (ties across lanes and chunks)
        ("constant acceleration", one_segment(R_LONG, {(0, 2): 0.5, (1, 2): 0.25, (2, 2): 1.0}),
         [nan, 0.0, nan, 0.0, 0.0, 0.0, nan, 0.0], [0, 0, 0, 0]),
        # (b) z = -(G / 2) t^2: F = 0 on every row; 0 / 0 = NaN never updates
        ("free fall", one_segment(R_LONG, {(2, 2): -G / 2.0}),
         [0.0, 0.0, 0.0, 0.0, -np.inf, -1.0, np.inf, -1.0], [0, 0, -1, -1]),
        # (b') x / 0 = +inf updates the maximum
        ("free fall, sideways jerk, row 0", rate_inf_at(0), [0.0, 0.0, nan, t_last, np.inf, 0.0, nan, nan],
         [0, LAST, 0, -2]),
        ("free fall, sideways jerk, row 700", rate_inf_at(700), [0.0, 700 * DT, nan, 0.0, np.inf, 700 * DT, nan, nan],
         [700, 0, 700, -2]),
        ("hover", one_segment(40, {(0, 0): 1.0, (1, 1): 2.0}), [G, 0.0, G, 0.0, 0.0, 0.0, 1.0, 0.0], [0, 0, 0, 0]),
    ]
    # (c) the thrust minimum exactly on a chosen row: the lane, wave-reduce and chunk boundaries
    for r in MIN_ROWS:
        far = LAST if r < LAST - r else 0
        cases.append((f"thrust minimum on row {r}", thrust_min_at(r),
                      [G, r * DT, nan, far * DT, SLOPE / G, r * DT, nan, far * DT], [r, far, r, far]))
    cases += [
        ("thrust minimum on the last of 512 rows", thrust_min_at(511, 512),
         [G, 511 * DT, nan, 0.0, SLOPE / G, 511 * DT, nan, 0.0], [511, 0, 511, 0]),
        ("thrust minimum on the last of 513 rows", thrust_min_at(512, 513),
         [G, 512 * DT, nan, 0.0, SLOPE / G, 512 * DT, nan, 0.0], [512, 0, 512, 0]),
        ("1 row", thrust_min_at(0, 1), [G, 0.0, G, 0.0, SLOPE / G, 0.0, 1.0, 0.0], [0, 0, 0, 0]),
        # (d) tracks without rows, mixed into the batch
        ("one waypoint", (np.zeros(0), np.zeros((0, 3, 10))), IDENTITY, [-1, -1, -1, -1]),
        ("NaN times", (np.full(2, np.nan), np.full((2, 3, 10), np.nan)), IDENTITY, [-1, -1, -1, -1]),
        (f"{K_SEG_LDS + 1} segments", many_segments(),
         [G, MANY_ROW * DT, nan, 0.0, SLOPE / G, MANY_ROW * DT, nan, 0.0], [MANY_ROW, 0, MANY_ROW, 0]),
    ]
    # one-waypoint and NaN tracks between the others too
    cases.insert(3, ("one waypoint (early)", (np.zeros(0), np.zeros((0, 3, 10))), IDENTITY, [-1, -1, -1, -1]))
    cases.insert(7, ("NaN times (early)", (np.full(1, np.nan), np.full((1, 3, 10), np.nan)), IDENTITY, [-1, -1, -1, -1]))
    return ([c[0] for c in cases], [c[1][0] for c in cases], [c[1][1] for c in cases],
            np.array([c[2] for c in cases], np.float64), np.array([c[3] for c in cases], np.int64))


def short_tracks(n):
    """n two-waypoint tracks of 3 rows at DT: thrust_min_at(1, 3) and (2, 3) alternately."""
    a, b = thrust_min_at(1, 3), thrust_min_at(2, 3)
    return [a[0] if k % 2 == 0 else b[0] for k in range(n)], [a[1] if k % 2 == 0 else b[1] for k in range(n)]


# ---- fitted tracks -----------------------------------------------------------------------------
FIT_LONG = K_SEG_LDS + 4  # segments of the added set: beyond the walk's LDS stage of segment times
FIT_DTS = (0.01, 0.1)
FIT_REF_DT = 0.1  # the dt of the comparison with the restatement (Python loops over the rows)
V_MAX, A_MAX = 1.0, 2.0
GRAVITY = 9.81


@functools.lru_cache(maxsize=None)
def fit_waypoints():
    """trajsweep_inputs.fit_waypoints(): 64 waypoint sets of 1..12 segments, all within the
    walk's LDS stage of segment times (kTcSegLds), and one set beyond it."""
    import trajsweep_inputs as tsi
    return tuple(tsi.fit_waypoints()) + (synth.random_track_waypoints(1300, FIT_LONG),)
