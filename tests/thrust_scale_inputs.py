"""Inputs of the thrust-limit scaling tests (test_gpu_thrust_scale.py, test_thrust_scale_cpu.py)
and of the CPU test of those inputs (test_thrust_scale_inputs_cpu.py): hand-built coefficient
tracks whose answers are exact doubles, grouped by the limits they run under (a call has one
set of limits), and fitted tracks.

G = 9.75 and every segment time a power of two, so a / s^2 at s = 1.5 (s2 = 2.25 exactly) and
the squares and roots behind the answers are exact: F = (13, 0, 9.75) has |F| = 16.25.

Everything is input data: built once per process, shared, read-only.
"""
import collections
import functools

import numpy as np

from eppamd import synth
from thrust_scale_ref import F_MAX, F_MIN, RATE, TILT, Limits

G = 9.75
A = 29.25          # a_x with A / 2.25 = 13
INF = float("inf")

L_FMAX = Limits(G, 0.0, 16.25, INF, -1.0)
L_TILT = Limits(G, 0.0, INF, INF, G / 16.25)
L_RATE = Limits(G, 0.0, INF, 1.0, -1.0)
L_FMIN = Limits(G, 5.75, INF, INF, -1.0)
L_FMIN_LOW = Limits(G, 3.25, INF, INF, -1.0)
L_FALL = Limits(G, 5.75, INF, 1.0, 0.5)

# what a case claims: scale (None: not an exact double, see the case), status, violated bits,
# t_fmax (None: not claimed): thrust_grid's time of the greatest thrust at scale 1
Want = collections.namedtuple("Want", "scale status violated t_fmax", defaults=(None,))
Group = collections.namedtuple("Group", "name limits names Ts Cs wants")


def segments(n, T=1.0):
    """n hovering segments (all coefficients zero) of time T."""
    return np.full(n, T), np.zeros((n, 3, 10))


def one(coeffs, T=1.0):
    """One segment; coeffs: {(axis, power): value}."""
    Ts, C = segments(1, T)
    for (d, p), v in coeffs.items():
        C[0, d, p] = v
    return Ts, C


def peak_at(tau, a_peak=A):
    """x'' = a_peak - 12 (t - tau)^2 on T = 1: c2 = (a_peak - 12 tau^2) / 2, c3 = 4 tau, c4 = -1,
    exact for a dyadic tau; the greatest a_x, a_peak, is attained at tau alone."""
    return {(0, 2): (a_peak - 12.0 * tau * tau) / 2.0, (0, 3): 4.0 * tau, (0, 4): -1.0}


def peak_track(n_seg, pos, tau):
    """n_seg segments of hover (T = 1) with peak_at(tau) as segment pos."""
    Ts, C = segments(n_seg)
    for (d, p), v in peak_at(tau).items():
        C[pos, d, p] = v
    return Ts, C


PEAK_POINTS = (("point 0", 0.0), ("point 1", 1.0 / 64), ("point 31", 31.0 / 64), ("point 63", 63.0 / 64),
               ("tau = T", 1.0))
# (segments, the peak's segment): first, segment 4 (a wave's second stride), last of 5, 17, 44
PEAK_PLACES = ((5, 0), (5, 4), (17, 0), (17, 4), (17, 16), (44, 0), (44, 4), (44, 43))


@functools.lru_cache(maxsize=None)
def hand_groups():
    nan_track = (np.full(2, np.nan), np.zeros((2, 3, 10)))
    one_wp = (np.zeros(0), np.zeros((0, 3, 10)))
    fmax = [
        # x = 1/2 * 29.25 t^2: at 1.5, F = (13, 0, 9.75), |F| = 16.25 = f_max
        ("f_max", one({(0, 2): A / 2.0}), Want(1.5, 0, F_MAX, 0.0)),
        ("one waypoint", one_wp, Want(1.0, -1, 0)),
        ("feasible at 1", one({(0, 2): 2.0, (1, 3): 0.25, (2, 2): -1.0}, 2.0), Want(1.0, 0, 0)),
        ("NaN time", nan_track, Want(1.0, -1, 0)),
        # a_x = 1e9: 1e9 / 1024^2 is still some 950 m/s^2
        ("needs more than 1024", one({(0, 2): 0.5e9}), Want(1.0, 1, F_MAX, 0.0)),
        ("hover", segments(3, 0.5), Want(1.0, 0, 0, 0.0)),
        # x'' = A - 48 (t - 1)^2: the point before tau = T is 48 / 4096 lower, enough for the
        # search's 2^-12 to tell a dropped tau = T point
        ("sharp peak on tau = T", one({(0, 2): (A - 48.0) / 2.0, (0, 3): 16.0, (0, 4): -4.0}), Want(1.5, 0, F_MAX, 1.0)),
    ]
    for n_seg, pos in PEAK_PLACES:
        for what, tau in PEAK_POINTS:
            fmax.append((f"peak on {what} of segment {pos} of {n_seg}", peak_track(n_seg, pos, tau),
                         Want(1.5, 0, F_MAX, pos + tau)))
    groups = [
        ("f_max", L_FMAX, fmax),
        ("tilt", L_TILT, [("tilt", one({(0, 2): A / 2.0}), Want(1.5, 0, TILT)),
                          ("hover", segments(2), Want(1.0, 0, 0))]),
        # x = 32.90625 t^3 / 6: c3 = 5.484375 exactly, j_x = 32.90625 = 9.75 * 1.5^3; the rate is
        # greatest at t = 0, where it is j_x / (g s^3)
        ("rate", L_RATE, [("rate", one({(0, 3): 32.90625 / 6.0}), Want(1.5, 0, RATE)),
                          ("one waypoint", one_wp, Want(1.0, -1, 0))]),
        ("f_min", L_FMIN, [
            # z = -1/2 * 9 t^2: F_z = 9.75 - 9 / s^2 = 5.75 at 1.5
            ("f_min", one({(2, 2): -4.5}), Want(1.5, 0, F_MIN)),
            # z = -1/2 * 29.25 t^2: the thrust points down and is 19.5 at 1 (3.25 at 1.5): feasible
            # at 1, infeasible at larger scales -- the documented non-monotone case
            ("thrust axis down", one({(2, 2): -A / 2.0}), Want(1.0, 0, 0)),
        ]),
        # a_z = -6.5 * 1.34375^2: a / s2 = 6.5 exactly and F_z = 3.25 = f_min, while a * (1 / s2)
        # rounds above 6.5 and F_z below 3.25 (where a reciprocal in place of the division shows)
        ("f_min at 1.34375", L_FMIN_LOW, [("f_min at 1.34375", one({(2, 2): -11.73681640625 / 2.0}),
                                           Want(1.34375, 0, F_MIN))]),
        # a_z = -g: F = 0 at scale 1 -- thrust 0 < f_min, rate and cos_tilt NaN (they violate
        # nothing although their limits are on); F_z = g (1 - 1 / s^2) >= 5.75 from s = 1.5612..
        ("free fall", L_FALL, [("free fall", one({(2, 2): -G / 2.0}), Want(None, 0, F_MIN))]),
    ]
    return tuple(Group(name, L, tuple(c[0] for c in cases), tuple(c[1][0] for c in cases),
                       tuple(c[1][1] for c in cases), tuple(c[2] for c in cases)) for name, L, cases in groups)


FREE_FALL_SCALE = (1.5612, 1.5613)  # sqrt(1 / (1 - 5.75 / 9.75)) = 1.56125, to the search's 2^-12

# ---- fitted tracks -----------------------------------------------------------------------------
V_MAX, A_MAX = 8.0, 12.0
GRAVITY = 9.81
# limits under which most of the v_max 8 / a_max 12 fits need 1 < s < 4
L_FIT = Limits(GRAVITY, 9.0, 10.5, 0.5, 0.96)
FIT_LONG = 44
FIT_DT = 0.01


@functools.lru_cache(maxsize=None)
def fit_waypoints():
    """65 waypoint sets of 3..12 segments, then one of 44."""
    sets = [synth.random_track_waypoints(2100 + k, 3 + k % 10) for k in range(65)]
    return tuple(sets) + (synth.random_track_waypoints(2300, FIT_LONG),)


@functools.lru_cache(maxsize=None)
def short_waypoints():
    """41 sets of three waypoints (two segments); the GPU test tiles their fits to 1025 tracks."""
    return tuple(synth.random_track_waypoints(2400 + k, 2) for k in range(41))


N_SHORT = 1025
