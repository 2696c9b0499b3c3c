"""The tracks of the time-allocation tests (CPU and GPU share them): waypoints, start times,
start velocity / acceleration.  The shapes are the smallest at which the code can take another
path: M = 1 (no gradient), 2 (M - 1 = 1), 3, 4, 12, 40 and 41 (both sides of the LDS limit of
the segment scratch), non-zero v0 / a0, a segment near t_min (the gradient's clamp acts)."""
from collections import namedtuple

import numpy as np

Track = namedtuple("Track", "name wp T v0 a0")

H, T_MIN = 0.1, 0.1


def _track(name, seed, M, v0=None, a0=None, times=None):
    rs = np.random.RandomState(seed)
    wp = np.cumsum(rs.uniform(-2.0, 2.0, (M + 1, 3)) + np.array([1.5, 0.0, 0.0]), axis=0)
    dist = np.linalg.norm(np.diff(wp, axis=0), axis=1)
    T = (0.6 + dist / 1.5) * rs.uniform(0.7, 1.4, M)  # a plausible but unbalanced allocation
    if times is not None:
        T = np.asarray(times, float)
    return Track(name, wp, T, v0, a0)


def tracks():
    return {t.name: t for t in (
        _track("m1", 1, 1),
        _track("m2", 2, 2),
        _track("m3", 3, 3),
        _track("m4", 4, 4),
        _track("m12", 12, 12),
        _track("m40", 40, 40),
        _track("m41", 41, 41),
        _track("va", 5, 3, v0=(0.8, -0.3, 0.2), a0=(0.1, 0.4, -0.2)),
        # 0.11 - h / 2 = 0.06 < t_min: the variants that shorten segment 0 are clamped
        _track("clamp", 6, 3, times=(T_MIN + 0.01, 1.5, 2.0)),
    )}


# groups of tracks that go to the device as one batch
def batches():
    t = tracks()
    many = [_track(f"b{k}", 100 + k, 2 + k % 3) for k in range(65)]
    return {
        "one": [t["m3"]],
        "two": [t["m2"], t["va"]],
        "ragged_lds": [t["m1"], t["m2"], t["m3"], t["m4"], t["m12"], t["m40"], t["clamp"]],
        "ragged_long": [t["m3"], t["m41"], t["m1"], t["m12"]],
        "many": many,
    }


def v0a0(group):
    """(n, 3) arrays for the C call: None when no track of the group has any."""
    if all(t.v0 is None and t.a0 is None for t in group):
        return None, None
    v = np.array([t.v0 if t.v0 is not None else (0, 0, 0) for t in group], float)
    a = np.array([t.a0 if t.a0 is not None else (0, 0, 0) for t in group], float)
    return v, a


# (track, step0) of the one-step comparisons (max_iter = 1): the CPU test asserts that none of
# their decisions is a coin-flip, the GPU test compares the device's step with the restated one
def one_step_cases():
    t = tracks()
    return [(t[n], s) for n, s in (("m2", 0.5), ("m2", 1.0), ("m3", 0.5), ("m4", 0.5), ("m12", 0.5), ("m40", 0.5),
                                   ("m41", 0.5), ("va", 0.5), ("clamp", 0.5), ("clamp", 1.0))]
