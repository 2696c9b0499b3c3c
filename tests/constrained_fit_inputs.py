"""TEST INFRASTRUCTURE ONLY -- the inputs of the constrained min-snap fit's tests
(test_gpu_minsnap_constrained.py) and their conversion to the two layouts: the library's
(mask uint8[W], values float64[W, 4, 3]; epp_minsnap_batch_constrained) and the oracle's
(fixed_mask[v * 5 + k], fixed_val[(v * 5 + k) * 3 + d]; oracle.minsnap_solve).

Waypoints come from synth.random_track_waypoints, segment times are Nfabian times at
v_max = 1, a_max = 2, as in the existing fit tests.  Random pins stay on derivatives 1 and 2
(velocity, acceleration): random jerk and snap at inner waypoints make the problem so
ill-conditioned that the two CPU restatements differ by more than the device's tolerance.
Pins of derivatives 3 and 4 take their values from a free fit's own derivatives.  Every case
here is measured against the refined truth by test_constrained_fit_inputs_cpu.py.
"""
import functools
from math import factorial

import numpy as np

import oracle as O
from eppamd import synth

V_MAX, A_MAX = 1.0, 2.0
N_TRACKS = 16
SEGMENTS = (1, 2, 3, 4, 5, 12, 40, 41)  # 40 / 41: LDS against global segment scratch (kMaxLdsSeg)
RAGGED_SEGMENTS = (1, 2, 3, 5, 8, 30, 11, 14, 17, 4, 20, 23, 26, 7, 29, 13)
SHAPE_SEGMENTS = 9                       # the elimination-shape cases: 8 inner vertices, meeting at 4


class Case:
    """One track: waypoints, segment times, mask uint8[W], values float64[W, 4, 3] (NaN in every
    slot that is not used), and what it is."""

    def __init__(self, wp, mask, values, what, times=None):
        self.wp = np.asarray(wp, np.float64)
        self.T = O.segment_times(self.wp, V_MAX, A_MAX) if times is None else np.asarray(times, np.float64)
        self.mask = np.asarray(mask, np.uint8)
        self.values = np.asarray(values, np.float64)
        self.what = what
        W = len(self.wp)
        assert self.mask.shape == (W,) and self.values.shape == (W, 4, 3) and self.T.shape == (W - 1,)

    def used(self):
        """bool[W, 4]: the slots the fit reads (all four at the two ends)."""
        u = ((self.mask[:, None] >> np.arange(4)[None, :]) & 1).astype(bool)
        u[0] = u[-1] = True
        return u

    def fixed_dict(self):
        """constrained_fit_ref / minsnap_np layout: {(v, k): value}."""
        fixed, u = {}, self.used()
        for v in range(len(self.wp)):
            fixed[(v, 0)] = self.wp[v]
            for k in range(1, 5):
                if u[v, k - 1]:
                    fixed[(v, k)] = self.values[v, k - 1]
        return fixed

    def oracle_tables(self):
        """oracle.minsnap_solve layout."""
        W = len(self.wp)
        m = np.zeros((W, 5), np.uint8)
        val = np.zeros((W, 5, 3))
        m[:, 0] = 1
        val[:, 0] = self.wp
        u = self.used()
        m[:, 1:] = u
        val[:, 1:][u] = self.values[u]
        return m, val

    def oracle_coeffs(self):
        m, val = self.oracle_tables()
        return O.minsnap_solve(m, val, self.T, 3, 4)


def _blank(W):
    return np.zeros(W, np.uint8), np.full((W, 4, 3), np.nan)


def _ends(values, rs, kind):
    """The two end states.  kind 2: end velocity and acceleration and start jerk and snap
    non-zero; else generateTrajectory's {v0, a0, 0, 0} and rest."""
    values[0] = values[-1] = 0.0
    values[0, 0] = rs.uniform(-0.5, 0.5, 3)
    values[0, 1] = rs.uniform(-0.5, 0.5, 3)
    if kind == 2:
        values[0, 2] = rs.uniform(-0.5, 0.5, 3)
        values[0, 3] = rs.uniform(-0.5, 0.5, 3)
        values[-1, 0] = rs.uniform(-0.5, 0.5, 3)
        values[-1, 1] = rs.uniform(-0.5, 0.5, 3)


def make_track(seed, n_seg, kind):
    """kind 0: random subsets of {velocity, acceleration} at random inner waypoints; 1:
    velocity at every inner waypoint; 2: free inside, full end states."""
    wp = synth.random_track_waypoints(seed, n_seg)
    rs = np.random.RandomState(seed + 7919)
    mask, values = _blank(len(wp))
    _ends(values, rs, kind)
    for w in range(1, n_seg):
        bits = rs.randint(0, 4) if kind == 0 else 1 if kind == 1 else 0
        mask[w] = bits
        for k in (1, 2):
            if bits >> (k - 1) & 1:
                values[w, k - 1] = rs.uniform(-0.5, 0.5, 3)
    return Case(wp, mask, values, f"{n_seg} segments, seed {seed}, kind {kind}")


@functools.lru_cache(maxsize=None)
def batch(n_seg):
    """16 tracks of n_seg segments, the three kinds in turn."""
    return tuple(make_track(4000 + 31 * n_seg + k, n_seg, k % 3) for k in range(N_TRACKS))


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """16 tracks of 1..30 segments with caller times near Nfabian's."""
    out = []
    for k, n_seg in enumerate(RAGGED_SEGMENTS):
        c = make_track(5000 + k, n_seg, k % 3)
        rs = np.random.RandomState(6000 + k)
        out.append(Case(c.wp, c.mask, c.values, c.what + ", caller times", c.T * rs.uniform(0.9, 1.3, n_seg)))
    return tuple(out)


def vertex_derivatives(coeffs, T):
    """float64[W, 5, 3]: derivatives 0..4 of a fit at its vertices (vertex v from the start of
    segment v; the last from the end of the last segment)."""
    M = len(T)
    out = np.zeros((M + 1, 5, 3))
    for v in range(M):
        for k in range(5):
            out[v, k] = factorial(k) * coeffs[v, :, k]
    for k in range(5):
        out[M, k] = [O.poly_eval(coeffs[M - 1, d], T[M - 1], k) for d in range(3)]
    return out


@functools.lru_cache(maxsize=None)
def shape_batch():
    """9 segments (8 inner vertices, the two eliminations meet at m = 4): one pin, velocity or
    acceleration, at inner vertex 1, at the last, at m and at both its neighbours; and all
    four derivatives pinned at m to the free fit's own values there."""
    n_seg = SHAPE_SEGMENTS
    nin = n_seg - 1
    m = (nin + 1) // 2
    out = []
    for j, v in enumerate((1, nin, m - 1, m, m + 1)):
        for k in (1, 2):
            seed = 7000 + 2 * j + k
            wp = synth.random_track_waypoints(seed, n_seg)
            rs = np.random.RandomState(seed)
            mask, values = _blank(len(wp))
            _ends(values, rs, 0)
            mask[v] = 1 << (k - 1)
            values[v, k - 1] = rs.uniform(-0.5, 0.5, 3)
            out.append(Case(wp, mask, values, f"derivative {k} pinned at vertex {v} of {n_seg} segments"))
    wp = synth.random_track_waypoints(7100, n_seg)
    mask, values = _blank(len(wp))
    _ends(values, np.random.RandomState(7100), 0)
    free = Case(wp, mask, values, "free")
    dv = vertex_derivatives(free.oracle_coeffs(), free.T)
    mask, values = mask.copy(), values.copy()
    mask[m] = 0xF
    values[m] = dv[m, 1:]
    out.append(Case(wp, mask, values, f"all four derivatives pinned at vertex {m}"))
    return tuple(out)


def all_cases():
    """Every case a GPU test compares with the oracle."""
    for n_seg in SEGMENTS:
        yield from batch(n_seg)
    yield from ragged_batch()
    yield from shape_batch()
