"""Inputs of the row sampler's tests (test_sample_batch_cpu.py, test_gpu_sample_batch.py).

Every set is a pair of lists (segment times, coefficients M x 3 x 10) per track.  The fitted
tracks come from a fit the caller names -- the CPU oracle's (fit_oracle: the CPU tests, which
check the inputs and the bound without the code under test) or the device's
(capi.minsnap_batch / minsnap_batch_times: the GPU tests); the hand-made ones are the same
either way.  No set has T_total / dt above 2e4 (the recurrence acc + dt stalls for tiny dt).
"""
import numpy as np

import oracle as O
from eppamd import synth

DT = 0.1
EDGE_DT = 0.25  # the recurrence-edge batch: its "T a multiple of dt" case is stated at 0.25
K_ROW_CHUNK = 512  # csrc/traj_sample.h kRowChunk (test_sample_batch_cpu.py holds it to the header)

FIT_SEGS = (1, 2, 5, 12, 13, 24, 30, 41)
EXTENT = 0.5  # small tracks: the whole ragged batch stays near 6,000 rows at DT


def fit_problem():
    """(waypoint arrays, v0, a0): tracks of FIT_SEGS segments, v0 / a0 non-zero on every
    second track."""
    tracks = [synth.random_track_waypoints(5200 + k, n, EXTENT) for k, n in enumerate(FIT_SEGS)]
    rs = np.random.RandomState(52)
    v0 = rs.uniform(-0.5, 0.5, (len(tracks), 3))
    a0 = rs.uniform(-0.5, 0.5, (len(tracks), 3))
    v0[::2] = 0.0
    a0[::2] = 0.0
    return tracks, v0, a0


def fit_oracle():
    """The fit_problem tracks fitted by the CPU oracle at (v_max, a_max) = (1.0, 2.0)."""
    tracks, v0, a0 = fit_problem()
    fits = [O.minsnap_track(wp, 1.0, 2.0, v0[k], a0[k]) for k, wp in enumerate(tracks)]
    return [f[0] for f in fits], [f[1] for f in fits]


def _concat(Ts, Cs, which):
    return np.concatenate([Ts[i] for i in which]), np.concatenate([Cs[i] for i in which])


def ragged(Ts, Cs):
    """The fitted tracks, then a 130- and a 131-segment track made by concatenating fitted
    tracks' (T, C) (41 + 41 + 41 + 5 + 2 [+ 1] segments; the sampler needs no continuity):
    the 64-lane staging loop of the segment times makes three trips, M even and odd."""
    assert [len(t) for t in Ts] == list(FIT_SEGS)
    Ts, Cs = list(Ts), list(Cs)
    for which in ((7, 7, 7, 2, 1), (7, 7, 7, 2, 1, 0)):
        T, Cf = _concat(Ts, Cs, which)
        Ts.append(T)
        Cs.append(Cf)
    assert [len(t) for t in Ts[-2:]] == [130, 131]
    return Ts, Cs


# per-track start offsets of the ragged batch (10 tracks): signed zeros, exact binary
# fractions, large and tiny magnitudes, one so large that the sum rounds to an integer
T0S = np.array([0.0, -0.0, 3.25, -7.5, 1e6, 2.0 ** -40, 0.1, -1e-3, 1234.5678, 2.0 ** 52])

NAN_FILL = 0x7FF8DEADBEEF0001  # a quiet NaN with a payload no arithmetic produces


def _live_coeffs(rs, M, T_scale):
    """M x 3 x 10 coefficients, every one non-zero, c_j ~ +-(0.5..1.5) / T_scale^j so that every
    term matters at the end of the segment."""
    mag = rs.uniform(0.5, 1.5, (M, 3, 10)) * rs.choice([-1.0, 1.0], (M, 3, 10))
    return mag / np.maximum(T_scale, 1.0) ** np.arange(10)


CHUNK_ROWS = (1, 8, 9, K_ROW_CHUNK - 1, K_ROW_CHUNK, K_ROW_CHUNK + 1, 2 * K_ROW_CHUNK + 1)


def chunk_edges():
    """One-segment tracks of exactly CHUNK_ROWS rows at DT (T = (n - 0.5) dt), all ten
    coefficients non-zero on all three axes."""
    rs = np.random.RandomState(512)
    Ts = [np.array([(n - 0.5) * DT]) for n in CHUNK_ROWS]
    Cs = [_live_coeffs(rs, 1, float(T[0])) for T in Ts]
    return Ts, Cs


# the recurrence-edge batch at EDGE_DT: (name, segment times, expected row count or None)
EDGE_CASES = (
    ("dt greater than the whole track", [0.1, 0.1], 1),
    ("T exact multiples of dt", [0.5, 0.25, 1.0], None),
    ("zero-length segment in the middle", [0.6, 0.0, 0.7], None),
    ("three consecutive segments shorter than dt", [0.7, 0.1, 0.05, 0.2, 0.9], None),
    ("one waypoint", [], 0),
    ("T all zero", [0.0, 0.0, 0.0], 0),
    ("T all NaN", [np.nan, np.nan], 0),
)


def recurrence_edges(Ts, Cs):
    """(names, Ts, Cs): the EDGE_CASES tracks (live coefficients) with fitted tracks (5 and 12
    segments) between them; the name of an ordinary track is None."""
    rs = np.random.RandomState(25)
    names, oT, oC = [], [], []
    for i, (name, T, _) in enumerate(EDGE_CASES):
        T = np.array(T, np.float64)
        names.append(name)
        oT.append(T)
        oC.append(_live_coeffs(rs, len(T), 1.0))
        k = 2 + i % 2
        names.append(None)
        oT.append(Ts[k])
        oC.append(Cs[k])
    return names, oT, oC


SINGLE_SEGS = (3, 12, 40)
SINGLE_T0 = 3.25


def single_problem():
    """Per SINGLE_SEGS: (waypoints, segment times by the host's Nfabian, v0, a0)."""
    rs = np.random.RandomState(40)
    out = []
    for k, n in enumerate(SINGLE_SEGS):
        wp = synth.random_track_waypoints(6400 + k, n, 2.0)
        v0, a0 = rs.uniform(-0.3, 0.3, 3), rs.uniform(-0.3, 0.3, 3)
        out.append((wp, O.segment_times(wp, 1.0, 2.0), v0, a0))
    return out


def single_oracle():
    """The single_problem tracks fitted by the CPU oracle (its times are the same Nfabian)."""
    fits = [O.minsnap_track(wp, 1.0, 2.0, v0, a0) for wp, _, v0, a0 in single_problem()]
    return [f[0] for f in fits], [f[1] for f in fits]


def all_sets_cpu():
    """Every input set of the GPU tests with the oracle's fits: (name, dt, Ts, Cs)."""
    fT, fC = fit_oracle()
    _, eT, eC = recurrence_edges(fT, fC)
    return (("ragged", DT) + ragged(fT, fC), ("chunk edges", DT) + chunk_edges(),
            ("recurrence edges", EDGE_DT, eT, eC), ("single track", DT) + single_oracle())
