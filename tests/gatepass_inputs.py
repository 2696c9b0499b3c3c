"""Inputs of the gate-passage tests (test_gpu_gatepass.py) and of the CPU tests of those inputs
(test_gatepass_inputs_cpu.py): hand-built straight tracks, gate frame tables and edge sets,
with the outcome each one claims.

The tracks fly at V = 8 m/s sampled at DT = 0.125 s.  Both are powers of two, so the row times
j * DT and the positions, STEP = 1 m apart, are exact doubles whichever way they are summed; the
single-gate cases use yaw 0 (c = 1, s = 0), so their gate-frame values are exact too.  A track
"through" a gate plane has rows J and J + 1 half a step before and behind it: chord J crosses.

Everything is input data: built once per process, shared, read-only.
"""
import functools
import os
import re

import numpy as np

from eppamd import capi, synth

DT = 0.125
V = 8.0
STEP = V * DT
HE = capi.GATE_HALF_EDGE
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "efficient-path-planner_amd", "csrc")
K_SEG_LDS = int(re.search(r"kTcSegLds = (\d+);", open(os.path.join(_CSRC, "traj_walk.h")).read()).group(1))
ROW_CHUNK = int(re.search(r"kRowChunk = (\d+);", open(os.path.join(_CSRC, "traj_sample.h")).read()).group(1))
assert ROW_CHUNK == 512  # (the chunk-boundary tracks below are written for it)

# one gate at the origin, yaw 0: gate frame = world frame, crossed along +y
FR1 = capi.gate_frames([[0.0, 0.0, 0.0]], [0.0])


def line(p0, v, T):
    """Coefficients of p = p0 + v t over segments of times T (each continues the line)."""
    p0, v, T = np.asarray(p0, float), np.asarray(v, float), np.atleast_1d(np.asarray(T, float))
    c = np.zeros((len(T), 3, 10))
    t0 = 0.0
    for s in range(len(T)):
        c[s, :, 0] = p0 + v * t0
        c[s, :, 1] = v
        t0 += T[s]
    return T, c


def through(J, R, plane=0.0, x=0.0, z=0.0, vy=V):
    """One segment, R rows, flying along y; rows J and J + 1 half a step before / behind y = plane."""
    return line([x, plane - np.sign(vy) * (J + 0.5) * STEP, z], [0.0, vy, 0.0], [(R - 0.5) * DT])


@functools.lru_cache(maxsize=None)
def single_gate_tracks():
    """(names, Ts, Cs, want): tracks against FR1, want = the chord that passes the gate or -1.
    The first four (and all but the NaN track) have exact gate-frame values."""
    n_seg = K_SEG_LDS + 1
    cases = [
        ("chord 0", through(0, 20), 0),
        ("last chord", through(18, 20), 18),
        ("lane group edge 7|8", through(7, 20), 7),
        ("inside a lane's group 3|4", through(3, 20), 3),
        ("chunk boundary 511|512", through(511, 530), 511),
        ("first chord of the second chunk 512|513", through(512, 530), 512),
        ("chunk boundary 1023|1024", through(1023, 1040), 1023),
        # rows 0..5 in segment 0 (5.5 DT long), row 6 half a step into segment 1
        ("segment boundary 5|6", line([0.0, -5.5 * STEP, 0.0], [0.0, V, 0.0], [5.5 * DT, 10.0 * DT]), 5),
        ("1 row", through(0, 1), -1),
        ("2 rows", through(0, 2), 0),
        ("512 rows, last chord", through(510, 512), 510),
        ("513 rows, last chord", through(511, 513), 511),
        (f"{n_seg} segments", line([0.0, -20.5 * STEP, 0.0], [0.0, V, 0.0], np.full(n_seg, 5.5 * DT)), 20),
        ("wrong direction", through(3, 20, vy=-V), -1),
        ("outside in x", through(3, 20, x=0.5), -1),
        ("outside in z", through(3, 20, z=-0.5), -1),
        ("x offset == half edge", through(3, 20, x=HE), 3),
        ("z offset == -half edge", through(3, 20, z=-HE), 3),
        ("x offset just past the half edge", through(3, 20, x=np.nextafter(HE, 1.0)), -1),
        ("z offset just past the half edge", through(3, 20, z=-np.nextafter(HE, 1.0)), -1),
        # rows at y = -2, -1, 0, 1, ...: row 2 lies on the gate plane, g.y == 0 exactly
        ("a row on the gate plane", line([0.0, -2.0, 0.0], [0.0, V, 0.0], [19.5 * DT]), -1),
        ("NaN times", (np.full(2, np.nan), np.full((2, 3, 10), np.nan)), -1),
    ]
    return ([c[0] for c in cases], [c[1][0] for c in cases], [c[1][1] for c in cases],
            np.array([c[2] for c in cases], np.int64))


def two_laps():
    """Four segments of six rows each: +y at x = 0 through gate A (yaw 0 at the origin), -y at
    x = 5 through gate B (yaw pi at (5, 0, 0): it is crossed flying -y), and both once more."""
    T = np.array([5.5 * DT, 6 * DT, 6 * DT, 6 * DT])
    c = np.zeros((4, 3, 10))
    c[0, :, 0], c[0, 1, 1] = [0.0, -2.5, 0.0], V
    c[1, :, 0], c[1, 1, 1] = [5.0, 3.0, 0.0], -V
    c[2, :, 0], c[2, 1, 1] = [0.0, -3.0, 0.0], V
    c[3, :, 0], c[3, 1, 1] = [5.0, 3.0, 0.0], -V
    return T, c


A = [0.0, 0.0, 0.0]
FAR = [100.0, 0.0, 0.0]


@functools.lru_cache(maxsize=None)
def multi_gate_cases():
    """[(name, frames, Ts, Cs, want (n_tracks, G) chords)]: one launch each."""
    y0 = capi.gate_frames
    lap = two_laps()
    return [
        ("two gates passed by the same chord", y0([A, [0.0, 0.25, 0.0]], [0.0, 0.0]),
         [through(3, 20)[0]], [through(3, 20)[1]], np.array([[3, 3]])),
        ("two gates whose crossings lie in different chunks", y0([A, [0.0, 600.0, 0.0]], [0.0, 0.0]),
         [through(100, 720)[0]], [through(100, 720)[1]], np.array([[100, 700]])),
        ("gate 1's only crossing before gate 0's", y0([[0.0, 10.0, 0.0], A], [0.0, 0.0]),
         [through(3, 20)[0]], [through(3, 20)[1]], np.array([[13, -1]])),
        ("a gate listed twice on a two-lap track", y0([A, [5.0, 0.0, 0.0], A, [5.0, 0.0, 0.0]], [0.0, np.pi, 0.0, np.pi]),
         [lap[0]], [lap[1]], np.array([[2, 8, 14, 20]])),
        ("a later gate crossed while an earlier one never is", y0([FAR, A], [0.0, 0.0]),
         [through(3, 20)[0]], [through(3, 20)[1]], np.array([[-1, -1]])),
    ]


def short_tracks(n):
    """n two-row tracks, alternately passing FR1 (chord 0) and flying the wrong way (-1)."""
    ok, no = through(0, 2), through(0, 2, vy=-V)
    Ts = [ok[0] if k % 2 == 0 else no[0] for k in range(n)]
    Cs = [ok[1] if k % 2 == 0 else no[1] for k in range(n)]
    return Ts, Cs, np.where(np.arange(n) % 2 == 0, 0, -1)


# ---- edges -------------------------------------------------------------------------------------
BLOCK = 256  # gate_pass.hip: kGcBlock
EDGE_COUNTS = (1, 63, 64, 65, BLOCK + 1)
GATE_COUNTS = (1, 2, 63, 64)
LO, HI = np.array([-6.0, -6.0, 0.0]), np.array([6.0, 6.0, 2.0])


@functools.lru_cache(maxsize=None)
def random_frames(G):
    """G gates in the box with any yaw."""
    rs = np.random.RandomState(500 + G)
    return capi.gate_frames(rs.uniform(LO, HI, size=(G, 3)), rs.uniform(-np.pi, np.pi, G))


@functools.lru_cache(maxsize=None)
def random_edges(n, G):
    """n edges of which most cross the plane of gate i % G near its centre, in either direction
    and partly outside the opening, so every gate's bit is set for some edge."""
    f = random_frames(G)
    rs = np.random.RandomState(7000 + 64 * n + G)
    g = np.arange(n) % G
    c, s = f[g, 3], f[g, 4]
    # gate-frame points (x, y, z): the reference's frame is g = R(yaw) t, so t = R(-yaw) g
    ga = np.column_stack([rs.uniform(-0.6, 0.6, n), -rs.uniform(0.05, 0.4, n), rs.uniform(-0.6, 0.6, n)])
    gb = np.column_stack([rs.uniform(-0.6, 0.6, n), rs.uniform(0.05, 0.4, n), rs.uniform(-0.6, 0.6, n)])
    flip = rs.uniform(size=n) < 0.25  # the wrong direction
    first = np.arange(n) < G          # each gate's first edge crosses it, well inside
    ga[first, 0::2] *= 0.5
    gb[first, 0::2] *= 0.5
    flip[first] = False
    ga[flip], gb[flip] = gb[flip].copy(), ga[flip].copy()

    def world(p):
        return np.column_stack([c * p[:, 0] + s * p[:, 1], -s * p[:, 0] + c * p[:, 1], p[:, 2]]) + f[g, :3]
    return world(ga), world(gb)


def exact_edges():
    """(s1, s2, want): edges against FR1 with exact gate-frame values, one per outcome."""
    up = np.nextafter(HE, 1.0)
    rows = [
        ([0.0, -0.5, 0.0], [0.0, 0.5, 0.0], True),     # crossed
        ([0.0, 0.5, 0.0], [0.0, -0.5, 0.0], False),    # the wrong direction
        ([0.0, -1.5, 0.0], [0.0, -0.5, 0.0], False),   # stays before the plane
        ([0.5, -0.5, 0.0], [0.5, 0.5, 0.0], False),    # outside in x
        ([0.0, -0.5, 0.5], [0.0, 0.5, 0.5], False),    # outside in z
        ([HE, -0.5, 0.0], [HE, 0.5, 0.0], True),       # |x offset| == half edge: inside
        ([0.0, -0.5, -HE], [0.0, 0.5, -HE], True),     # |z offset| == half edge: inside
        ([up, -0.5, 0.0], [up, 0.5, 0.0], False),
        ([0.0, -0.5, -up], [0.0, 0.5, -up], False),
        ([0.0, -1.0, 0.0], [0.0, 0.0, 0.0], False),    # ends on the plane: g2.y == 0
        ([0.0, 0.0, 0.0], [0.0, 1.0, 0.0], False),     # starts on the plane: g1.y == 0
        ([np.nan, -0.5, 0.0], [0.0, 0.5, 0.0], False),  # NaN compares false
        ([1.0, -0.5, 0.0], [-1.0, 0.5, 0.0], True),    # the midpoint decides, not the ends
    ]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))


# ---- fitted tracks -----------------------------------------------------------------------------
N_FIT_GATES = 8
FIT_ON = 11  # the track (12 segments) the gates are placed on


def gates_on_rows(rows, n_gates=N_FIT_GATES):
    """A frame table of n_gates gates on one sampled track (R, 10): gate g at the midpoint of the
    chord at fraction (g + 1) / (n_gates + 1) of the rows, turned so that the chord's direction
    is the gate frame's +y (g = R(yaw) t: yaw = pi / 2 - atan2(dy, dx))."""
    xyz = rows[:, [0, 3, 6]]
    j = ((np.arange(n_gates) + 1) * (len(xyz) - 1)) // (n_gates + 1)
    d = xyz[j + 1] - xyz[j]
    return capi.gate_frames((xyz[j] + xyz[j + 1]) / 2, np.pi / 2 - np.arctan2(d[:, 1], d[:, 0])), j


def fit_waypoints():
    """trajsweep_inputs.fit_waypoints(): 64 waypoint sets of 1..12 segments round the same ring."""
    import trajsweep_inputs as tsi
    return tsi.fit_waypoints()
