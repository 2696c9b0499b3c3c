"""Inputs of the swept-check tests (test_gpu_trajsweep.py) and of the CPU test of those inputs
(test_trajsweep_cpu.py): straight-line tracks against one thin box, and the oracle's answer to
"which chord between consecutive rows fails first".

The thin box is the single obstacle pole of a 1-OBB world under configs/config_filling.json:
0.1 m wide, inflated by 0.2 m, so 0.5 m across for a ray.  The tracks fly along +x through its
centre line at V = 8 m/s sampled at DT = 0.1 s: the rows lie STEP = 0.8 m apart, and a track
whose rows j and j + 1 sit half a step before and behind the pole's centre has every row 0.4 m
from it (outside the inflated extent, valid for every point check) and exactly one chord,
j, through it.

Everything is input data and oracle output: built once per process, shared, read-only.
"""
import functools

import numpy as np

import oracle as O
import small_path_inputs as spi
from eppamd import capi, synth

DT = 0.1
V = 8.0
STEP = V * DT
Z = 0.5
CAN_PASS = (False, True)


@functools.lru_cache(maxsize=None)
def thin_poses():
    return synth.track_world(2024, n_gates=0, n_obstacles=1)


@functools.lru_cache(maxsize=None)
def thin_ref():
    """The oracle's 1-OBB world."""
    fgeom, rg, ro = spi.setup()
    ref = O.world_build(fgeom, *thin_poses(), rg, ro)
    assert len(ref) == 1
    return ref


def thin_obbs():
    return capi.build_obbs(spi.setup()[0], *thin_poses())


def linear(x0, vx, y, z, n_seg=1, T0=0.0):
    """Coefficients of x = x0 + vx t (y, z fixed); n_seg = 2: a second segment that continues
    the line after T0."""
    c = np.zeros((n_seg, 3, 10))
    for s in range(n_seg):
        c[s, 0, :2] = (x0 + vx * T0 * s, vx)
        c[s, 1, 0] = y
        c[s, 2, 0] = z
    return c


def _through(J, R):
    """One segment, R rows, rows J and J + 1 half a step before / behind the pole."""
    cx, cy = (float(v) for v in thin_ref()[0]["center"][:2])
    return np.array([(R - 0.5) * DT]), linear(cx - (J + 0.5) * STEP, V, cy, Z)


@functools.lru_cache(maxsize=None)
def edge_tracks():
    """(names, Ts, Cs, want): the only failing chord at each edge of the kernel's bookkeeping
    (kRowChunk = 512 samples per half of the double buffer, 8 consecutive samples per lane of
    a full chunk), tracks of exactly 1, 2 and 513 rows, and valid neighbours in between."""
    cx, cy = (float(v) for v in thin_ref()[0]["center"][:2])
    away = (np.array([3.0]), linear(cx - 4.0, -V, cy, Z))  # flies away from the pole: valid
    cases = [
        ("chord 0", *_through(0, 20), 0),
        ("last chord", *_through(18, 20), 18),
        ("lane group edge 7|8", *_through(7, 20), 7),
        ("inside a lane's group 3|4", *_through(3, 20), 3),
        ("chunk boundary 511|512", *_through(511, 530), 511),
        ("chunk boundary 1023|1024", *_through(1023, 1040), 1023),
        ("first chord of the second chunk 512|513", *_through(512, 530), 512),
        # rows 0..5 in segment 0 (5.5 DT long), row 6 half a step into segment 1
        ("segment boundary 5|6", np.array([5.5 * DT, 10.0 * DT]), linear(cx - 5.5 * STEP, V, cy, Z, 2, 5.5 * DT), 5),
        ("1 row", *_through(0, 1), -1),
        ("2 rows", *_through(0, 2), 0),
        ("513 rows, last chord", *_through(511, 513), 511),
        ("513 rows, valid", np.array([512.5 * DT]), linear(cx + 1.0, V, cy, Z), -1),
        ("512 rows, valid", np.array([511.5 * DT]), linear(cx + 1.0, V, cy, Z), -1),
    ]
    names, Ts, Cs, want = [], [], [], []
    for name, T, Cf, w in cases:
        names += [name, "away"]
        Ts += [T, away[0]]
        Cs += [Cf, away[1]]
        want += [w, -1]
    return names, Ts, Cs, want


def thin_track():
    """(Ts, Cs, straddling chord): rows all valid, chord 10 through the pole."""
    T, Cf = _through(10, 20)
    return [T], [Cf], 10


def oracle_sweep(ref, Ts, Cs, dt, can_pass, eps=1e-9):
    """(first failing chord, its start row's time, takes part, rows) per track from the CPU
    oracle: World::checkRayValid on consecutive rows of the oracle's sampling.  A track takes
    part when the oracle's flags do not change with the inflation radii moved by -eps and +eps
    (the oracle's Horner order differs from the device's fused one by ~1e-15 in the
    positions)."""
    _, rg, ro = spi.setup()
    nt = len(Ts)
    first = np.full(nt, -1, np.int64)
    time = np.full(nt, -1.0)
    robust = np.ones(nt, bool)
    n_rows = np.zeros(nt, np.int64)
    for k in range(nt):
        if len(Ts[k]) == 0:
            continue
        rows = O.sample_traj(Ts[k], Cs[k], dt)
        n_rows[k] = len(rows)
        if len(rows) < 2:
            continue
        xyz = rows[:, [0, 3, 6]]
        f = O.check_motions(ref, rg, ro, xyz[:-1], xyz[1:], can_pass, 0, threads=8)
        robust[k] = (np.array_equal(O.check_motions(ref, rg - eps, ro - eps, xyz[:-1], xyz[1:], can_pass, 0, threads=8), f)
                     and np.array_equal(O.check_motions(ref, rg + eps, ro + eps, xyz[:-1], xyz[1:], can_pass, 0, threads=8), f))
        bad = np.flatnonzero(f == 0)
        if len(bad):
            first[k] = bad[0]
            time[k] = rows[bad[0], 9]
    return first, time, robust, n_rows


# ---- fitted tracks ---------------------------------------------------------------------------
FIT_SEEDS = tuple(1200 + k for k in range(64))


def fit_waypoints():
    """64 waypoint sets of 1..12 segments."""
    return [synth.random_track_waypoints(s, 1 + k % 12) for k, s in enumerate(FIT_SEEDS)]
