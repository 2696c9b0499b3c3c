"""GPU: the collision kernels on worlds far from the origin, bit-exact against the oracle.

Every spatial index the kernels use (the cull grid, the class grid, the motion tiles) is built
in float over double data, and each is argued to be an exact superset of the reference's rtree
query.  Near the origin (float)p resolves 1e-6 m and the arguments are never under load.  Here
the same capped C2 track stands at the origin (the control), about 1 km and about 100 km away
(far_world_inputs.py), with states, edges and hover tracks on and just under the union's top
faces: the sliver whose fine coordinate exceeds 4 n (1 + 2^-20), where the cull grid once cut
(test_far_world_inputs_cpu.py proves that the inputs reach it).

Every kernel choice runs: k_states_v5 (and its 1024-thread shape), k_states_v4, the generic
k_states and the brute-force small path; the tile kernel k_motions_v5, the cell-list kernels,
the generic k_motions and the small path; k_traj_check and k_traj_sweep; and a world updated
from near to far and back.  On a mismatch the first ten indices are printed, and whether they
are ladder entries.
"""
import functools

import numpy as np
import pytest

from eppamd import capi, synth

import far_world_inputs as I

pytestmark = pytest.mark.gpu

STATE_IMPLS = ("v5", "v5b1024", "v4", "generic")
MOTION_IMPLS = ("tile", "v4", "generic")


@functools.lru_cache(maxsize=None)
def _world(name):
    """The device world of a name; shared and left unchanged."""
    _, rg, ro = I.setup()
    return capi.World(I.world(name)[0], rg, ro)


def _env(monkeypatch, states=None, block=None, motions=None):
    for key, val in (("EPP_STATES_KERNEL", states), ("EPP_V5_BLOCK", block), ("EPP_MOTIONS_KERNEL", motions)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)


def _states_env(monkeypatch, impl):
    _env(monkeypatch, states=impl[:2] if impl.startswith("v") else impl, block=impl[3:] if impl.startswith("v5b") else None)


class _Diffs:
    """Collects got != exp per call; check() fails with every call that differed: the number of
    mismatches, how many of them are ladder entries, and the first ten."""

    def __init__(self):
        self.msgs = []

    def same(self, got, exp, what, ladder):
        got, exp = np.asarray(got), np.asarray(exp)
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        bad = np.flatnonzero(got != exp)
        if len(bad):
            lines = [f"    [{i}] got {got[i]} expected {exp[i]} ladder {bool(ladder[i])}" for i in bad[:10]]
            self.msgs.append(f"{what}: {len(bad)} of {len(exp)} differ, {int(ladder[bad].sum())} of them ladder "
                             "entries\n" + "\n".join(lines))

    def check(self):
        if self.msgs:
            msg = "\n".join(self.msgs)
            print(msg)
            pytest.fail(msg)


# ---- states ----------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", STATE_IMPLS)
@pytest.mark.parametrize("name", I.WORLDS)
def test_states(name, impl, monkeypatch):
    _states_env(monkeypatch, impl)
    d = _Diffs()
    w = _world(name)
    pts, kind, _ = I.states(name)
    lad = kind == 2
    for cp in (0, 1):
        d.same(w.check_states(pts, bool(cp)), I.exp_states(name, cp), f"{name} {impl} check_states can_pass {cp}", lad)
    exp = I.exp_states(name, 0)
    valid, idx = w.check_states(pts, False, compact=True)
    d.same(valid, exp, f"{name} {impl} check_states compact flags", lad)
    if not np.array_equal(np.sort(idx), np.flatnonzero(exp)):
        d.msgs.append(f"{name} {impl} compact indices: {len(idx)} given, {int(exp.sum())} expected")
    for md in I.MIN_DISTANCES:
        d.same(w.check_states_mindist(pts, md), I.exp_states(name, md), f"{name} {impl} mindist {md}", lad)
    d.check()


@pytest.mark.parametrize("name", I.WORLDS)
def test_states_small_path(name, monkeypatch):
    _env(monkeypatch)
    d = _Diffs()
    w = _world(name)
    pts, kind, _ = I.states(name)
    n = 257
    lad = kind[:n] == 2
    for cp in (0, 1):
        d.same(w.check_states(pts[:n], bool(cp)), I.exp_states(name, cp)[:n], f"{name} small check_states {cp}", lad)
    for md in I.MIN_DISTANCES:
        d.same(w.check_states_mindist(pts[:n], md), I.exp_states(name, md)[:n], f"{name} small mindist {md}", lad)
    d.check()


# ---- motions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", MOTION_IMPLS)
@pytest.mark.parametrize("name", I.WORLDS)
def test_motions(name, impl, monkeypatch):
    _env(monkeypatch, motions=None if impl == "tile" else impl)
    d = _Diffs()
    w = _world(name)
    s, e, kind = I.edges(name)
    lad = (kind == 1) | (kind == 2)
    for mode in (0, 1):
        for cp in (0, 1):
            d.same(w.check_motions(s, e, bool(cp), mode), I.exp_motions(name, mode, cp),
                   f"{name} {impl} check_motions mode {mode} can_pass {cp}", lad)
    d.check()


@pytest.mark.parametrize("name", I.WORLDS)
def test_motions_small_path(name, monkeypatch):
    _env(monkeypatch)
    d = _Diffs()
    w = _world(name)
    s, e, kind = I.edges(name)
    n = 513
    lad = ((kind == 1) | (kind == 2))[:n]
    for mode in (0, 1):
        for cp in (0, 1):
            d.same(w.check_motions(s[:n], e[:n], bool(cp), mode), I.exp_motions(name, mode, cp)[:n],
                   f"{name} small check_motions mode {mode} can_pass {cp}", lad)
    d.check()


# ---- trajectories ----------------------------------------------------------------------------
def _hover_check(d, w, name):
    """k_traj_check on the hover tracks: every row of a track is its point, so the first invalid
    row is 0 (time 0.0) where the oracle's minDistance flag of the point is 0, else none."""
    Ts, Cs = I.hover_tracks(name)
    _, lad = I.hover_points(name)
    for md in I.MIN_DISTANCES:
        first, time = w.check_trajectories(Ts, Cs, I.DT, md)
        flag = I.exp_hover_mindist(name, md)
        d.same(first, np.where(flag == 0, 0, -1), f"{name} check_trajectories md {md} first row", lad)
        d.same(time, np.where(flag == 0, 0.0, -1.0), f"{name} check_trajectories md {md} time", lad)


@pytest.mark.parametrize("name", I.WORLDS)
def test_hover_tracks_check(name, monkeypatch):
    _env(monkeypatch)
    d = _Diffs()
    assert (capi.sample_count(I.hover_tracks(name)[0][:4], I.DT) >= 2).all()
    _hover_check(d, _world(name), name)
    d.check()


@pytest.mark.parametrize("name", I.WORLDS)
def test_hover_tracks_sweep(name, monkeypatch):
    """k_traj_sweep on the hover tracks: every chord is the degenerate edge point -> point, so
    the first failing chord is 0 where check_motions (mode 0) of the oracle rejects it."""
    _env(monkeypatch)
    d = _Diffs()
    w = _world(name)
    Ts, Cs = I.hover_tracks(name)
    _, lad = I.hover_points(name)
    for cp in (0, 1):
        first, time = w.sweep_trajectories(Ts, Cs, I.DT, bool(cp))
        flag = I.exp_hover_chords(name, cp)
        d.same(first, np.where(flag == 0, 0, -1), f"{name} sweep_trajectories can_pass {cp} chord", lad)
        d.same(time, np.where(flag == 0, 0.0, -1.0), f"{name} sweep_trajectories can_pass {cp} time", lad)
    d.check()


@pytest.mark.parametrize("name", I.WORLDS)
def test_fitted_tracks_equal_the_composition(name, monkeypatch):
    """Eight tracks fitted through waypoints moved with the world: k_traj_check equals
    epp_sample_batch -> epp_check_states_mindist -> first zero flag per track on the same device
    (not the oracle, whose Horner order differs)."""
    _env(monkeypatch)
    d = _Diffs()
    w = _world(name)
    dx, dy = I.OFFSETS[name]
    tracks = [synth.random_track_waypoints(600 + k, 12) + [dx, dy, 0.0] for k in range(8)]
    Ts, Cs, st = capi.minsnap_batch(tracks, 1.0, 2.0)
    assert (st == 0).all(), st
    cnt = capi.sample_count(Ts, I.DT)
    roff = np.concatenate([[0], np.cumsum(cnt)])
    rows = capi.sample_batch(Ts, Cs, I.DT)
    assert len(rows) == roff[-1] and (cnt > 10).all()
    none = np.zeros(len(Ts), bool)
    hits = 0
    for md in I.MIN_DISTANCES:
        flags = w.check_states_mindist(rows[:, [0, 3, 6]], md)
        exp_first, exp_time = np.full(len(Ts), -1, np.int64), np.full(len(Ts), -1.0)
        for k in range(len(Ts)):
            bad = np.flatnonzero(flags[roff[k]:roff[k + 1]] == 0)
            if len(bad):
                exp_first[k], exp_time[k] = bad[0], rows[roff[k] + bad[0], 9]
        first, time = w.check_trajectories(Ts, Cs, I.DT, md)
        print(f"{name} md {md}: {int(cnt.sum())} rows, first {first.tolist()}")
        d.same(first, exp_first, f"{name} fitted md {md} first row", none)
        d.same(time, exp_time, f"{name} fitted md {md} time", none)
        hits += int((exp_first >= 0).sum())
    d.check()
    assert hits > 0  # some track meets the world


# ---- world update ------------------------------------------------------------------------------
def test_update_near_far_near(monkeypatch):
    """One world updated from "near" to "100km" and back: the cull limits and float origins are
    rebuilt with the index (the generic kernel, the discrete32 cell-list kernel and k_traj_check
    read them)."""
    _, rg, ro = I.setup()
    d = _Diffs()
    w = capi.World(I.world("near")[0], rg, ro)
    try:
        for step, name in enumerate(("near", "100km", "near")):
            if step:
                w.update(I.world(name)[0])
            pts, kind, _ = I.states(name)
            s, e, ek = I.edges(name)
            lad = (ek == 1) | (ek == 2)
            for impl in ("v5", "generic"):
                _states_env(monkeypatch, impl)
                d.same(w.check_states(pts, False), I.exp_states(name, 0), f"step {step} {name} {impl} check_states",
                       kind == 2)
            for impl in ("tile", "v4"):
                _env(monkeypatch, motions=None if impl == "tile" else impl)
                d.same(w.check_motions(s, e, False, 1), I.exp_motions(name, 1, 0),
                       f"step {step} {name} {impl} check_motions mode 1", lad)
            _env(monkeypatch)
            _hover_check(d, w, name)
        d.check()
    finally:
        w.close()
