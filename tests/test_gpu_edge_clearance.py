"""GPU: swept clearance (include/epp.h): epp_motions_clearance, the Euclidean distance between
each straight edge and the nearest collision OBB, and epp_traj_chord_clearance_batch, the
closest approach of the chords between the rows of fitted tracks straight from their
coefficients; and the Python / PathPlanner layers.

Against the numpy restatement (edge_clearance_ref.py: the same IEEE operations in the same
association, one correctly rounded square root after the minimum) dist and t must be the same
bytes and nearest the same integers.  By definition the fused call is epp_sample_count +
epp_sample_batch + epp_motions_clearance on consecutive rows (columns 0 / 3 / 6) + a per-track
minimum that prefers the earliest chord, with time = t_j + t * (t_j+1 - t_j) on the sampled
time column: all five outputs are compared with that composition with ==.

Worlds, edge sets and tracks: edge_clearance_inputs.py.  T = kClearTile, the LDS tile of both
kernels.
"""
import functools

import numpy as np
import pytest

import clearance_ref as cr
import edge_clearance_inputs as ei
import edge_clearance_ref as er
import small_path_inputs as spi
import trajsweep_inputs as tsi
from eppamd import capi
from test_edge_clearance_cpu import BOUND, argument_errors, scale
from test_gpu_trajsweep import _sample

pytestmark = pytest.mark.gpu

FIT_DT = 0.1


@functools.lru_cache(maxsize=None)
def _world(name):
    _, rg, ro = spi.setup()
    return capi.World(ei.obbs(name), rg, ro)


@functools.lru_cache(maxsize=None)
def _fit():
    Ts, Cs, st = capi.minsnap_batch(tsi.fit_waypoints(), 1.0, 2.0)
    assert (st == 0).all()
    return Ts, Cs


def _same_bytes(got, exp, what):
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64)) if len(got) == len(exp) else None
    assert got.tobytes() == exp.tobytes(), (what, bad[:8], got[bad[:8]], exp[bad[:8]])


# ---- 1. edges against the restatement -----------------------------------------------------------
@pytest.mark.parametrize("name", ei.WORLDS)
def test_edges_equal_restatement(name):
    world = _world(name)
    assert world.n == {"0": 0, "filling": 3, "1": 1, "T-1": ei.T - 1, "T": ei.T, "T+1": ei.T + 1}[name]
    d2, t, near = ei.expected(name, ei.BLOCK + 1)  # (a shorter set is a prefix of this one)
    for n in ei.EDGE_COUNTS:
        s1, s2 = ei.edges(name, n)
        dist, got_t, got_near = world.edge_clearances(s1, s2)
        assert (dist.dtype, got_t.dtype, got_near.dtype) == (np.float64, np.float64, np.int32)
        assert len(dist) == len(got_t) == len(got_near) == n
        print(f"{name} OBBs, {n} edges: differing dist {int((dist != er.dist(d2[:n])).sum())},"
              f" t {int((got_t != t[:n]).sum())}, nearest {int((got_near != near[:n]).sum())}")
        assert np.array_equal(got_near, near[:n]), n
        _same_bytes(got_t, t[:n], (name, n, "t"))
        _same_bytes(dist, er.dist(d2[:n]), (name, n, "dist"))
    if name in ("0", "filling"):
        assert np.isinf(dist).all() and (got_t == -1.0).all() and (got_near == -1).all()


def test_edges_t_and_nearest_are_optional():
    world = _world("T+1")
    s1, s2 = ei.edges("T+1", 65)
    full = world.edge_clearances(s1, s2)
    d1, d2 = capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
    d_dist = capi.DeviceBuffer(8 * len(s1))
    capi.check(capi.lib().epp_motions_clearance(world.handle, d1.ptr, d2.ptr, len(s1), d_dist.ptr, None, None, None))
    capi.sync()
    _same_bytes(d_dist.download(np.float64, len(s1)), full[0], "dist alone")


# ---- 2. the existing queries ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1", "T+1", "filling"])
def test_zero_length_edges_and_endpoints(name):
    """A zero-length edge is its point, and no edge is farther than its nearer end: both bit
    for bit, because the endpoints go through clearance's own d2."""
    world = _world(name)
    s1, s2 = ei.edges(name, ei.BLOCK + 1)
    dist, t, near = world.edge_clearances(s1, s2)
    ends = []
    for p in (s1, s2):
        pd, pn = world.clearance(p)
        zd, zt, zn = world.edge_clearances(p, p)
        _same_bytes(zd, pd, (name, "zero length"))
        assert np.array_equal(zn, pn) and (zt[zn >= 0] == 0.0).all() and (zt[zn < 0] == -1.0).all()
        ends.append(pd)
    fin = er.finite_edges(s1, s2)
    lim = np.minimum(*ends)
    assert (dist[fin] <= lim[fin]).all() and (dist[fin] * dist[fin] <= (lim * lim)[fin]).all()
    assert (dist[fin] < lim[fin]).sum() >= (32 if name != "filling" else 0)


def test_blocked_edges_are_close():
    """An edge first_hits(can_pass_gate=True) reports blocked has a point in a collision OBB
    grown by its owner's radius r per axis (collision_common.h: rec_ray_parts tests the half
    sizes h_k + r), so every excess e_k <= r there: d2 <= 3 r^2, up to the measured error of
    d2 (BOUND * max(1, L^2)), which the square root turns into at most that over 2 sqrt(3) r;
    4 spacings for the roundings of sqrt(3) r and the root."""
    import firsthit_inputs as fi
    _, rg, ro = spi.setup()
    r = max(rg, ro)
    world = _world("72")
    s1, s2 = fi.edges("72", fi.BLOCK + 1)
    t_hit, obb = world.first_hits(s1, s2, True)
    dist, t, near = world.edge_clearances(s1, s2)
    blocked = obb >= 0
    assert blocked.sum() >= 32 and (~blocked).sum() >= 32
    lim = np.sqrt(3.0) * r
    tol = BOUND * scale(ei.obbs("72"), s1, s2, near) / (2.0 * lim) + 4 * np.spacing(lim)
    print(f"blocked {int(blocked.sum())}: max dist {dist[blocked].max():.6f}, sqrt(3) r = {lim:.6f}")
    assert (dist[blocked] <= lim + tol[blocked]).all()


# ---- 3. the fused call against the composition and the restatement -----------------------------
def _compose(world, Ts, Cs, dt):
    """The definition: consecutive sampled rows -> World.edge_clearances (one call over every
    track's chords) -> per track the earliest chord of the minimum distance and its time."""
    rows, roff = _sample(Ts, Cs, dt)
    nt = len(Ts)
    out = (np.full(nt, np.inf), np.full(nt, -1, np.int64), np.full(nt, -1.0), np.full(nt, -1.0),
           np.full(nt, -1, np.int32))
    a = np.concatenate([np.arange(roff[k], max(roff[k], roff[k + 1] - 1)) for k in range(nt)] + [np.zeros(0, np.int64)])
    a = a.astype(np.int64)
    if len(a) == 0:
        return out, np.diff(roff)
    xyz = np.ascontiguousarray(rows[:, [0, 3, 6]])
    dist, t, near = world.edge_clearances(xyz[a], xyz[a + 1])
    coff = np.zeros(nt + 1, np.int64)
    coff[1:] = np.cumsum(np.maximum(np.diff(roff) - 1, 0))
    for k in range(nt):
        c = slice(coff[k], coff[k + 1])
        res = er.chords_min(dist[c], t[c], near[c], rows[roff[k]:roff[k + 1], 9])
        for o, v in zip(out, res):
            o[k] = v
    return out, np.diff(roff)


def _assert_equals_composition(world, Ts, Cs, dt):
    exp, cnt = _compose(world, Ts, Cs, dt)
    got = world.trajectory_chord_clearances(Ts, Cs, dt)
    assert [g.dtype for g in got] == [np.float64, np.int64, np.float64, np.float64, np.int32]
    for g, e, what in zip(got, exp, ("clearance", "chord", "t", "time", "nearest")):
        assert np.array_equal(g, e), (what, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    clr, chord, t, time, near = got
    none = chord == -1
    assert np.array_equal(none, np.isinf(clr)) and (chord < np.maximum(cnt - 1, 0))[~none].all()
    assert (t[none] == -1.0).all() and (time[none] == -1.0).all() and (near[none] == -1).all()
    assert ((t[~none] >= 0) & (t[~none] <= 1)).all() and (near[~none] >= 0).all()
    assert none[cnt < 2].all()
    return got, cnt


def test_track_edges():
    """edge_clearance_inputs' straight tracks beside the pole: the closest chord at each edge of
    the walk's bookkeeping, tracks without a chord, 1 / 2 / kTcSegLds / kTcSegLds + 1 segments,
    a failed fit's NaN times.  One launch, then some in launches of their own; and against the
    restatement on the restatement's own rows."""
    names, Ts, Cs, want = ei.edge_tracks()
    world = _world("1")
    (clr, chord, t, time, near), cnt = _assert_equals_composition(world, Ts, Cs, ei.DT)
    print("edges:", list(zip(names, chord.tolist(), clr.tolist(), t.tolist())))
    assert chord.tolist() == want
    assert cnt[names.index("1 row")] == 1 and cnt[names.index("2 rows")] == 2
    assert cnt[names.index("513 rows, last chord")] == ei.K_ROW_CHUNK + 1
    assert chord[names.index(f"chunk boundary {ei.K_ROW_CHUNK - 1}|{ei.K_ROW_CHUNK}")] == ei.K_ROW_CHUNK - 1
    for k, name in enumerate(names):
        if want[k] < 0:
            assert (clr[k], chord[k], t[k], time[k], near[k]) == (np.inf, -1, -1.0, -1.0, -1), name
        elif name != "across the pole":
            assert abs(clr[k] - ei.SIDE) < 1e-9 and near[k] == 0 and 0.3 < t[k] < 0.45, name
    exp = er.tracks(ei.obbs("1"), [cr.sample_rows(T, Cf, ei.DT) for T, Cf in zip(Ts, Cs)])
    for g, e, what in zip((clr, chord, t, time, near), exp, ("clearance", "chord", "t", "time", "nearest")):
        assert np.array_equal(g, e), (what, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    for k in range(0, len(Ts), 3):
        alone = world.trajectory_chord_clearances(Ts[k:k + 1], Cs[k:k + 1], ei.DT)
        assert all(a[0] == g[k] for a, g in zip(alone, (clr, chord, t, time, near))), names[k]


@pytest.mark.parametrize("name", ["72", "T+1", "filling", "0"])
def test_fitted_tracks_equal_composition(name):
    world = _world(name)
    Ts, Cs = _fit()
    assert len(Ts) == 64 and {len(t) for t in Ts} == set(range(1, 13))
    got, cnt = _assert_equals_composition(world, Ts, Cs, FIT_DT)
    print(f"{name}: chords {got[1].tolist()}")
    if name in ("72", "T+1"):
        _, cnt = _assert_equals_composition(world, Ts, Cs, 0.01)
        assert cnt.max() > 2 * ei.K_ROW_CHUNK and cnt.min() < ei.K_ROW_CHUNK  # several chunks, and less than one
        assert np.isfinite(got[0]).all()
    else:
        assert np.isinf(got[0]).all() and (got[1] == -1).all()


def test_chords_with_a_non_finite_end_are_ignored():
    """Three segments along the pole's side, the middle one's coefficients NaN: its rows are
    NaN, the chords that touch them never count, the others do."""
    T, Cf = ei._beside(2, 0, 3, 5.5 * ei.DT)
    Cf = Cf.copy()
    Cf[1] = np.nan
    world = _world("1")
    (clr, chord, t, time, near), cnt = _assert_equals_composition(world, [T], [Cf], ei.DT)
    assert cnt[0] >= 17 and chord[0] == 2 and abs(clr[0] - ei.SIDE) < 1e-9
    Cf[0] = np.nan  # (now chord 2 has a NaN end: the closest is a chord of the last segment)
    (clr, chord, t, time, near), _ = _assert_equals_composition(world, [T], [Cf], ei.DT)
    assert chord[0] >= 11 and np.isfinite(clr[0])


def test_more_tracks_than_workgroups():
    """2560 tracks: the persistent grid has at most 8 workgroups per CU, so every workgroup
    takes several tracks and keeps no state from one to the next."""
    world = _world("72")
    Ts, Cs = _fit()
    assert 2560 > 8 * capi.cu_count()
    got = world.trajectory_chord_clearances(Ts * 40, Cs * 40, FIT_DT)
    first = world.trajectory_chord_clearances(Ts, Cs, FIT_DT)
    for r in range(40):
        assert all(np.array_equal(g[64 * r:64 * (r + 1)], f) for g, f in zip(got, first))


def test_optional_outputs_may_be_null():
    world = _world("72")
    Ts, Cs = _fit()
    nt = len(Ts)
    full = world.trajectory_chord_clearances(Ts, Cs, FIT_DT)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_clr = capi.DeviceBuffer(8 * nt)
    capi.check(capi.lib().epp_traj_chord_clearance_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, FIT_DT,
                                                         d_clr.ptr, None, None, None, None, None))
    capi.sync()
    assert np.array_equal(d_clr.download(np.float64, nt), full[0])


# ---- 4. rows against chords ----------------------------------------------------------------------
def test_chords_are_never_farther_than_rows():
    for name in ("72", "T+1"):
        world = _world(name)
        Ts, Cs = _fit()
        rows = world.trajectory_clearance(Ts, Cs, FIT_DT)[0]
        chords = world.trajectory_chord_clearances(Ts, Cs, FIT_DT)[0]
        two = capi.sample_count(Ts, FIT_DT) >= 2
        assert two.sum() >= 60 and (chords[two] <= rows[two]).all()
        print(f"{name}: chords closer than rows on {int((chords[two] < rows[two]).sum())} of {int(two.sum())} tracks,"
              f" by up to {np.max((rows - chords)[two]):.4f} m")


def test_a_bar_between_two_rows():
    """The track across the pole: rows 10 and 11 lie 0.4 m before and behind its centre plane,
    chord 10 goes through it.  The rows keep their 0.35 m; the chords have none."""
    T, Cf = ei.bar_track()
    xyz, time = cr.sample_rows(T, Cf, ei.DT)  # the claim, on the restatement
    d2_rows = cr.states(ei.obbs("1"), xyz)[0]
    d2_chords = er.edges(ei.obbs("1"), xyz[:-1], xyz[1:])[0]
    assert np.sqrt(d2_rows.min()) > 0.3 and np.sqrt(d2_chords.min()) < 1e-6 and int(np.argmin(d2_chords)) == 10
    world = _world("1")
    rows = world.trajectory_clearance([T], [Cf], ei.DT)
    chords = world.trajectory_chord_clearances([T], [Cf], ei.DT)
    print(f"rows {rows[0][0]:.6f} at row {rows[1][0]}, chords {chords[0][0]:.3e} at chord {chords[1][0]} t {chords[2][0]:.4f}")
    assert rows[0][0] - chords[0][0] > 0.05 and chords[1][0] == 10 and rows[1][0] in (10, 11)


# ---- 5. C++ / pybind ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planner():
    import online_traj_planner as otp
    gates, obstacles = spi.poses(72)
    return otp.PathPlanner(np.array(gates), np.array(obstacles), spi.FILLING_CONFIG)


def test_path_planner_edge_and_path_clearance():
    pp = _planner()
    world = _world("72")
    for n in (1, 257, 20000):  # one edge, zero-copy, staged through HBM
        s1, s2 = ei.edges("72", n)
        got = pp.edge_clearances(s1, s2)
        exp = world.edge_clearances(s1, s2)
        assert (got[0].dtype, got[1].dtype, got[2].dtype) == (np.float64, np.float64, np.int32)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    for path in tsi.fit_waypoints()[:12]:
        path = np.asarray(path, float)
        if len(path) < 2:
            continue
        dist, t, near = world.edge_clearances(path[:-1], path[1:])
        j = int(np.argmin(dist))
        got = pp.path_clearance(path)
        assert got == (dist[j], j, t[j], near[j])
        assert isinstance(got[0], float) and isinstance(got[1], int) and isinstance(got[3], int)
    with pytest.raises(ValueError, match="at least two points"):
        pp.path_clearance(np.zeros((1, 3)))


def test_path_planner_candidate_swept_clearances():
    pp = _planner()
    sets = tsi.fit_waypoints()[:8]
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    exp = _world("72").trajectory_chord_clearances(Ts, Cs, FIT_DT)
    got = pp.candidate_swept_clearances(sets, 1.0, 2.0, FIT_DT)
    assert [g.dtype for g in got] == [np.float64, np.int64, np.float64, np.float64, np.int32]
    assert all(np.array_equal(g, e) for g, e in zip(got, exp))
    assert np.isfinite(got[0]).all()
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_swept_clearances([sets[0], sets[1][:1]], 1.0, 2.0, FIT_DT)
    assert [len(r) for r in pp.candidate_swept_clearances([], 1.0, 2.0, FIT_DT)] == [0, 0, 0, 0, 0]


# ---- 6. argument errors --------------------------------------------------------------------------
def test_argument_errors():
    argument_errors(capi.lib())
    world = _world("1")
    L = capi.lib()
    p = capi.DeviceBuffer(64)
    assert L.epp_motions_clearance(world.handle, p.ptr, p.ptr, -1, p.ptr, None, None, None) == -1
    assert L.epp_motions_clearance(world.handle, None, None, 0, None, None, None, None) == capi.EPP_OK
    assert L.epp_traj_chord_clearance_batch(world.handle, p.ptr, p.ptr, p.ptr, 1, 0.0, p.ptr, None, None, None, None,
                                            None) == -1
