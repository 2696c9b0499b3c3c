"""GPU: peak speed / acceleration search (epp_traj_peaks) and time scaling to v_max / a_max
(epp_traj_scale_to_limits, epp_generate_trajectory_limited_host) against the numpy truth of
tests/pyref_feasibility.py (the reference's formulation: roots of the convolved polynomial,
external/poly_traj/src/segment.cpp:83-185, src/trajectory.cpp:191-227, :344-429).

Tolerances: peaks within 1e-9 relative of the truth (the kernel's algorithm restated in
numpy measured 7.1e-14 at worst against it on 300 tracks, so 1e-9 leaves four orders for the
device's Horner ordering); the magnitude re-evaluated at the reported time within 1e-12
relative of the reported peak (the time itself is ill-conditioned at a flat top and is not
compared with the truth's).
"""
import functools

import numpy as np
import pytest

import oracle as O
import pyref_feasibility as F
from eppamd import capi, synth

pytestmark = pytest.mark.gpu

PEAK_TOL = 1e-9
EVAL_TOL = 1e-12


def _magnitude_at(T, C, t, k, want):
    """|p^(k)| of the track at track time t (oracle Horner).  A time on a segment boundary
    belongs to both neighbours (the end of one, the start of the next), which agree only to
    the fit's continuity, so both are evaluated and the one nearer `want` is returned."""
    start, best = 0.0, None
    eps = 8 * np.spacing(max(t, 1.0))
    for i in range(len(T)):
        if start - eps <= t <= start + T[i] + eps:
            tl = min(max(t - start, 0.0), T[i])
            m = float(np.sqrt(sum(O.poly_eval(C[i][d], tl, k) ** 2 for d in range(3))))
            if best is None or abs(m - want) < abs(best - want):
                best = m
        start += T[i]
    assert best is not None, (t, float(np.sum(T)))
    return best


def _check_against_truth(Ts, Cs, pk, st, skip=()):
    worst = 0.0
    for k in range(len(Ts)):
        if k in skip:
            continue
        assert st[k] == 0, k
        truth = F.traj_peaks(Ts[k], Cs[k])
        for j, deriv in ((0, 1), (2, 2)):
            print(f"track {k} d{deriv}: gpu {pk[k, j]!r} truth {truth[j]!r} t {pk[k, j + 1]!r}")
            assert abs(pk[k, j] - truth[j]) <= PEAK_TOL * truth[j], (k, deriv, pk[k, j], truth[j])
            worst = max(worst, abs(pk[k, j] - truth[j]) / truth[j])
            assert 0.0 <= pk[k, j + 1] <= np.sum(Ts[k]) * (1 + 1e-15)
            m = _magnitude_at(Ts[k], Cs[k], pk[k, j + 1], deriv, pk[k, j])
            assert abs(m - pk[k, j]) <= EVAL_TOL * pk[k, j], (k, deriv, m, pk[k, j])
    print("worst relative peak error", worst)


def _fit(tracks, seed):
    """Fits with v0 / a0 non-zero in every second track."""
    rs = np.random.RandomState(seed)
    v0 = rs.uniform(-0.5, 0.5, (len(tracks), 3))
    a0 = rs.uniform(-0.5, 0.5, (len(tracks), 3))
    v0[::2] = 0.0
    a0[::2] = 0.0
    Ts, Cs, st = capi.minsnap_batch(tracks, 1.0, 2.0, v0, a0)
    assert (st == 0).all()
    return Ts, Cs


# ---- 1. peaks vs truth ------------------------------------------------------------------
@pytest.mark.parametrize("n_seg", [1, 2, 5, 12, 41])
def test_peaks_vs_truth(n_seg):
    """41 segments: past the fit's 40-segment LDS kernel; 5, 12, 41: more segments than waves."""
    tracks = [synth.random_track_waypoints(20000 + 31 * n_seg + k, n_seg) for k in range(16)]
    Ts, Cs = _fit(tracks, n_seg)
    pk, st = capi.traj_peaks(Ts, Cs)
    _check_against_truth(Ts, Cs, pk, st)


def test_peaks_ragged_batch():
    """1..30 segments in one launch: fewer and more segments than the workgroup has waves."""
    tracks = [synth.random_track_waypoints(900 + k, 1 + (k * 7) % 30) for k in range(40)]
    Ts, Cs = _fit(tracks, 77)
    pk, st = capi.traj_peaks(Ts, Cs)
    _check_against_truth(Ts, Cs, pk, st)


# ---- 2. hand-made segments --------------------------------------------------------------
def _seg(x=(), y=(), z=()):
    c = np.zeros((1, 3, 10))
    for d, v in enumerate((x, y, z)):
        c[0, d, :len(v)] = v
    return c


CUBIC = _seg(x=(0.0, 0.0, 1.0, -1.0 / 3.0))  # x = t^2 - t^3 / 3: v = 1 - (t - 1)^2, a = 2 - 2 t


def test_hand_made_segments():
    slow = _seg(x=(0.0, 0.1))
    Ts = [
        [2.5],                       # 0 constant velocity: g = 0 everywhere, no bracket
        [2.0],                       # 1 the cubic: the root of g_1 on the grid point T/2
        [2.0, 2.0],                  # 2 two identical segments: the tie goes to the first
        [1.0, 0.5],                  # 3 peak at t = 0 (lane 0's left end)
        [0.5, 0.5, 0.5, 0.5, 1.5],   # 4 peak at the very end of the last segment (lane 63's right end)
    ]
    Cs = [
        _seg(x=(1.0, 0.3), y=(0.0, -0.4), z=(2.0, 1.2)),
        CUBIC,
        np.concatenate([CUBIC, CUBIC]),
        np.concatenate([_seg(x=(0.0, 5.0, -1.0)), slow]),       # v = 5 - 2 t, a = -2
        np.concatenate([slow, slow, slow, slow, _seg(x=(0.0, 0.0, 1.0))]),  # last: v = 2 t, a = 2
    ]
    pk, st = capi.traj_peaks(Ts, Cs)
    print(repr(pk))
    assert (st == 0).all()
    assert pk[0, 0] == pytest.approx(1.3, rel=1e-15) and pk[0, 1] == 0.0
    assert pk[0, 2] == 0.0 and pk[0, 3] == 0.0
    assert pk[1, 0] == pytest.approx(1.0, rel=1e-15) and pk[1, 1] == pytest.approx(1.0, abs=1e-12)
    assert pk[1, 2] == 2.0 and pk[1, 3] == 0.0            # |a| = 2 at both ends: the earlier
    assert pk[2, 0] == pk[1, 0] and pk[2, 1] == pk[1, 1]  # not 3.0, the second segment's
    assert pk[2, 2] == 2.0 and pk[2, 3] == 0.0
    assert pk[3, 0] == 5.0 and pk[3, 1] == 0.0
    assert pk[3, 2] == 2.0 and pk[3, 3] == 0.0
    assert pk[4, 0] == 3.0 and pk[4, 1] == 3.5
    assert pk[4, 2] == 2.0 and pk[4, 3] == 2.0            # a = 2 on all of the last segment: its start
    for k in range(5):
        np.testing.assert_allclose(pk[k, [0, 2]], F.traj_peaks(Ts[k], Cs[k])[[0, 2]], rtol=PEAK_TOL, atol=0)


def test_rest_to_rest_fit_peaks_at_half_time():
    wp = np.array([[0.0, 0.0, 1.0], [3.0, -2.0, 1.5]])
    Ts, Cs, st = capi.minsnap_batch([wp], 1.0, 2.0)
    pk, pst = capi.traj_peaks(Ts, Cs)
    assert st[0] == 0 and pst[0] == 0
    assert pk[0, 1] == pytest.approx(Ts[0][0] / 2, rel=1e-6)
    assert pk[0, 0] == pytest.approx(315.0 / 128.0 * np.linalg.norm(wp[1] - wp[0]) / Ts[0][0], rel=1e-8)
    np.testing.assert_allclose(pk[0, [0, 2]], F.traj_peaks(Ts[0], Cs[0])[[0, 2]], rtol=PEAK_TOL, atol=0)


# ---- 3. failed tracks -------------------------------------------------------------------
def test_failed_tracks_are_flagged_and_left_untouched():
    tracks = [synth.random_track_waypoints(900 + k, 1 + (k * 7) % 30) for k in range(40)]
    tracks.insert(5, np.zeros((1, 3)))                         # fewer than 2 waypoints: no segment
    tracks.insert(9, np.array([[0, 0, 1.0], [0, 0, 1.0]]))     # zero-length segment: T = 0
    Ts, Cs, st = capi.minsnap_batch(tracks, 1.0, 2.0)
    assert st[5] == -1 and st[9] == -2
    pk, pst = capi.traj_peaks(Ts, Cs)
    for k in range(len(tracks)):
        if k in (5, 9):
            assert pst[k] == -1 and np.isnan(pk[k]).all(), k
    _check_against_truth(Ts, Cs, pk, pst, skip=(5, 9))
    Tn, Cn, sc, sst = capi.scale_to_limits(Ts, Cs, 1.0, 2.0)
    for k in (5, 9):
        assert sst[k] == -1 and sc[k] == 1.0
        assert Tn[k].tobytes() == Ts[k].tobytes() and Cn[k].tobytes() == Cs[k].tobytes()
    ok = [k for k in range(len(tracks)) if k not in (5, 9)]
    assert (sst[ok] == 0).all()
    pk2, _ = capi.traj_peaks([Tn[k] for k in ok], [Cn[k] for k in ok])
    assert (pk2[:, 0] <= 1.0 * (1 + 1e-3)).all() and (pk2[:, 2] <= 2.0 * (1 + 1e-3)).all()


# ---- 4. scaling -------------------------------------------------------------------------
# Seeds 20000..20063, 12 segments, fitted at (1.0, 2.0).  On the truth: at limits (1.0, 2.0)
# 15 tracks are within range, the velocity branch decides 49, the acceleration branch 0; at
# (3.0, 0.6) 25 are within range, velocity 0, acceleration (sqrt) 39.  One round each.
_SCALE_FIT = {}


def _scale_fit():
    if not _SCALE_FIT:
        tracks = [synth.random_track_waypoints(20000 + k, 12) for k in range(64)]
        Ts, Cs, st = capi.minsnap_batch(tracks, 1.0, 2.0)
        assert (st == 0).all()
        _SCALE_FIT["fit"] = (Ts, Cs)
    return _SCALE_FIT["fit"]


def _check_scaling(Ts, Cs, v_max, a_max, truth=None):
    """epp_traj_scale_to_limits on one batch against the truth's loop (F.scale_to_limits per
    track; truth: precomputed results by track index).  Returns how many tracks were within
    range, decided by the velocity branch, and by the acceleration (sqrt) branch."""
    Tn, Cn, sc, st = capi.scale_to_limits(Ts, Cs, v_max, a_max)
    assert (st == 0).all()
    pk, pst = capi.traj_peaks(Tn, Cn)
    assert (pst == 0).all()
    rs = np.random.RandomState(3)
    n_in = n_v = n_a = 0
    for k in range(len(Ts)):
        before = F.traj_peaks(Ts[k], Cs[k])
        vv, av = before[0] / v_max, before[2] / a_max
        _, _, s_truth, within, rounds = (truth[k] if truth and k in truth
                                         else F.scale_to_limits(Ts[k], Cs[k], v_max, a_max))
        assert within and rounds <= 2
        print(f"track {k}: gpu scale {sc[k]!r} truth {s_truth!r} peaks after {pk[k, 0]!r} {pk[k, 2]!r}")
        assert abs(sc[k] - s_truth) <= 1e-9 * s_truth, (k, sc[k], s_truth)
        assert pk[k, 0] <= v_max * (1 + 1e-3) and pk[k, 2] <= a_max * (1 + 1e-3), (k, pk[k])
        np.testing.assert_allclose(Tn[k], Ts[k] * sc[k], rtol=1e-12, atol=0)
        if vv <= 1 + 1e-3 and av <= 1 + 1e-3:
            n_in += 1
            assert sc[k] == 1.0 and np.array_equal(Tn[k], Ts[k]) and np.array_equal(Cn[k], Cs[k]), k
            assert Tn[k].tobytes() == Ts[k].tobytes() and Cn[k].tobytes() == Cs[k].tobytes(), k
        else:
            n_v += vv >= np.sqrt(av)
            n_a += vv < np.sqrt(av)
            assert sc[k] > 1.0
        for tau in rs.uniform(0, Ts[k].sum(), 20):  # the same path, s times slower
            d = np.abs(F.position(Tn[k], Cn[k], sc[k] * tau) - F.position(Ts[k], Cs[k], tau)).max()
            assert d < 1e-9, (k, tau, d)
    print("within range", n_in, "velocity branch", n_v, "acceleration branch", n_a)
    return n_in, n_v, n_a


@pytest.mark.parametrize("v_max,a_max", [(1.0, 2.0), (3.0, 0.6)])
def test_scale_to_limits(v_max, a_max):
    Ts, Cs = _scale_fit()
    assert len(Ts) == 64
    n_in, n_v, n_a = _check_scaling(Ts, Cs, v_max, a_max)
    assert n_in > 0 and (n_v > 0 if (v_max, a_max) == (1.0, 2.0) else n_a > 0)


# ---- 5. argument errors -----------------------------------------------------------------
@pytest.mark.parametrize("v_max,a_max", [(0.0, 2.0), (1.0, -1.0)])
def test_scale_argument_errors(v_max, a_max):
    T, Cf = [np.array([2.0])], [CUBIC]
    with pytest.raises(capi.EppError) as e:
        capi.scale_to_limits(T, Cf, v_max, a_max)
    assert e.value.code == capi.EPP_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.EppError) as e:
        capi.generate_trajectory_limited(np.array([[0, 0, 1.0], [1, 0, 1.0]]), v_max, a_max, 0.1)
    assert e.value.code == capi.EPP_ERR_INVALID_ARGUMENT


# ---- 6. end to end ----------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_generate_trajectory_limited(seed):
    import polynomial_trajectory as PT

    wp = synth.random_track_waypoints(500 + seed, 3 + 2 * seed)
    t0 = 3.25
    rows, scale = capi.generate_trajectory_limited(wp, 1.0, 2.0, 0.1, t0, return_scale=True)
    Ts, Cs, st = capi.minsnap_batch([wp], 1.0, 2.0)
    Tn, Cn, sc, sst = capi.scale_to_limits(Ts, Cs, 1.0, 2.0)
    assert st[0] == 0 and sst[0] == 0 and scale == sc[0]
    exp = O.sample_traj(Tn[0], Cn[0], 0.1, t0)
    assert rows.shape == exp.shape
    assert np.array_equal(rows[:, 9], exp[:, 9])            # time column exact
    assert np.abs(rows[:, :9] - exp[:, :9]).max() < 1e-6
    speed = np.linalg.norm(rows[:, [1, 4, 7]], axis=1)
    assert speed.max() <= 1.0 * (1 + 1e-3), speed.max()
    # the binding: today's rows without the flag, the limited rows with it
    plain = PT.generate_trajectory(wp, 1.0, 2.0, 0.1)
    assert np.array_equal(plain, capi.generate_trajectory(wp, 1.0, 2.0, 0.1))
    limited = PT.generate_trajectory(wp, 1.0, 2.0, 0.1, t0, enforceLimits=True)
    assert np.array_equal(limited, rows)
    pk, _ = capi.traj_peaks(Ts, Cs)
    v_peak, a_peak = PT.max_velocity_and_acceleration(wp, 1.0, 2.0)
    assert v_peak == pk[0, 0] and a_peak == pk[0, 2]


# ---- 7. long tracks ---------------------------------------------------------------------
# An "ompl"-simplified track has about 330 waypoints.  The limit kernels' loops make a second
# trip only on such tracks: the in-place coefficient rewrite (256 threads over M * 3
# polynomials) from M = 86, the time rewrite and track_invalid's loop over T from M = 257,
# track_invalid's loop over the coefficients from M = 9.  The tracks: the first M segments of
# eight 41-segment fits laid end to end (the peaks are per segment, a joint between two fits is
# one more segment boundary, where _magnitude_at accepts either neighbour).
LONG_M = (85, 86, 256, 257, 328)
LIMIT_PAIRS = ((1.0, 2.0), (3.0, 0.6))


@functools.lru_cache(maxsize=None)
def _long_tracks():
    tracks = [synth.random_track_waypoints(20000 + 31 * 41 + k, 41) for k in range(8)]
    Ts, Cs = _fit(tracks, 41)
    T, Cf = np.concatenate(Ts), np.concatenate(Cs)
    assert len(T) == 328
    return [T[:M].copy() for M in LONG_M], [Cf[:M].copy() for M in LONG_M]


@functools.lru_cache(maxsize=None)
def _ragged_fit():
    tracks = [synth.random_track_waypoints(900 + k, 1 + (k * 7) % 30) for k in range(40)]
    return _fit(tracks, 77)


@functools.lru_cache(maxsize=None)
def _long_scale_truth(v_max, a_max):
    """F.scale_to_limits of every long track and the branch that decides its first round
    ("in": within range, "v", "a"); CPU only."""
    Ts, Cs = _long_tracks()
    out = []
    for T, Cf in zip(Ts, Cs):
        pk = F.traj_peaks(T, Cf)
        vv, av = pk[0] / v_max, pk[2] / a_max
        branch = "in" if vv <= 1 + 1e-3 and av <= 1 + 1e-3 else "v" if vv >= np.sqrt(av) else "a"
        out.append((F.scale_to_limits(T, Cf, v_max, a_max), branch))
    return out


def test_peaks_long_tracks():
    Ts, Cs = _long_tracks()
    assert [len(T) for T in Ts] == list(LONG_M)
    pk, st = capi.traj_peaks(Ts, Cs)
    _check_against_truth(Ts, Cs, pk, st)
    # the peak of a longer prefix is never lower, and each track's is found in a batch of its own
    assert (np.diff(pk[:, 0]) >= 0).all() and (np.diff(pk[:, 2]) >= 0).all()
    for k in range(len(Ts)):
        alone, ast = capi.traj_peaks(Ts[k:k + 1], Cs[k:k + 1])
        assert ast[0] == 0 and alone[0].tobytes() == pk[k].tobytes(), k


def test_long_tracks_take_both_scaling_branches_on_the_truth():
    """(the inputs are what they are meant to be: on the CPU truth alone)"""
    branches = []
    for v_max, a_max in LIMIT_PAIRS:
        for (_, _, _, within, rounds), branch in _long_scale_truth(v_max, a_max):
            assert within and rounds <= 2
            branches.append(branch)
    print("branches", branches)
    assert "v" in branches and "a" in branches


@pytest.mark.parametrize("v_max,a_max", LIMIT_PAIRS)
def test_scale_long_tracks_beside_the_ragged_set(v_max, a_max):
    """One launch: the 1..30-segment ragged set and the long tracks, test_scale_to_limits'
    assertions on every track."""
    rT, rC = _ragged_fit()
    lT, lC = _long_tracks()
    Ts, Cs = list(rT) + list(lT), list(rC) + list(lC)
    truth = {len(rT) + i: t for i, (t, _) in enumerate(_long_scale_truth(v_max, a_max))}
    n_in, n_v, n_a = _check_scaling(Ts, Cs, v_max, a_max, truth)
    long_branches = [b for _, b in _long_scale_truth(v_max, a_max)]
    assert ("v" if (v_max, a_max) == (1.0, 2.0) else "a") in long_branches
    assert n_v + n_a >= len(lT) - long_branches.count("in")


def test_invalid_long_tracks_are_flagged_and_left_untouched():
    """A NaN coefficient, a zero and an infinite segment time, each past element 255 of a
    300-segment track: found by the second trips of track_invalid's loops."""
    lT, lC = _long_tracks()
    rT, rC = _ragged_fit()
    T300, C300 = lT[-1][:300], lC[-1][:300]
    bad = []
    Cn = C300.copy()
    Cn.reshape(-1)[3 * 10 * 260 + 7] = np.nan
    bad.append((T300.copy(), Cn))
    for i, v in ((270, 0.0), (299, np.inf)):
        Tb = T300.copy()
        Tb[i] = v
        bad.append((Tb, C300.copy()))
    good = [(lT[0], lC[0]), (rT[17], rC[17]), (T300, C300), (lT[3], lC[3])]
    order = [good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3]]
    Ts, Cs = [t for t, _ in order], [c for _, c in order]
    bad_at, good_at = (1, 3, 5), (0, 2, 4, 6)
    pk, st = capi.traj_peaks(Ts, Cs)
    Tn, Cn, sc, sst = capi.scale_to_limits(Ts, Cs, 1.0, 2.0)
    for k in bad_at:
        assert st[k] == -1 and np.isnan(pk[k]).all(), k
        assert sst[k] == -1 and sc[k] == 1.0, k
        assert Tn[k].tobytes() == Ts[k].tobytes() and Cn[k].tobytes() == Cs[k].tobytes(), k
    # the valid neighbours: as in a launch of their own
    gT, gC = [Ts[k] for k in good_at], [Cs[k] for k in good_at]
    pk_g, st_g = capi.traj_peaks(gT, gC)
    Tg, Cg, sc_g, sst_g = capi.scale_to_limits(gT, gC, 1.0, 2.0)
    assert (st_g == 0).all() and (sst_g == 0).all() and (sc_g > 1.0).any()
    for i, k in enumerate(good_at):
        assert st[k] == 0 and sst[k] == 0 and pk[k].tobytes() == pk_g[i].tobytes(), k
        assert sc[k] == sc_g[i] and Tn[k].tobytes() == Tg[i].tobytes() and Cn[k].tobytes() == Cg[i].tobytes(), k
    _check_against_truth(gT, gC, pk_g, st_g)


@pytest.mark.parametrize("n", [5, 9])
def test_tie_within_a_wave_goes_to_the_earlier_segment(n):
    """Segments s and s + 4 are searched by the same wave (4 waves stride over the segments):
    n identical cubics tie in both peaks, within a wave and across waves; the peak times are the
    first segment's, as test_hand_made_segments' case 2 asserts across waves."""
    pk_single = capi.traj_peaks([[2.0]], [CUBIC])[0][0]
    pk, st = capi.traj_peaks([[2.0] * n, [2.0]], [np.concatenate([CUBIC] * n), CUBIC])
    print(repr(pk))
    assert (st == 0).all()
    assert (pk[:, 0] == pk_single[0]).all() and (pk[:, 2] == pk_single[2]).all()
    assert (pk[:, 1] == pk_single[1]).all() and (pk[:, 3] == 0.0).all()
