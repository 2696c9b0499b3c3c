"""CPU: the inputs of test_gpu_fit_limits.py without the code under test.

1. The constants and formulas fit_limits_inputs.py restates are the sources' (the cited text is
   still in the cited file), and the boundary values derived from the restatement are the
   eight the tests were written for; every "largest" case asks for at most kLdsBudget bytes of
   LDS and every "first refused" case for more.
2. The row-slicing cases give exactly the row counts they are named for, by the restated
   recurrence and by the oracle's sampler.
3. The comparisons of the GPU tests bite: a fit with two components of v0 swapped, with the a0
   term dropped, or with one segment's coefficients shifted by one slot leaves the tolerance
   the GPU test uses for that quantity (the coefficient rule of the batch fit, the row bound
   with its allowance of the refit, the 1e-6 of the longest refit's rows, the 2 D S of a cost
   and 2 (2 D S) / h of a gradient entry) on every case.
4. The recorded oracle rows of the 4280-segment refit belong to this module's track, and the
   restricted reference of the gradient's bounds is time_alloc_ref.reference_distance.
"""
import functools
import re
from fractions import Fraction

import numpy as np
import pytest

import fit_limits_inputs as FI
import minsnap_np as MN
import oracle as O
import sample_batch_ref as SR

from conftest import PKG


def _squash(s):
    return re.sub(r"\s+", "", s)


def test_restated_text_is_the_sources():
    text = {}
    for name, fname, want in FI.SOURCE_TEXT:
        if fname not in text:
            text[fname] = _squash(open(f"{PKG}/csrc/{fname}").read())
        assert _squash(want) in text[fname], (name, fname)


def test_boundaries():
    assert FI.limits() == {"batch": (670, 671), "gradient": (647, 648), "descent": (586, 587),
                           "refit": (4280, 4281), "refit big": (275, 276)}
    for entry, f in FI.LDS_BYTES.items():
        taken, refused = FI.limits()[entry]
        assert all(f(M) <= FI.K_LDS_BUDGET for M in range(1, taken + 1)), entry
        assert f(taken) <= FI.K_LDS_BUDGET < f(refused), (entry, f(taken), f(refused))
        print(entry, "largest", taken, f(taken), "bytes; first refused", refused, f(refused), "of", FI.K_LDS_BUDGET)
    assert FI.refit_layout(40)[:2] == (True, False) and FI.refit_layout(41)[:2] == (False, False)
    assert FI.refit_layout(275)[:2] == (False, False) and FI.refit_layout(276)[:2] == (False, True)
    assert FI.refit_segments() == (41, 275, 276, 4280)
    assert FI.mixed_batch_segments() == [1, 12, 670, 2, 41]
    # 41 segments are 42 waypoints: one past the refit's kernel-argument path (W <= 41)
    assert FI.refit_segments()[0] + 1 == FI.K_REFIT_ARG_W + 1


def test_start_values_are_distinct_and_large():
    for k in range(8):
        for x in FI.v0a0(k):
            assert (np.abs(x) >= 0.1).all() and len(set(np.abs(x).tolist())) == 3, (k, x)
    v, a = FI.v0a0_batch(5)
    assert len({tuple(r) for r in v}) == 5 and len({tuple(r) for r in a}) == 5


def test_row_counts():
    _, _, Tc = FI.track(FI.ROW_TRACK)
    C = FI.oracle_fit(FI.track(FI.ROW_TRACK)[0], Tc, *FI.v0a0(0))
    assert [R for R, _ in FI.row_cases()] == [1, 128, 129, 2048, 2049, 3000]
    for R, dt in FI.row_cases():
        assert FI.count_rows(Tc, dt) == R == len(O.sample_traj(Tc, C, dt)), (R, dt)
        assert float(np.sum(Tc)) / dt <= 2e4
    # the slices: one writer; one full chunk; two writers; 16 full chunks; 16 writers of 129
    # rows (a chunk of one row; the last writer 114); 188 rows each, chunks of 128 + 60
    assert [FI.refit_slices(R) for R, _ in FI.row_cases()] == [(1, 1), (1, 128), (2, 65), (16, 128), (16, 129),
                                                                (16, 188)]
    R = FI.ROW_COUNTS[-1]
    assert 2048 < R < 4096 and -(-R // 16) % 128 != 0
    for M in FI.refit_segments():
        assert FI.count_rows(FI.track(M)[2], FI.refit_dt(M)) > 2048, M


def test_caller_times_are_scaled_nfabian():
    for M in (1, 12, 41):
        wp, Tn, Tc = FI.track(M)
        assert np.array_equal(Tn, O.segment_times(wp, FI.V_MAX, FI.A_MAX))
        f = Tc / Tn
        assert (f >= 0.7).all() and (f <= 1.4).all() and (M == 1 or f.min() < f.max())


# ---- the comparisons bite -----------------------------------------------------------------
def _norm_err(C, truth, T):
    """test_gpu_minsnap._norm_err for one track."""
    Tn = np.asarray(T)[:, None, None] ** np.arange(10)[None, None, :]
    return float((np.abs(C - truth) * Tn).max() / (np.abs(truth) * Tn).max())


def _mutants(wp, T, v0, a0, fit):
    """The three wrong fits: v0's first two components swapped, a0 dropped, and the right fit
    with segment 0's coefficients (a one-segment track: axis 0's) moved up one slot."""
    right = fit(wp, T, v0, a0)
    shifted = right.copy()
    if len(T) > 1:
        shifted[0] = right[1]
    else:
        shifted[0, 0] = np.roll(right[0, 0], 1)
    return {"v0 swapped": fit(wp, T, v0[[1, 0, 2]], a0), "a0 dropped": fit(wp, T, v0, np.zeros(3)),
            "coefficients shifted": shifted}


@functools.lru_cache(maxsize=None)
def _truth(M):
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    return MN.track_batch_refined(wp[None], Tc[None], v0, a0)[0]


@pytest.mark.parametrize("M", [1, 2, 12, 41])
def test_coefficient_rule_rejects_each_mistake(M):
    """The batch fit's rule: _norm_err <= max(the oracle's own, twice the oracle's worst over the
    module's tracks).  The oracle's worst on these tracks is below 1e-7 (test_gpu_fit_limits.py
    records it); a mistake is off by the size of the coefficients."""
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    truth = _truth(M)
    eo = _norm_err(FI.oracle_fit(wp, Tc, v0, a0), truth, Tc)
    print(M, "oracle's distance from the truth", eo)
    assert eo < 1e-7
    for name, C in _mutants(wp, Tc, v0, a0, FI.oracle_fit).items():
        e = _norm_err(C, truth, Tc)
        print(M, name, e)
        assert e > 1e-4, (M, name, e)  # (three orders above any floor the rule can take)


@pytest.mark.parametrize("M", [12, 41])
def test_row_bound_rejects_each_mistake(M):
    """The refit's rule: the sampler's bound plus 1e-9 max(1, T_total)^2 against the truth on
    the right coefficients."""
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    dt = float(np.sum(Tc)) / 40.5
    right = FI.oracle_fit(wp, Tc, v0, a0)
    tr = SR.Truth(Tc, right, dt)
    extra = Fraction(1e-9) * Fraction(max(1.0, float(np.sum(Tc)))) ** 2
    ok, _ = tr.ratios(O.sample_traj(Tc, right, dt), extra)
    assert ok.all()
    for name, C in _mutants(wp, Tc, v0, a0, FI.oracle_fit).items():
        ok, _ = tr.ratios(O.sample_traj(Tc, C, dt), extra)
        assert not ok.all(), (M, name)
        # the first row is the start vertex itself: it shows v0 and a0 directly
        if name != "coefficients shifted":
            assert not ok[0].all(), (M, name)


def test_recorded_rows_of_the_largest_refit_are_this_tracks():
    """The record's time column is the restated recurrence on this module's track at its dt and
    T0, its first row the start vertex; the values are the oracle's at recording."""
    M = FI.limits()["refit"][0]
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    rows = FI.refit_largest_rows()
    seg, tin, tac = FI.CR.recurrence(Tc, FI.refit_dt(M))
    assert rows.shape == (len(seg), 10) and len(seg) > 2048 and np.isfinite(rows).all()
    assert rows[:, 9].tobytes() == (tac + np.float64(FI.T0)).tobytes()
    np.testing.assert_allclose(rows[0, [0, 3, 6]], wp[0], atol=1e-9)
    np.testing.assert_allclose(rows[0, [1, 4, 7]], v0, atol=1e-9)
    np.testing.assert_allclose(rows[0, [2, 5, 8]], a0, atol=1e-9)
    # rows that fall on a segment's start are that waypoint (tin = 0 never recurs; the nearest:
    # a row within 1 ms of a segment's start is within |v| * 1 ms of its waypoint)
    near = np.flatnonzero(tin < 1e-3)
    assert len(near) >= 1
    for r in near:
        v = np.linalg.norm(rows[r, [1, 4, 7]]) + 1.0
        assert np.linalg.norm(rows[r, [0, 3, 6]] - wp[seg[r]]) <= v * 1e-3, r


def test_held_entries():
    h = FI.held_entries(647)
    assert h[:3] == [0, 1, 16] and h[-3:] == [640, 645, 646] and len(h) == 44
    assert FI.kkt_entries(647) == [0, 1, 2, 646, 647]


@pytest.mark.parametrize("M", [3, 12])
def test_cost_and_gradient_bounds_reject_each_mistake(M):
    """The gradient's and the descent's rule: J within 2 D S and a gradient entry within
    2 (2 D S) / h of the truth, D by the restricted reference (which on all variants is
    time_alloc_ref.reference_distance)."""
    import time_alloc_ref as tr
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    t = FI.AllocTrack(f"m{M}", wp, Tc, v0, a0)
    every = list(range(M + 1))
    per, D = FI.alloc_reference(t, every, every)
    Dr, perr = tr.reference_distance([t], FI.H, FI.T_MIN)
    assert D == pytest.approx(Dr, rel=1e-6) and [per[v][0] for v in every] == perr[t.name][1].tolist()
    assert 0.0 < D < 64 * tr.EPS
    V = tr.variants(Tc, FI.H, FI.T_MIN)
    J = np.array([per[v][0] for v in every])
    S = np.array([per[v][1] for v in every])
    g = (J[1:] - J[0]) / FI.H
    bj, bg = 2 * D * S[0], 2 * (2 * D * np.maximum(S[1:], S[0])) / FI.H
    Ct = tr.solve(wp, V, v0, a0)
    shifted = Ct.copy()
    shifted[:, 0] = Ct[:, 1]
    mutants = {"v0 swapped": tr.costs_at(wp, V, v0[[1, 0, 2]], a0), "a0 dropped": tr.costs_at(wp, V, v0, np.zeros(3)),
               "coefficients shifted": np.array([tr.cost(v, c) for v, c in zip(V, shifted)])}
    for name, Jm in mutants.items():
        gm = (Jm[1:] - Jm[0]) / FI.H
        print(M, name, "J off by", abs(Jm[0] - J[0]) / bj, "bounds; g by", np.max(np.abs(gm - g) / bg))
        assert abs(Jm[0] - J[0]) > bj and (np.abs(gm - g) > bg).any(), (M, name)


def test_oracle_rows_reject_each_mistake():
    """The longest refit's rule: rows within 1e-6 of the oracle's."""
    M = 41
    wp, _, Tc = FI.track(M)
    v0, a0 = FI.v0a0(M)
    dt = float(np.sum(Tc)) / 40.5
    want = O.sample_traj(Tc, FI.oracle_fit(wp, Tc, v0, a0), dt)
    for name, C in _mutants(wp, Tc, v0, a0, FI.oracle_fit).items():
        got = O.sample_traj(Tc, C, dt)
        assert np.abs(got[:, :9] - want[:, :9]).max() > 1e-3, name
