"""CPU: the inputs of test_gpu_clearance.py (clearance_inputs.py) checked with the numpy
restatement alone (clearance_ref.py): the restated recurrence gives the oracle sampler's rows,
every track's minimum is separated from its runner-up by more than 1e-9 relative except for
the deliberate exact ties, zero and positive clearances occur where the cases claim them, and
the closest rows land where the cases say.  The fitted tracks here are the oracle's own fits
of the GPU test's waypoints (the GPU fits differ from them by rounding only)."""
import functools

import numpy as np
import pytest

import clearance_inputs as ci
import clearance_ref as cr
import oracle as O
import small_path_inputs as spi
import trajsweep_inputs as tsi


@functools.lru_cache(maxsize=None)
def _fit():
    sets = tsi.fit_waypoints()
    fits = [O.minsnap_track(wp, 1.0, 2.0) for wp in sets]
    return [np.asarray(f[0], float) for f in fits], [np.asarray(f[1], float).reshape(-1, 3, 10) for f in fits]


@functools.lru_cache(maxsize=None)
def _fit_rows():
    Ts, Cs = _fit()
    return [cr.sample_rows(T, Cf, ci.FIT_DT) for T, Cf in zip(Ts, Cs)]


def _separation(d2m, ob=None):
    """(min, runner-up) over all (row, OBB) pairs of one track, NaN / inf pairs aside.  With ob:
    pairs of the minimum's own row against another box of the same gate are left out of the
    runner-up -- the frame boxes of a gate share edges, and a row closest to a shared edge is
    equally far from both by construction (a structural tie, like two mirror-image boxes; both
    sides evaluate it with the same operations on the same bits, so the lower index wins on
    both)."""
    f = np.where(np.isfinite(d2m), d2m, np.inf)
    r, i = np.unravel_index(np.argmin(f), f.shape)
    lo = f[r, i]
    rest = f.copy()
    rest[r, i] = np.inf
    if ob is not None and ob[i]["is_gate"]:
        g = 6 * (i // 6)  # (config_filling.json: 6 OBBs per gate, the gates first)
        assert ob[g:g + 6]["is_gate"].all()
        rest[r, g:g + 6] = np.inf
    return lo, rest.min()


def test_restated_rows_are_the_oracle_samplers():
    """Row count and time column exactly; positions to the 1e-12 the two Horner orders allow."""
    Ts, Cs = _fit()
    names, eTs, eCs, _, _ = ci.edge_tracks()
    for T, Cf, rows in list(zip(Ts, Cs, _fit_rows()))[::4] + [(T, Cf, cr.sample_rows(T, Cf, ci.DT))
                                                           for T, Cf in zip(eTs, eCs) if len(T) and np.isfinite(T).all()]:
        ref = O.sample_traj(T, Cf, ci.FIT_DT)
        assert len(ref) == len(rows[0])
        assert np.array_equal(ref[:, 9], rows[1])
        assert np.allclose(ref[:, [0, 3, 6]], rows[0], rtol=0, atol=1e-12)


def test_edge_tracks_land_where_they_claim():
    names, Ts, Cs, want, zero = ci.edge_tracks()
    ob = ci.obbs("1")
    assert len(ob) == 1 and not ob[0]["filling"]
    rows = [cr.sample_rows(T, Cf, ci.DT) for T, Cf in zip(Ts, Cs)]
    d2, row, time, near = cr.tracks(ob, Ts, Cs, ci.DT, rows)
    assert row.tolist() == want, list(zip(names, row.tolist(), want))
    n_rows = dict(zip(names, (len(r[0]) for r in rows)))
    for name, n in ci.EDGE_ROWS.items():
        assert n_rows[name] == n, (name, n_rows[name])
    assert n_rows["row R-1"] == 20 and n_rows["row 1024"] >= 1026 and n_rows[f"{ci.K_SEG_LDS + 1} segments"] > 201
    k = names.index("segment boundary, row 5")  # rows 5 and 6 come from different polynomials
    seg = cr.recurrence(Ts[k], ci.DT)[0]
    assert seg[5] == 0 and seg[6] == 1
    for k, name in enumerate(names):
        if want[k] < 0:
            assert np.isinf(d2[k]) and time[k] == -1.0 and near[k] == -1
            continue
        assert (d2[k] == 0.0) == zero[k], name
        assert near[k] == 0 and time[k] == rows[k][1][want[k]]
        d2m = cr.d2_matrix(ob, rows[k][0])
        if name == "resting":  # every row equal: row 0 wins an exact tie
            assert (d2m == d2m[0]).all() and d2[k] > 0.0
        elif zero[k]:  # rows inside the box tie at 0: the first one wins
            inside = np.flatnonzero(d2m[:, 0] == 0.0)
            assert inside[0] == want[k] and len(inside) > 1 and d2m[want[k] - 1, 0] > 1e-6
        else:
            lo, up = _separation(d2m)
            assert up > lo * (1 + 1e-9) and lo > 0.0, (name, lo, up)


@pytest.mark.parametrize("name", ci.WORLDS)
def test_fitted_tracks_have_separated_minima(name):
    ob = ci.obbs(name)
    Ts, Cs = _fit()
    rows = _fit_rows()
    d2, row, time, near = cr.tracks(ob, Ts, Cs, ci.FIT_DT, rows)
    if name == "filling":
        assert ob["filling"].all() and np.isinf(d2).all() and (row == -1).all() and (near == -1).all()
        return
    assert (near >= 0).all() and not ob["filling"][near].any()
    ties = 0
    for k in range(len(Ts)):
        d2m = cr.d2_matrix(ob, rows[k][0])
        lo, up = _separation(d2m, ob)
        if lo == 0.0:  # rows inside a box: exact ties at 0, the earliest row and lowest OBB win
            ties += 1
            continue
        assert up > lo * (1 + 1e-9), (name, k, lo, up)
    print(f"{name}: zero clearance {int((d2 == 0).sum())}, positive {int((d2 > 0).sum())}, "
          f"min positive {np.sqrt(d2[d2 > 0].min()):.3g}, max {np.sqrt(d2.max()):.3g}")
    assert (d2 > 0).sum() >= 4  # (the 1100-OBB world is dense: most tracks touch a box there)
    if name in ("72", "300", "1100", "T", "T+1"):
        assert (d2 == 0).sum() >= 4
    if name == "1100":  # the nearest OBB lies past the first tile for some track
        assert (near >= ci.T).sum() >= 1


@pytest.mark.parametrize("name", ["T+1", "1100"])
def test_last_box_track_is_nearest_the_last_box(name):
    ob = ci.obbs(name)
    T, Cf = ci.last_box_track(name)
    rows = cr.sample_rows(T, Cf, ci.DT)
    d2, row, time, near = cr.tracks(ob, [T], [Cf], ci.DT, [rows])
    assert len(rows[0]) == 11 and row[0] == 0  # (ten additions of 0.1 stay below 1.0) and near[0] == len(ob) - 1 and near[0] >= ci.T
    assert abs(np.sqrt(d2[0]) - 0.02) < 1e-12
    lo, up = _separation(cr.d2_matrix(ob, rows[0]))
    assert up > lo * (1 + 1e-9)


@pytest.mark.parametrize("name", ci.WORLDS)
def test_state_sets_hold_what_they_claim(name):
    ob = ci.obbs(name)
    pts = ci.points(name, ci.BLOCK + 1)
    d2, near = cr.states(ob, pts)
    finite = np.isfinite(pts).all(axis=1)
    assert (~finite).sum() == 5 and np.isinf(d2[~finite]).all() and (near[~finite] == -1).all()
    if name == "filling":
        assert np.isinf(d2).all() and (near == -1).all()
        return
    assert np.isfinite(d2[finite]).all() and (near[finite] >= 0).all()
    assert (d2 == 0).sum() >= 24 and (d2 > 0).sum() >= 64
    assert (np.sqrt(d2[finite]) > 40.0).sum() == 3  # the points 50 m outside everything
    if name in ("1100", "T+1"):
        assert (near >= ci.T).any()


def test_consistency_case_stays_clear_of_both_thresholds():
    """The property test's tracks (72 OBBs, md = half the smaller inflate radius): no clearance
    within 1e-6 of md or of sqrt(3) md, and both sides of both thresholds occur."""
    _, rg, ro = spi.setup()
    md = 0.5 * min(rg, ro)
    Ts, Cs = _fit()
    d2 = cr.tracks(ci.obbs("72"), Ts, Cs, ci.FIT_DT, _fit_rows())[0]
    clr = np.sqrt(d2)
    assert (np.abs(clr - md) > 1e-6).all() and (np.abs(clr - np.sqrt(3) * md) > 1e-6).all()
    assert (clr < md).sum() >= 4 and (clr > np.sqrt(3) * md).sum() >= 4
