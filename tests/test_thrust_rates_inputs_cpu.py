"""CPU: the claims of thrust_rates_inputs.py, proven with the restatement (thrust_rates_ref.py)
and, for the fitted tracks, with the oracle's fits standing in for the GPU's."""
import functools

import numpy as np

import clearance_ref as CR
import oracle as O
import thrust_rates_inputs as ti
import thrust_rates_ref as tr


@functools.lru_cache(maxsize=None)
def _hand():
    names, Ts, Cs, want_out, want_rows = ti.hand_tracks()
    return names, Ts, Cs, want_out, want_rows, tr.tracks(Ts, Cs, ti.DT, ti.G)


def test_fitted_tracks_lie_on_both_sides_of_the_lds_stage_and_are_separated():
    wps = ti.fit_waypoints()
    segs = [len(w) - 1 for w in wps]
    assert min(segs) >= 1 and min(segs) <= ti.K_SEG_LDS < max(segs) == ti.FIT_LONG
    assert sum(s <= ti.K_SEG_LDS for s in segs) == 64
    Ts, Cs, _ = O.minsnap_batch(list(wps), ti.V_MAX, ti.A_MAX, threads=8)
    out, rows, tracks = tr.tracks(Ts, Cs, ti.FIT_REF_DT, ti.GRAVITY)
    assert (rows >= 0).all() and np.isfinite(out).all()
    # a fitted track starts and ends at rest; in between it is neither in free fall nor level
    assert (out[:, 0] > 5.0).all() and (out[:, 2] > out[:, 0]).all() and (out[:, 4] > 0).all()
    assert (out[:, 6] > 0.9).all() and (out[:, 6] < 1.0).all()
    assert len({len(t.time) for t in tracks}) > 10 and max(len(t.time) for t in tracks) > ti.ROW_CHUNK
    for k, t in enumerate(tracks):
        for q, (v, is_min) in enumerate(t.quantities()):
            assert tr.separated(v, is_min, rows[k, q]), (k, q)


def test_hand_tracks_row_times_and_values_are_exact():
    names, Ts, Cs, _, _, (_, _, tracks) = _hand()
    assert ti.DT == 2.0 ** -6 and ti.G * 16 == int(ti.G * 16) and ti.R_LONG > 2 * ti.ROW_CHUNK
    for name, T, t in zip(names, Ts, tracks):
        if len(T) and np.isfinite(T).all():
            assert np.array_equal(t.time, np.arange(len(t.time)) * ti.DT), name  # row j at j DT exactly
    counts = dict(zip(names, (len(t.time) for t in tracks)))
    assert counts["constant acceleration"] == ti.R_LONG and counts["1 row"] == 1
    assert counts["one waypoint"] == counts["NaN times"] == counts["NaN times (early)"] == 0
    assert counts["thrust minimum on the last of 512 rows"] == 512
    assert counts["thrust minimum on the last of 513 rows"] == 513
    # the recurrence of the many-segment track: the row the minimum is claimed on lies in the last segment
    k = names.index(f"{ti.K_SEG_LDS + 1} segments")
    seg, tin, _ = CR.recurrence(Ts[k], ti.DT)
    assert len(Ts[k]) > ti.K_SEG_LDS and seg[ti.MANY_ROW] == len(Ts[k]) - 1 and tin[ti.MANY_ROW] == 2 * ti.DT


def test_hand_tracks_claims():
    names, Ts, Cs, want_out, want_rows, (out, rows, tracks) = _hand()
    for k, name in enumerate(names):
        claimed = ~np.isnan(want_out[k])
        assert np.array_equal(out[k][claimed], want_out[k][claimed]), (name, out[k], want_out[k])
        claimed = want_rows[k] != -2
        assert np.array_equal(rows[k][claimed], want_rows[k][claimed]), (name, rows[k], want_rows[k])
        for q, (v, is_min) in enumerate(tracks[k].quantities()):
            assert tr.separated(v, is_min, rows[k, q]), (name, q)
    t = dict(zip(names, tracks))
    # (a) every row the same bits
    a = t["constant acceleration"]
    for v in (a.thrust, a.rate, a.cos_tilt):
        assert len(set(v.tobytes()[8 * i:8 * i + 8] for i in range(len(v)))) == 1
    # (b) exact free fall: f2 == 0 on every row, rate and cos_tilt 0 / 0
    b = t["free fall"]
    assert (b.f2 == 0).all() and (b.thrust == 0).all() and np.isnan(b.rate).all() and np.isnan(b.cos_tilt).all()
    # (b') x / 0 = +inf on the chosen row only
    for r in (0, 700):
        c = t[f"free fall, sideways jerk, row {r}"]
        assert c.f2[r] == 0 and c.rate[r] == np.inf and np.isnan(c.cos_tilt[r])
        assert np.isfinite(np.delete(c.rate, r)).all() and (np.delete(c.f2, r) > 0).all()
    # (c) the chosen rows cover the lane, the wave reduction and both chunk boundaries
    assert {63, 64, ti.ROW_CHUNK - 1, ti.ROW_CHUNK, ti.ROW_CHUNK + 1, 2 * ti.ROW_CHUNK - 1, 2 * ti.ROW_CHUNK, 0,
            ti.LAST} == set(ti.MIN_ROWS)


def test_short_tracks():
    Ts, Cs = ti.short_tracks(5)
    out, rows, tracks = tr.tracks(Ts, Cs, ti.DT, ti.G)
    assert [len(t.time) for t in tracks] == [3] * 5 and rows[:, 0].tolist() == [1, 2, 1, 2, 1]
    assert all(len(T) == 1 for T in Ts)
