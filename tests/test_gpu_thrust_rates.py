"""GPU: thrust and body rates of fitted tracks (include/epp.h): epp_sample_derivative_batch, any
derivative of the rows; epp_thrust_rates, the thrust, roll / pitch body rate and tilt of
samples; epp_traj_thrust_rates_batch, their extremes over the rows of fitted tracks straight
from the coefficients; and the Python / PathPlanner layers.

By definition the fused call is epp_sample_batch (the time column), epp_sample_derivative_batch
at orders 2 and 3, epp_thrust_rates on those values and per-track reductions that keep the
earliest row: every output is compared with that composition with ==.  Against the restatement
(thrust_rates_ref.py) the values are held to the square root's ulp (its compare_* functions,
which test_thrust_rates_cpu.py shows to reject four mistakes) and the rows are equal where the
restatement's extreme is separated from the runner-up.

Tracks: thrust_rates_inputs.py (its claims are checked on the CPU in
test_thrust_rates_inputs_cpu.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import clearance_ref as CR
import sample_batch_ref as SR
import thrust_rates_inputs as ti
import thrust_rates_ref as tr
from conftest import CONFIG
from eppamd import capi, synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fit():
    Ts, Cs, st = capi.minsnap_batch(list(ti.fit_waypoints()), ti.V_MAX, ti.A_MAX)
    assert (st == 0).all()
    return Ts, Cs


@functools.lru_cache(maxsize=None)
def _hand_ref():
    _, Ts, Cs, _, _ = ti.hand_tracks()
    return tr.tracks(Ts, Cs, ti.DT, ti.G)


# ---- 1. the derivative sampler -----------------------------------------------------------------
SD_DT = 0.1


@functools.lru_cache(maxsize=None)
def _sd_tracks():
    """A few fitted tracks (the long one among them), a hand-built one of more than two chunks,
    the many-segment one, and tracks without rows in between."""
    Ts, Cs = _fit()
    names, hT, hC, _, _ = ti.hand_tracks()
    pick = [names.index("thrust minimum on row 513"), names.index(f"{ti.K_SEG_LDS + 1} segments"),
            names.index("one waypoint"), names.index("NaN times")]
    keep = [0, 5, 11, 64]
    return ([Ts[k] for k in keep[:2]] + [hT[pick[2]], hT[pick[0]]] + [Ts[k] for k in keep[2:]] +
            [hT[pick[3]], hT[pick[1]]],
            [Cs[k] for k in keep[:2]] + [hC[pick[2]], hC[pick[0]]] + [Cs[k] for k in keep[2:]] +
            [hC[pick[3]], hC[pick[1]]])


def test_sample_derivative_orders_0_1_2_equal_the_row_sampler():
    Ts, Cs = _sd_tracks()
    rows = capi.sample_batch(Ts, Cs, SD_DT)
    cnt = capi.sample_count(Ts, SD_DT)
    assert (cnt[[2, 6]] == 0).all() and (np.delete(cnt, [2, 6]) > 0).all() and len(rows) == cnt.sum()
    for order in (0, 1, 2):
        got, roff = capi.sample_derivative(Ts, Cs, SD_DT, order)
        assert got.dtype == np.float64 and got.shape == (len(rows), 3) and np.array_equal(np.diff(roff), cnt)
        want = rows[:, [order, 3 + order, 6 + order]]
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (order, np.argwhere(got != want)[:4].tolist())


def test_sample_derivative_long_rows_equal_the_row_sampler():
    """More than two chunks of rows (DT = 2^-6) and the many-segment track."""
    names, hT, hC, _, _ = ti.hand_tracks()
    ks = [names.index("thrust minimum on row 1024"), names.index(f"{ti.K_SEG_LDS + 1} segments"),
          names.index("thrust minimum on the last of 513 rows")]
    Ts, Cs = [hT[k] for k in ks], [hC[k] for k in ks]
    rows = capi.sample_batch(Ts, Cs, ti.DT)
    assert len(rows) == ti.R_LONG + 226 + 513
    for order in (0, 1, 2):
        got, _ = capi.sample_derivative(Ts, Cs, ti.DT, order)
        assert got.tobytes() == np.ascontiguousarray(rows[:, [order, 3 + order, 6 + order]]).tobytes(), order


@pytest.mark.parametrize("order", [3, 4, 9])
def test_sample_derivative_equals_restatement(order):
    Ts, Cs = _sd_tracks()
    got, roff = capi.sample_derivative(Ts, Cs, SD_DT, order)
    for k in range(len(Ts)):
        rec = CR.recurrence(Ts[k], SD_DT)
        want = tr.track_values(Ts[k], Cs[k], SD_DT, order, rec)
        g = got[roff[k]:roff[k + 1]]
        assert g.shape == want.shape, k
        assert g.tobytes() == want.tobytes(), (k, order, np.argwhere(g != want)[:4].tolist())
        if order == 9:
            assert np.array_equal(g, 362880.0 * np.asarray(Cs[k])[rec[0], :, 9])


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, 9])
def test_sample_derivative_within_the_exact_bound(order):
    """Every value of every row against exact rational arithmetic (sample_batch_ref.exact) and
    its derived bound 32 * 2^-53 * S: the check that does not rest on the restatement."""
    Ts, Cs = _sd_tracks()
    got, roff = capi.sample_derivative(Ts, Cs, SD_DT, order)
    worst, n = 0.0, 0
    for k in range(len(Ts)):
        seg, tin, _ = CR.recurrence(Ts[k], SD_DT)
        g = got[roff[k]:roff[k + 1]]
        assert len(g) == len(seg), k
        Cf = np.asarray(Cs[k], np.float64)
        for r in range(len(g)):
            for d in range(3):
                p, S = SR.exact(Cf[seg[r], d], tin[r], order)
                assert SR.within(g[r, d], p, S), (k, r, d, order, float(g[r, d]), float(p))
                worst = max(worst, SR.ratio(g[r, d], p, S))
                n += 1
    assert n == 3 * roff[-1] and n > 3000
    print(f"order {order}: {n} values, worst |got - exact| / (32 * 2^-53 * S) = {worst:.3f}")


def test_sample_derivative_row_offsets_with_gaps():
    Ts, Cs = _sd_tracks()
    cnt = capi.sample_count(Ts, SD_DT)
    nt = len(Ts)
    roff = np.zeros(nt, np.int64)
    roff[1:] = np.cumsum(cnt + 3)[:-1]  # three rows of room behind every track
    roff += 2
    n_rows = int(roff[-1] + cnt[-1] + 3)
    dense, doff = capi.sample_derivative(Ts, Cs, SD_DT, 3)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    word = 0x7FF8_DEAD_BEEF_0001  # a NaN with a payload
    d_val, d_roff = capi._filled(24 * n_rows, word), capi.DeviceBuffer.from_array(roff)
    capi.check(capi.lib().epp_sample_derivative_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, SD_DT, 3, d_roff.ptr, d_val.ptr,
                                                      None))
    capi.sync()
    got = d_val.download(np.uint64, 3 * n_rows).reshape(n_rows, 3)
    written = np.zeros(n_rows, bool)
    for k in range(nt):
        written[roff[k]:roff[k] + cnt[k]] = True
        assert got[roff[k]:roff[k] + cnt[k]].tobytes() == dense[doff[k]:doff[k + 1]].tobytes(), k
    assert (got[~written] == word).all() and (~written).sum() == 3 * nt + 2
    # a NULL row_offsets: every track from row 0 (one track)
    capi.check(capi.lib().epp_sample_derivative_batch(d_T.ptr, d_C.ptr, d_off.ptr, 1, SD_DT, 3, None, d_val.ptr, None))
    capi.sync()
    assert d_val.download(np.float64, 3 * int(cnt[0])).tobytes() == dense[:cnt[0]].tobytes()


# ---- 2. per sample -----------------------------------------------------------------------------
def _samples(n):
    rs = np.random.RandomState(300 + n)
    a, j = rs.uniform(-20, 20, (n, 3)), rs.uniform(-60, 60, (n, 3))
    hand = [
        ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0]),                                # hover
        ([0.0, 0.0, -ti.G], [0.0, 0.0, 0.0]),                              # free fall: 0 / 0
        ([2.0 ** -560, 0.0, -ti.G], [0.0, 6 * 2.0 ** 400, 0.0]),           # x / 0 = +inf
        ([ti.G, 0.0, 0.0], [0.0, 1.0, 0.0]),                               # 45 degrees
        ([0.0, 0.0, -3 * ti.G], [1.0, 0.0, 0.0]),                          # upside down
        ([np.nan, 1.0, 2.0], [1.0, 2.0, 3.0]), ([1.0, 2.0, 3.0], [np.inf, 0.0, 0.0]),
        ([1e200, 0.0, 0.0], [0.0, 1.0, 0.0]),                              # f2 overflows
    ]
    for i, (x, y) in enumerate(hand[:n]):
        a[i], j[i] = x, y
    return a, j


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_thrust_rates_equal_restatement(n):
    a, j = _samples(n)
    got = capi.thrust_rates(a, j, ti.G)
    assert all(g.dtype == np.float64 and g.shape == (n,) for g in got)
    exp = tr.samples(a, j, ti.G)[:3]
    bad = tr.compare_samples(got, exp)
    fin = [np.isfinite(e) for e in exp]
    print(f"n {n}: worst ulps", [float(CR.ulps(g[f], e[f]).max()) if f.any() else 0.0 for g, e, f in zip(got, exp, fin)],
          "non-finite", [int((~f).sum()) for f in fin])
    assert bad == []
    if n >= 8:
        assert got[0][0] == ti.G and got[1][0] == 0.0 and got[2][0] == 1.0  # hover, exactly
        assert np.isinf(got[1]).any() and np.isnan(got[1]).any() and (got[0] == 0.0).any()


def test_thrust_rates_optional_outputs_may_be_null():
    a, j = _samples(65)
    full = capi.thrust_rates(a, j, ti.G)
    n = len(a)
    d_a, d_j = capi.DeviceBuffer.from_array(a), capi.DeviceBuffer.from_array(j)
    d_f, d_x = capi.DeviceBuffer(8 * n), capi.DeviceBuffer(8 * n)
    L = capi.lib()
    capi.check(L.epp_thrust_rates(d_a.ptr, d_j.ptr, n, ti.G, d_f.ptr, None, None, None))
    capi.sync()
    assert d_f.download(np.float64, n).tobytes() == full[0].tobytes()
    capi.check(L.epp_thrust_rates(d_a.ptr, d_j.ptr, n, ti.G, d_f.ptr, None, d_x.ptr, None))
    capi.sync()
    assert d_x.download(np.float64, n).tobytes() == full[2].tobytes()
    capi.check(L.epp_thrust_rates(d_a.ptr, d_j.ptr, n, ti.G, d_f.ptr, d_x.ptr, None, None))
    capi.sync()
    assert d_x.download(np.float64, n).tobytes() == full[1].tobytes()


# ---- 3. the fused call against the composition -------------------------------------------------
def _compose(Ts, Cs, dt, g):
    """The definition, on the device's own values: the time column of epp_sample_batch, the
    order-2 and order-3 values of epp_sample_derivative_batch, epp_thrust_rates on them, and
    the reductions in numpy.  Returns (out, rows, per-track (thrust, rate, cos_tilt))."""
    rows = capi.sample_batch(Ts, Cs, dt)
    acc, roff = capi.sample_derivative(Ts, Cs, dt, 2)
    jerk, _ = capi.sample_derivative(Ts, Cs, dt, 3)
    assert len(rows) == len(acc) == len(jerk) == roff[-1]
    f, w, c = capi.thrust_rates(acc, jerk, g)
    out, idx, per = np.empty((len(Ts), 8)), np.empty((len(Ts), 4), np.int64), []
    for k in range(len(Ts)):
        s = slice(roff[k], roff[k + 1])
        out[k], idx[k] = tr.reduce(f[s], w[s], c[s], rows[s, 9])
        per.append((f[s], w[s], c[s]))
    return out, idx, per


def _assert_equals_composition(Ts, Cs, dt, g):
    exp_out, exp_rows, per = _compose(Ts, Cs, dt, g)
    out, rows = capi.trajectory_thrust_rates(Ts, Cs, dt, g)
    assert out.dtype == np.float64 and out.shape == (len(Ts), 8) and rows.dtype == np.int64 and rows.shape == (len(Ts), 4)
    assert np.array_equal(rows, exp_rows), np.argwhere(rows != exp_rows)[:8].tolist()
    assert out.tobytes() == exp_out.tobytes(), (np.argwhere(out != exp_out)[:8].tolist())
    return out, rows, per


@pytest.mark.parametrize("dt", ti.FIT_DTS)
def test_fitted_tracks_equal_composition(dt):
    Ts, Cs = _fit()
    assert len(Ts) == 65 and len(Ts[64]) == ti.FIT_LONG > ti.K_SEG_LDS
    out, rows, _ = _assert_equals_composition(Ts, Cs, dt, ti.GRAVITY)
    assert (rows >= 0).all() and np.isfinite(out).all()
    print(f"dt {dt}: f_min {out[:, 0].min():.3f}..{out[:, 0].max():.3f}, rate_max up to {out[:, 4].max():.3f} rad/s, "
          f"largest tilt {np.degrees(np.arccos(out[:, 6].min())):.1f} deg, rows up to {rows.max()}")


def test_hand_tracks_equal_composition_and_claims():
    names, Ts, Cs, want_out, want_rows = ti.hand_tracks()
    out, rows, _ = _assert_equals_composition(Ts, Cs, ti.DT, ti.G)
    for k, name in enumerate(names):
        claimed = ~np.isnan(want_out[k])
        assert np.array_equal(out[k][claimed], want_out[k][claimed]), (name, out[k], want_out[k])
        claimed = want_rows[k] != -2
        assert np.array_equal(rows[k][claimed], want_rows[k][claimed]), (name, rows[k], want_rows[k])
    # single-track batches equal their slice of the full batch
    for k, name in enumerate(names):
        o1, r1 = capi.trajectory_thrust_rates(Ts[k:k + 1], Cs[k:k + 1], ti.DT, ti.G)
        assert o1.tobytes() == out[k:k + 1].tobytes() and np.array_equal(r1, rows[k:k + 1]), name


def test_rows_may_be_null():
    names, Ts, Cs, _, _ = ti.hand_tracks()
    nt = len(Ts)
    out, _ = capi.trajectory_thrust_rates(Ts, Cs, ti.DT, ti.G)
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    d_out = capi.DeviceBuffer(64 * nt)
    capi.check(capi.lib().epp_traj_thrust_rates_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, ti.DT, ti.G, d_out.ptr, None, None))
    capi.sync()
    assert d_out.download(np.float64, 8 * nt).tobytes() == out.tobytes()


# ---- 4. against the restatement ----------------------------------------------------------------
def _by_row(tracks_ref, rows_ref):
    return np.array([all(tr.separated(v, m, rows_ref[k, q]) for q, (v, m) in enumerate(t.quantities()))
                     for k, t in enumerate(tracks_ref)])


def test_hand_tracks_equal_restatement():
    names, Ts, Cs, _, _ = ti.hand_tracks()
    exp_out, exp_rows, ref = _hand_ref()
    by_row = _by_row(ref, exp_rows)
    assert by_row.all()  # (exact inputs: the same on the CPU and here)
    out, rows = capi.trajectory_thrust_rates(Ts, Cs, ti.DT, ti.G)
    bad = tr.compare_tracks(out, rows, exp_out, exp_rows, by_row)
    assert bad == [], [(names[k], what) for k, what in bad]


def test_fitted_tracks_equal_restatement():
    Ts, Cs = _fit()
    dt = ti.FIT_REF_DT
    exp_out, exp_rows, ref = tr.tracks(Ts, Cs, dt, ti.GRAVITY)  # (on the GPU's fits)
    by_row = _by_row(ref, exp_rows)
    print("tracks compared with the composition only:", np.flatnonzero(~by_row).tolist())
    assert (~by_row).sum() <= 1
    out, rows = capi.trajectory_thrust_rates(Ts, Cs, dt, ti.GRAVITY)
    bad = tr.compare_tracks(out, rows, exp_out, exp_rows, by_row)
    fin = np.isfinite(exp_out)
    print("worst ulps per output:", CR.ulps(np.where(fin, out, 0.0), np.where(fin, exp_out, 0.0)).max(axis=0).tolist())
    assert bad == [], bad[:8]
    # the per-sample values of the same rows
    acc, roff = capi.sample_derivative(Ts, Cs, dt, 2)
    jerk, _ = capi.sample_derivative(Ts, Cs, dt, 3)
    got = capi.thrust_rates(acc, jerk, ti.GRAVITY)
    exp = [np.concatenate([getattr(t, q) for t in ref]) for q in ("thrust", "rate", "cos_tilt")]
    assert acc.tobytes() == np.concatenate([t.acc for t in ref]).tobytes()
    assert jerk.tobytes() == np.concatenate([t.jerk for t in ref]).tobytes()
    assert tr.compare_samples(got, exp) == []


# ---- 5. more tracks than the persistent grid ---------------------------------------------------
def test_more_tracks_than_workgroups():
    cus = capi.cu_count()  # (the count the library sizes its persistent grids by)
    assert cus >= 1
    n = 2 * 8 * cus + 1
    Ts, Cs = ti.short_tracks(n)
    out, rows = capi.trajectory_thrust_rates(Ts, Cs, ti.DT, ti.G)
    for k in (0, 1):  # the two distinct tracks, each alone, against every copy in the batch
        o1, r1, _ = _assert_equals_composition(Ts[k:k + 1], Cs[k:k + 1], ti.DT, ti.G)
        assert r1[0].tolist() == [1 + k, 0, 1 + k, 0]  # (k == 0: rows 0 and 2 tie for the largest thrust)
        assert (out[k::2] == o1[0]).all() and (rows[k::2] == r1[0]).all()
    print(f"{n} tracks on {cus} CUs")


# ---- 6. graph capture, 7. argument errors ------------------------------------------------------
def test_graph_replay():
    names, Ts, Cs, _, _ = ti.hand_tracks()
    keep = [names.index(n) for n in ("thrust minimum on row 513", "free fall", "one waypoint", "hover")]
    A = ([Ts[k] for k in keep], [Cs[k] for k in keep])
    B = (A[0], [c * 0.5 for c in A[1]])  # the same times, other coefficients
    nt = len(keep)
    L = capi.lib()
    cnt = capi.sample_count(A[0], ti.DT)
    roff = np.zeros(nt, np.int64)
    roff[1:] = np.cumsum(cnt)[:-1]
    R = int(cnt.sum())
    d_T, d_C, d_off, _, nseg = capi._upload_tracks(*A)
    d_roff = capi.DeviceBuffer.from_array(roff)
    outs = [capi.DeviceBuffer(b) for b in (64 * nt, 32 * nt, 24 * R, 24 * R, 8 * R, 8 * R, 8 * R)]
    d_out, d_rows, d_acc, d_jerk, d_f, d_w, d_c = outs
    s, g = C.c_void_p(), C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(s)))
    capi.check(L.epp_graph_begin(s.value))
    capi.check(L.epp_traj_thrust_rates_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, ti.DT, ti.G, d_out.ptr, d_rows.ptr, s.value))
    capi.check(L.epp_sample_derivative_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, ti.DT, 2, d_roff.ptr, d_acc.ptr, s.value))
    capi.check(L.epp_sample_derivative_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, ti.DT, 3, d_roff.ptr, d_jerk.ptr, s.value))
    capi.check(L.epp_thrust_rates(d_acc.ptr, d_jerk.ptr, R, ti.G, d_f.ptr, d_w.ptr, d_c.ptr, s.value))
    capi.check(L.epp_graph_end(s.value, C.byref(g)))
    results = []
    for Tk, Ck in (A, B):
        exp_out, exp_rows = capi.trajectory_thrust_rates(Tk, Ck, ti.DT, ti.G)
        acc, _ = capi.sample_derivative(Tk, Ck, ti.DT, 2)
        jerk, _ = capi.sample_derivative(Tk, Ck, ti.DT, 3)
        exp = capi.thrust_rates(acc, jerk, ti.G)
        d_C.upload(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3, 10) for c in Ck]))
        for b in outs:
            capi.check(L.epp_memset(b.ptr, 0x5A, b.nbytes, None))  # poison
        capi.sync()
        capi.check(L.epp_graph_launch(g.value, s.value))
        capi.check(L.epp_stream_sync(s.value))
        assert d_out.download(np.float64, 8 * nt).tobytes() == exp_out.tobytes()
        assert np.array_equal(d_rows.download(np.int64, 4 * nt).reshape(nt, 4), exp_rows)
        assert d_acc.download(np.float64, 3 * R).tobytes() == acc.tobytes()
        assert d_jerk.download(np.float64, 3 * R).tobytes() == jerk.tobytes()
        for b, e in zip((d_f, d_w, d_c), exp):
            assert b.download(np.float64, R).tobytes() == e.tobytes()
        results.append(exp_out)
    assert results[0].tobytes() != results[1].tobytes()  # (the replay saw the changed coefficients)
    capi.check(L.epp_graph_destroy(g.value))
    L.epp_stream_destroy(s.value)


def test_argument_errors_leave_outputs_untouched():
    names, Ts, Cs, _, _ = ti.hand_tracks()
    Ts, Cs = Ts[:4], Cs[:4]
    nt = 4
    L = capi.lib()
    d_T, d_C, d_off, _, _ = capi._upload_tracks(Ts, Cs)
    a, j = _samples(64)
    d_a, d_j = capi.DeviceBuffer.from_array(a), capi.DeviceBuffer.from_array(j)
    size = 1 << 17  # every output of every call below lies in here
    out = capi.DeviceBuffer(size)
    capi.check(L.epp_memset(out.ptr, 0x5A, size, None))
    capi.sync()
    o = [out.ptr + (size // 4) * k for k in range(4)]
    nan, inf = float("nan"), float("inf")
    t = (d_T.ptr, d_C.ptr, d_off.ptr)
    bad = capi.EPP_ERR_INVALID_ARGUMENT
    for name, args in {
        "order -1": (*t, nt, ti.DT, -1, None, o[0]), "order 10": (*t, nt, ti.DT, 10, None, o[0]),
        "n_tracks < 0": (*t, -1, ti.DT, 2, None, o[0]), "dt == 0": (*t, nt, 0.0, 2, None, o[0]),
        "dt < 0": (*t, nt, -ti.DT, 2, None, o[0]), "dt NaN": (*t, nt, nan, 2, None, o[0]),
        "dt inf": (*t, nt, inf, 2, None, o[0]), "NULL seg_times": (None, d_C.ptr, d_off.ptr, nt, ti.DT, 2, None, o[0]),
        "NULL coeffs": (d_T.ptr, None, d_off.ptr, nt, ti.DT, 2, None, o[0]),
        "NULL wp_offsets": (d_T.ptr, d_C.ptr, None, nt, ti.DT, 2, None, o[0]),
    }.items():
        assert L.epp_sample_derivative_batch(*args, None) == bad, name
    assert L.epp_sample_derivative_batch(*t, nt, ti.DT, 2, None, None, None) == bad
    for name, args in {
        "n < 0": (d_a.ptr, d_j.ptr, -1, ti.G, o[0], o[1], o[2]), "g NaN": (d_a.ptr, d_j.ptr, 64, nan, o[0], o[1], o[2]),
        "g inf": (d_a.ptr, d_j.ptr, 64, inf, o[0], o[1], o[2]), "NULL acc": (None, d_j.ptr, 64, ti.G, o[0], o[1], o[2]),
        "NULL jerk": (d_a.ptr, None, 64, ti.G, o[0], o[1], o[2]),
        "NULL thrust": (d_a.ptr, d_j.ptr, 64, ti.G, None, o[1], o[2]),
    }.items():
        assert L.epp_thrust_rates(*args, None) == bad, name
    for name, args in {
        "n_tracks < 0": (*t, -1, ti.DT, ti.G, o[0], o[1]), "dt == 0": (*t, nt, 0.0, ti.G, o[0], o[1]),
        "dt < 0": (*t, nt, -ti.DT, ti.G, o[0], o[1]), "dt NaN": (*t, nt, nan, ti.G, o[0], o[1]),
        "dt inf": (*t, nt, inf, ti.G, o[0], o[1]), "g NaN": (*t, nt, ti.DT, nan, o[0], o[1]),
        "g inf": (*t, nt, ti.DT, inf, o[0], o[1]),
        "NULL seg_times": (None, d_C.ptr, d_off.ptr, nt, ti.DT, ti.G, o[0], o[1]),
        "NULL coeffs": (d_T.ptr, None, d_off.ptr, nt, ti.DT, ti.G, o[0], o[1]),
        "NULL wp_offsets": (d_T.ptr, d_C.ptr, None, nt, ti.DT, ti.G, o[0], o[1]),
        "NULL out": (*t, nt, ti.DT, ti.G, None, o[1]),
    }.items():
        assert L.epp_traj_thrust_rates_batch(*args, None) == bad, name
    # empty batches launch nothing
    capi.check(L.epp_sample_derivative_batch(None, None, None, 0, ti.DT, 2, None, o[0], None))
    capi.check(L.epp_thrust_rates(None, None, 0, ti.G, o[0], o[1], o[2], None))
    capi.check(L.epp_traj_thrust_rates_batch(None, None, None, 0, ti.DT, ti.G, o[0], o[1], None))
    capi.sync()
    assert (out.download(np.uint8, size) == 0x5A).all()


# ---- 8. C++ / pybind ---------------------------------------------------------------------------
def test_path_planner_candidate_thrust_rates():
    import online_traj_planner as otp
    gates, obstacles = synth.track_world(42)
    pp = otp.PathPlanner(np.array(gates), np.array(obstacles), CONFIG)
    sets = [np.asarray(w) for w in ti.fit_waypoints()[:12]]
    Ts, Cs, st = capi.minsnap_batch(sets, 1.0, 2.0)
    assert (st == 0).all()
    for g in (9.81, 3.71):
        exp_out, exp_rows = capi.trajectory_thrust_rates(Ts, Cs, 0.05, g)
        out, rows = pp.candidate_thrust_rates(sets, 1.0, 2.0, 0.05, g)
        assert out.dtype == np.float64 and out.shape == (12, 8) and rows.dtype == np.int64 and rows.shape == (12, 4)
        assert out.tobytes() == exp_out.tobytes() and np.array_equal(rows, exp_rows)
    out, rows = pp.candidate_thrust_rates(sets, 1.0, 2.0, 0.05)  # g defaults to 9.81
    assert out.tobytes() == capi.trajectory_thrust_rates(Ts, Cs, 0.05)[0].tobytes()
    print("f_min", out[:, 0].round(3).tolist(), "rate_max", out[:, 4].round(3).tolist())
    with pytest.raises(ValueError, match="At least two waypoints are required"):
        pp.candidate_thrust_rates([sets[0], sets[1][:1]], 1.0, 2.0, 0.05)
    assert [r.shape for r in pp.candidate_thrust_rates([], 1.0, 2.0, 0.05)] == [(0, 8), (0, 4)]
