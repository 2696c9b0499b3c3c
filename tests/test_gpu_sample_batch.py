"""GPU: the batched row sampler itself -- epp_sample_count / epp_sample_batch (k_sample_count,
k_sample_rows) through capi.sample_count / capi.sample_batch -- against the exact reference of
tests/sample_batch_ref.py: all ten columns, per-track t0, caller-laid row offsets, the chunk
edges with every coefficient live, the recurrence's edge cases, and the single-track refit
path beside the batch.  Every fused track kernel is tested "by definition" against a
composition that starts with these two calls; this module is what holds the calls themselves.

The value columns are held to |got - truth| <= 32 * 2^-53 * sum_j B[k][j] |c_j| |tin|^(j-k)
against exact rational arithmetic (derived in sample_batch_ref.py, shown to reject a wrong
derivative order, segment, tin and a dropped coefficient in test_sample_batch_cpu.py), the
position columns also bit for bit to the fused Horner of clearance_ref.horner, the time column
and the counts exactly.

Observed on an MI355X, worst |got - truth| / bound over the batches of this module (the ragged
fits 6,694 rows, the chunk edges 2,579, the recurrence edges 468, the three batch fits of
section 6): derivative 0: 0.041, derivative 1: 0.060, derivative 2: 0.083 -- well below the
1/3 the derivation leaves.  (The oracle's unfused Horner on the same inputs: 0.056, 0.070, 0.096.)

The single-track path against the batch (section 6): the time column is ==, the value columns
are NOT == (3, 12 and 40 segments: max |single - batch| 6.0e-13, 5.9e-13, 8.6e-13).  The two
fits run the same solve_track with different parameters: the batch kernel (k_minsnap) with 64
threads and the iterative-refinement step, the refit (k_refit) with 256 threads and without
that step (EPP_REFIT_REFINE, off: it cost 6-7 us of a ~30 us call) -- read in
csrc/minsnap_refit.hip, whose comment "the same arithmetic, so the same coefficients" speaks of the
G workgroups of one refit launch, and now says so.  Making them equal would put the
refinement back on the latency path, so the test asserts instead that both sides' rows are
within the bound of the truth evaluated on the batch's coefficients, the single-track rows
with 1e-9 * max(1, T_total)^2 more (the coefficient distance test_batch_vs_truth enforces,
carried through the acceleration column); without that allowance they are at up to 277 bounds
(~1e-12 absolute).
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import oracle as O
import sample_batch_inputs as SI
import sample_batch_ref as SR
from eppamd import capi

pytestmark = pytest.mark.gpu

DT = SI.DT


@functools.lru_cache(maxsize=None)
def _ragged():
    """(Ts, Cs) of the ragged batch, the fits by the device; shared and left unchanged."""
    tracks, v0, a0 = SI.fit_problem()
    Ts, Cs, st = capi.minsnap_batch(tracks, 1.0, 2.0, v0, a0)
    assert (st == 0).all()
    return SI.ragged(Ts, Cs)


@functools.lru_cache(maxsize=None)
def _ragged_truths():
    Ts, Cs = _ragged()
    return [SR.Truth(T, Cf, DT) for T, Cf in zip(Ts, Cs)]


@functools.lru_cache(maxsize=None)
def _ragged_rows():
    """(counts, row offsets (n + 1), rows) of the plain call: t0 None, contiguous."""
    Ts, Cs = _ragged()
    cnt = capi.sample_count(Ts, DT)
    roff = np.zeros(len(Ts) + 1, np.int64)
    roff[1:] = np.cumsum(cnt)
    rows = capi.sample_batch(Ts, Cs, DT)
    assert rows.shape == (roff[-1], 10)
    return cnt, roff, rows


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_batch(what, Ts, Cs, dt, truths, cnt, roff, rows, t0=None):
    """Counts against the restatement and the oracle, all ten columns against the truth."""
    assert cnt.dtype == np.int64 and cnt.tolist() == [len(t) for t in truths], what
    worst = np.zeros(3)
    for k, tr in enumerate(truths):
        if len(Ts[k]):  # (the oracle's sampler needs a segment)
            assert len(O.sample_traj(Ts[k], Cs[k], dt)) == cnt[k], (what, k)
        got = rows[roff[k]:roff[k] + cnt[k]]
        worst = np.maximum(worst, SR.assert_rows(got, tr, 0.0 if t0 is None else t0[k], (what, "track", k)))
    print(f"{what}: {int(cnt.sum())} rows, worst |got - truth| / bound per derivative order {worst.tolist()}")
    return worst


# ---- 1. fitted, ragged: all ten columns ---------------------------------------------------
def test_fitted_ragged_all_columns():
    Ts, Cs = _ragged()
    assert [len(T) for T in Ts] == list(SI.FIT_SEGS) + [130, 131]
    cnt, roff, rows = _ragged_rows()
    worst = _check_batch("ragged", Ts, Cs, DT, _ragged_truths(), cnt, roff, rows)
    assert (worst <= 1.0).all()


# ---- 2. per-track t0 ----------------------------------------------------------------------
def test_per_track_t0():
    Ts, Cs = _ragged()
    cnt, roff, plain = _ragged_rows()
    got = capi.sample_batch(Ts, Cs, DT, t0=SI.T0S)
    assert got.shape == plain.shape
    for k, tr in enumerate(_ragged_truths()):
        t = got[roff[k]:roff[k + 1], 9]
        exp = tr.time(SI.T0S[k])
        assert t.tobytes() == exp.tobytes(), (k, SI.T0S[k], t[:3], exp[:3])
    assert got[:, :9].tobytes() == plain[:, :9].tobytes()  # the value columns: not a bit
    zeros = capi.sample_batch(Ts, Cs, DT, t0=np.zeros(len(Ts)))
    assert zeros.tobytes() == plain.tobytes()  # t0 = NULL is t0 = 0.0


# ---- 3. scattered row offsets -------------------------------------------------------------
def _scatter(cnt, gap, spare, order):
    """(row offsets, buffer rows): the tracks in `order`, `gap` rows before each one and
    `spare` rows at both ends."""
    off = np.zeros(len(cnt), np.int64)
    pos = spare
    for k in order:
        pos += gap
        off[k] = pos
        pos += int(cnt[k])
    return off, pos + spare


def _assert_scattered(got, off, cnt, contig, croff):
    """Every track's rows are the contiguous call's and every other slot holds the fill."""
    owned = np.zeros(len(got), bool)
    for k in range(len(cnt)):
        a, b = int(off[k]), int(off[k] + cnt[k])
        assert not owned[a:b].any()
        owned[a:b] = True
        assert got[a:b].tobytes() == contig[croff[k]:croff[k + 1]].tobytes(), k
    outside = _u64(got)[~owned]
    assert (outside == np.uint64(SI.NAN_FILL)).all(), np.argwhere(outside != np.uint64(SI.NAN_FILL))[:4].tolist()
    return int((~owned).sum())


def test_scattered_row_offsets():
    Ts, Cs = _ragged()
    cnt, roff, plain = _ragged_rows()
    off, n_rows = _scatter(cnt, 3, 5, range(len(Ts) - 1, -1, -1))
    assert off[-1] == 8 and n_rows == cnt.sum() + 3 * len(Ts) + 10
    got = capi.sample_batch(Ts, Cs, DT, row_offsets=off, n_rows=n_rows, fill=SI.NAN_FILL)
    assert got.shape == (n_rows, 10)
    assert _assert_scattered(got, off, cnt, plain, roff) == 3 * len(Ts) + 10
    with pytest.raises(ValueError):  # (the wrapper refuses a layout that leaves the buffer)
        capi.sample_batch(Ts, Cs, DT, row_offsets=off, n_rows=n_rows - 6, fill=SI.NAN_FILL)


# ---- 4. chunk edges with every coefficient live -------------------------------------------
def test_chunk_edges_every_coefficient_live():
    Ts, Cs = SI.chunk_edges()
    truths = [SR.Truth(T, Cf, DT) for T, Cf in zip(Ts, Cs)]
    assert [len(t) for t in truths] == list(SI.CHUNK_ROWS)  # (on the restatement first)
    assert all((Cf != 0).all() for Cf in Cs)
    cnt = capi.sample_count(Ts, DT)
    roff = np.zeros(len(Ts) + 1, np.int64)
    roff[1:] = np.cumsum(cnt)
    rows = capi.sample_batch(Ts, Cs, DT)
    assert len(rows) == sum(SI.CHUNK_ROWS)
    worst = _check_batch("chunk edges", Ts, Cs, DT, truths, cnt, roff, rows)
    assert (worst <= 1.0).all()


# ---- 5. recurrence edges beside ordinary tracks, one launch -------------------------------
def test_recurrence_edges_beside_ordinary_tracks():
    fT, fC = _ragged()
    names, Ts, Cs = SI.recurrence_edges(fT, fC)
    dt = SI.EDGE_DT
    truths = [SR.Truth(T, Cf, dt) for T, Cf in zip(Ts, Cs)]
    want = {name: n for name, _, n in SI.EDGE_CASES}
    for name, tr in zip(names, truths):
        if name is None:
            assert len(tr) > 10
        elif want[name] is not None:
            assert len(tr) == want[name], name
        else:
            assert len(tr) > 1, name
    cnt = capi.sample_count(Ts, dt)
    off, n_rows = _scatter(cnt, 2, 2, range(len(Ts)))
    rows = capi.sample_batch(Ts, Cs, dt, row_offsets=off, n_rows=n_rows, fill=SI.NAN_FILL)
    worst = _check_batch("recurrence edges", Ts, Cs, dt, truths, cnt, np.append(off, n_rows), rows)
    assert (worst <= 1.0).all()
    # nothing is written for a track without rows, nor anywhere else outside the ranges
    owned = np.zeros(n_rows, bool)
    for k in range(len(Ts)):
        owned[off[k]:off[k] + cnt[k]] = True
    assert (_u64(rows)[~owned] == np.uint64(SI.NAN_FILL)).all()
    assert sorted(n for n, c in zip(names, cnt) if c == 0) == ["T all NaN", "T all zero", "one waypoint"]
    # the contiguous layout gives the same rows
    plain = capi.sample_batch(Ts, Cs, dt)
    assert plain.tobytes() == rows[owned].tobytes()


# ---- 6. the single-track path beside the batch --------------------------------------------
@pytest.mark.parametrize("case", range(len(SI.SINGLE_SEGS)))
def test_single_track_path_beside_the_batch(case):
    """generate_trajectory_times (k_refit: the refit inside the launch) against
    minsnap_batch_times + sample_batch on the same segment times.  The time column is ==.  The
    value columns are NOT == (see the module docstring): both fits are held to the truth of
    the batch's coefficients, the single-track rows with the coefficient distance the fits are
    allowed (1e-9, test_gpu_minsnap.py test_batch_vs_truth) carried through the acceleration
    column: 1e-9 * max(1, T_total)^2."""
    wp, T, v0, a0 = SI.single_problem()[case]
    assert len(T) == SI.SINGLE_SEGS[case]
    t0 = SI.SINGLE_T0
    single = capi.generate_trajectory_times(wp, T, DT, t0, v0, a0)
    Cb, st = capi.minsnap_batch_times([wp], [T], v0[None], a0[None])
    assert st[0] == 0
    batch = capi.sample_batch([T], Cb, DT, t0=[t0])
    assert single.shape == batch.shape and len(batch) == capi.sample_count([T], DT)[0]
    assert single[:, 9].tobytes() == batch[:, 9].tobytes()
    d = np.abs(single[:, :9] - batch[:, :9])
    print(f"{len(T)} segments: value columns equal: {np.array_equal(single[:, :9], batch[:, :9])}, "
          f"max |single - batch| {d.max()!r} at column {int(d.max(axis=0).argmax())}")
    tr = SR.Truth(T, Cb[0], DT)
    wb = SR.assert_rows(batch, tr, t0, "batch")
    extra = Fraction(1e-9) * Fraction(max(1.0, float(np.sum(T)))) ** 2
    ws = SR.assert_rows(single, tr, t0, "single", extra=extra, positions=False)
    print(f"worst error / bound: batch {wb.tolist()}, single (before the allowance) {ws.tolist()}")
    assert (wb <= 1.0).all()
