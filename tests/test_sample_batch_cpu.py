"""CPU: the row sampler's reference and inputs without the code under test, and the argument
checks of epp_sample_count / epp_sample_batch (they precede every device call).

1. On every input set of test_gpu_sample_batch.py (sample_batch_inputs.all_sets_cpu, the
   fitted tracks by the oracle's fit) the oracle's own rows (oracle.sample_traj, an unfused
   Horner) lie within sample_batch_ref's bound of the exact truth, and its row count and time
   column are the restated recurrence's.  No set needed more than the bound.
2. The bound bites: each of the four mistakes it is meant to reject (derivative order k + 1,
   the next segment's coefficients, the following row's tin, c_9 dropped) leaves it on at
   least one row of every fitted track.  "The next segment" needs a track of two segments,
   so the one-segment fit takes no part in that mutation alone.
"""
import functools
import re

import numpy as np
import pytest

import oracle as O
import sample_batch_inputs as SI
import sample_batch_ref as SR
from eppamd import capi

from conftest import PKG


@functools.lru_cache(maxsize=None)
def _sets():
    return SI.all_sets_cpu()


@functools.lru_cache(maxsize=None)
def _truths(name):
    for n, dt, Ts, Cs in _sets():
        if n == name:
            return dt, Ts, Cs, [SR.Truth(T, Cf, dt) for T, Cf in zip(Ts, Cs)]
    raise KeyError(name)


def test_inputs_are_what_they_are_meant_to_be():
    assert SI.K_ROW_CHUNK == int(re.search(r"kRowChunk = (\d+);",
                                           open(PKG + "/csrc/traj_sample.h").read()).group(1))
    for name, dt, Ts, Cs in _sets():
        for T, Cf in zip(Ts, Cs):
            assert np.shape(Cf) == (len(T), 3, 10)
            if len(T) and np.isfinite(T).all():
                assert np.sum(T) / dt <= 2e4  # (no small-dt probing)
    dt, Ts, Cs, tr = _truths("ragged")
    assert [len(T) for T in Ts] == list(SI.FIT_SEGS) + [130, 131] and len(SI.T0S) == len(Ts)
    rows = sum(len(t) for t in tr)
    print("ragged batch rows", rows)
    assert 5000 < rows < 7000
    dt, Ts, Cs, tr = _truths("chunk edges")
    assert [len(t) for t in tr] == list(SI.CHUNK_ROWS) == [1, 8, 9, 511, 512, 513, 1025]
    assert all((Cf != 0).all() for Cf in Cs)
    dt, Ts, Cs, tr = _truths("recurrence edges")
    for (name, T, want), t in zip(SI.EDGE_CASES, tr[::2]):
        if want is not None:
            assert len(t) == want, name
        else:
            assert len(t) > 1, name
    k = [c[0] for c in SI.EDGE_CASES].index("T exact multiples of dt")
    assert tr[2 * k].tac.tolist() == [0.25 * i for i in range(7)]  # t_end = 1.75 itself is no row
    k = [c[0] for c in SI.EDGE_CASES].index("three consecutive segments shorter than dt")
    assert not {1, 2, 3} <= set(tr[2 * k].seg.tolist())  # (a step jumps over at least one of them)
    for (wp, T, _, _), To in zip(SI.single_problem(), _truths("single track")[1]):
        assert np.array_equal(T, To)


@pytest.mark.parametrize("name", ["ragged", "chunk edges", "recurrence edges", "single track"])
def test_oracle_rows_within_the_bound_of_the_truth(name):
    dt, Ts, Cs, truths = _truths(name)
    worst = np.zeros(3)
    for k, (T, Cf, tr) in enumerate(zip(Ts, Cs, truths)):
        if len(T) == 0:  # (the oracle's sampler needs a segment)
            assert len(tr) == 0
            continue
        rows = O.sample_traj(T, Cf, dt, 0.0)
        # positions=False: the oracle's Horner is unfused, bits differ from the device's rule
        worst = np.maximum(worst, SR.assert_rows(rows, tr, 0.0, (name, k), positions=False))
        if len(rows):
            t0 = 3.25
            assert np.array_equal(O.sample_traj(T, Cf, dt, t0)[:, 9], tr.time(t0))
    print(name, "oracle worst |got - truth| / bound per derivative", worst.tolist())
    assert (worst <= 1.0).all()


@pytest.mark.parametrize("kind", SR.MUTATIONS)
def test_the_bound_rejects_each_mistake_on_every_fitted_track(kind):
    dt, Ts, Cs, truths = _truths("ragged")
    tried = 0
    for k, tr in enumerate(truths):
        if kind == "segment" and len(Ts[k]) < 2:
            continue
        assert SR.mutation_rejected(tr, kind), (kind, "track", k, len(Ts[k]), "segments")
        tried += 1
    assert tried >= len(truths) - 1


def test_reference_evaluation_by_hand():
    """p = 1 + 2 t + 3 t^2 at t = 0.5: 2.75, p' = 5, p'' = 6; S with a negative coefficient."""
    c = np.zeros(10)
    c[:3] = (1.0, -2.0, 3.0)
    assert SR.exact(c, 0.5, 0) == (0.75, 2.75)
    assert SR.exact(c, 0.5, 1) == (1.0, 5.0)
    assert SR.exact(c, 0.5, 2) == (6.0, 6.0)
    assert SR.exact(c, 0.5, 3) == (0, 0)
    c[9] = 2.0
    assert SR.exact(c, 2.0, 2)[0] == 6 + 72 * 2.0 * 2.0 ** 7
    assert SR.exact(c, 2.0, 2, skip=(9,))[0] == 6
    quad = c * (np.arange(10) < 3)  # the bound there: 32 * 2^-53 * 2.75 = 2^-46.54
    assert SR.within(0.75 + 2 ** -47, *SR.exact(quad, 0.5, 0))
    assert not SR.within(0.75 + 2 ** -46, *SR.exact(quad, 0.5, 0))


def test_symbols_and_argument_checks():
    L = capi.lib()
    for name in ("epp_sample_count", "epp_sample_batch"):
        assert hasattr(L, name) and name in capi.EXPORTED
    # stand-ins for device pointers: every case below is rejected before anything is read
    buf = np.zeros(64)
    p = buf.ctypes.data
    count = {
        "n_tracks < 0": (p, p, -1, 0.1, p),
        "NULL seg_times": (None, p, 1, 0.1, p),
        "NULL wp_offsets": (p, None, 1, 0.1, p),
        "NULL row_counts": (p, p, 1, 0.1, None),
    }
    for name, (T, off, n, dt, cnt) in count.items():
        assert L.epp_sample_count(T, off, n, dt, cnt, None) == capi.EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_sample_count" in L.epp_last_error(), name
    batch = {
        "n_tracks < 0": (p, p, p, -1, 0.1, None, p, p),
        "NULL seg_times": (None, p, p, 1, 0.1, None, p, p),
        "NULL coeffs": (p, None, p, 1, 0.1, None, p, p),
        "NULL wp_offsets": (p, p, None, 1, 0.1, p, p, p),
        "NULL row_offsets": (p, p, p, 1, 0.1, None, None, p),
        "NULL rows": (p, p, p, 1, 0.1, p, p, None),
    }
    for name, (T, Cf, off, n, dt, t0, roff, rows) in batch.items():
        assert L.epp_sample_batch(T, Cf, off, n, dt, t0, roff, rows, None) == capi.EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_sample_batch" in L.epp_last_error(), name
    # an empty batch is fine, with or without buffers, and launches nothing
    assert L.epp_sample_count(None, None, 0, 0.1, None, None) == capi.EPP_OK
    assert L.epp_sample_count(p, p, 0, 0.1, p, None) == capi.EPP_OK
    assert L.epp_sample_batch(None, None, None, 0, 0.1, None, None, None, None) == capi.EPP_OK
    assert L.epp_sample_batch(p, p, p, 0, 0.1, p, p, p, None) == capi.EPP_OK
