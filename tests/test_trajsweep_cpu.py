"""CPU: epp_traj_sweep_batch's argument checks (they precede every device call, so they run
without a GPU), its symbol, wrapper and compiled resources, and the fixtures of the GPU test
(trajsweep_inputs.py) checked with the oracle alone: the straight-line tracks put their only
failing chord where they claim, and the thin-box track has every row valid and one chord not."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import trajsweep_inputs as tsi
from eppamd import capi
from test_kernel_resources import LLVM, _kernel_metadata

EPP_ERR_INVALID_ARGUMENT = -1


def _call(world, T, Cf, off, n, dt, rows, cp=0, times=None):
    return capi.lib().epp_traj_sweep_batch(world, T, Cf, off, n, dt, cp, rows, times, None)


def test_symbol_wrapper_and_argument_checks():
    L = capi.lib()
    assert hasattr(L, "epp_traj_sweep_batch") and "epp_traj_sweep_batch" in capi.EXPORTED
    assert callable(capi.World.sweep_trajectories)
    # stand-ins for device pointers: every case below is rejected before anything is read
    buf = np.zeros(64)
    p = buf.ctypes.data
    world = C.c_void_p(p)  # (a non-NULL handle; never dereferenced by a rejected call)
    cases = {
        "NULL world": (None, p, p, p, 1, 0.05, p, 0),
        "n_tracks < 0": (world, p, p, p, -1, 0.05, p, 0),
        "dt == 0": (world, p, p, p, 1, 0.0, p, 0),
        "dt < 0": (world, p, p, p, 1, -0.05, p, 0),
        "dt NaN": (world, p, p, p, 1, float("nan"), p, 0),
        "dt inf": (world, p, p, p, 1, float("inf"), p, 0),
        "can_pass_gate 2": (world, p, p, p, 1, 0.05, p, 2),
        "can_pass_gate -1": (world, p, p, p, 1, 0.05, p, -1),
        "NULL seg_times": (world, None, p, p, 1, 0.05, p, 0),
        "NULL coeffs": (world, p, None, p, 1, 0.05, p, 1),
        "NULL wp_offsets": (world, p, p, None, 1, 0.05, p, 0),
        "NULL first_invalid": (world, p, p, p, 1, 0.05, None, 1),
    }
    for name, (w, T, Cf, off, n, dt, rows, cp) in cases.items():
        rc = _call(w, T, Cf, off, n, dt, rows, cp)
        assert rc == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_traj_sweep_batch" in L.epp_last_error(), name
    # an empty batch is fine, with or without buffers, and launches nothing
    assert _call(world, None, None, None, 0, 0.05, None) == capi.EPP_OK
    assert _call(world, p, p, p, 0, 0.05, p, cp=1, times=p) == capi.EPP_OK


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="ROCm LLVM tools absent")
def test_kernel_keeps_everything_in_registers():
    every = _kernel_metadata(capi.LIB_PATH)
    # k_traj_sweep: the three staging levels; k_traj_check: front staged or not
    for kernel, variants in (("k_traj_sweep", 3), ("k_traj_check", 2)):
        meta = {k: v for k, v in every.items() if kernel in k}
        assert len(meta) == variants, sorted(meta)
        for name, v in meta.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (name, v)
            # 4 waves per SIMD: the 8 two-wave workgroups per CU the launcher's grid counts on
            assert 0 < v["vgpr_count"] <= 128, (name, v)


def test_edge_fixtures_fail_where_they_claim():
    names, Ts, Cs, want = tsi.edge_tracks()
    ref = tsi.thin_ref()
    for cp in tsi.CAN_PASS:
        first, time, robust, n_rows = tsi.oracle_sweep(ref, Ts, Cs, tsi.DT, cp)
        assert robust.all()
        assert first.tolist() == want, list(zip(names, first.tolist(), want))
        assert ((first == -1) == (time == -1.0)).all()
    rows = dict(zip(names, n_rows.tolist()))
    assert rows["1 row"] == 1 and rows["2 rows"] == 2 and rows["513 rows, last chord"] == 513
    assert rows["513 rows, valid"] == 513 and rows["512 rows, valid"] == 512
    assert rows["chunk boundary 1023|1024"] >= 1026 and rows["segment boundary 5|6"] == 16
    # the segment-boundary chord's ends come from different polynomials
    k = names.index("segment boundary 5|6")
    T = Ts[k]
    t = O.sample_traj(T, Cs[k], tsi.DT)[:, 9]
    assert t[5] <= T[0] < t[6]
    # each failing track fails in exactly one chord: every other chord passes on its own
    _, rg, ro = tsi.spi.setup()
    for k, w in enumerate(want):
        if w < 0:
            continue
        xyz = O.sample_traj(Ts[k], Cs[k], tsi.DT)[:, [0, 3, 6]]
        f = O.check_motions(ref, rg, ro, xyz[:-1], xyz[1:], False, 0)
        assert np.flatnonzero(f == 0).tolist() == [w], names[k]


def test_thin_box_fixture_rows_valid_one_chord_invalid():
    Ts, Cs, chord = tsi.thin_track()
    ref = tsi.thin_ref()
    _, rg, ro = tsi.spi.setup()
    rows = O.sample_traj(Ts[0], Cs[0], tsi.DT)
    xyz = rows[:, [0, 3, 6]]
    assert len(rows) == 20
    # thinner than the row spacing, every row outside the inflated extent
    o = ref[0]
    assert 2 * (o["half"][0] + ro) < tsi.STEP
    assert (np.abs(xyz[:, 0] - o["center"][0]) > o["half"][0] + ro + 0.1).all()
    for md in (0.0, 0.1, ro):
        assert O.check_states_mindist(ref, xyz, md).all()
    for cp in tsi.CAN_PASS:
        assert O.check_states(ref, rg, ro, xyz, cp).all()
        f = O.check_motions(ref, rg, ro, xyz[:-1], xyz[1:], cp, 0)
        assert np.flatnonzero(f == 0).tolist() == [chord]
