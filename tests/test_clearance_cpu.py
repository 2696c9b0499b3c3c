"""CPU: the argument checks of epp_states_clearance and epp_traj_clearance_batch (they precede
every device call, so they run without a GPU), their symbols and wrappers, and hand values for
the numpy restatement of the definition (clearance_ref.py) the GPU tests compare against."""
import ctypes as C

import numpy as np

import clearance_ref as cr
from eppamd import capi

EPP_ERR_INVALID_ARGUMENT = -1


def test_symbols_wrappers_and_argument_checks():
    L = capi.lib()
    for name in ("epp_states_clearance", "epp_traj_clearance_batch"):
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.World.clearance) and callable(capi.World.trajectory_clearance)
    # stand-ins for device pointers: every case below is rejected before anything is read
    buf = np.zeros(64)
    p = buf.ctypes.data
    world = C.c_void_p(p)  # (a non-NULL handle; never dereferenced by a rejected call)
    states = {
        "NULL world": (None, p, 1, p, p),
        "n < 0": (world, p, -1, p, p),
        "NULL xyz": (world, None, 1, p, p),
        "NULL dist": (world, p, 1, None, p),
    }
    for name, (w, xyz, n, dist, near) in states.items():
        assert L.epp_states_clearance(w, xyz, n, dist, near, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_states_clearance" in L.epp_last_error(), name
    assert L.epp_states_clearance(world, None, 0, None, None, None) == capi.EPP_OK  # launches nothing
    assert L.epp_states_clearance(world, p, 0, p, p, None) == capi.EPP_OK
    tracks = {
        "NULL world": (None, p, p, p, 1, 0.05, p),
        "n_tracks < 0": (world, p, p, p, -1, 0.05, p),
        "dt == 0": (world, p, p, p, 1, 0.0, p),
        "dt < 0": (world, p, p, p, 1, -0.05, p),
        "dt NaN": (world, p, p, p, 1, float("nan"), p),
        "dt inf": (world, p, p, p, 1, float("inf"), p),
        "NULL seg_times": (world, None, p, p, 1, 0.05, p),
        "NULL coeffs": (world, p, None, p, 1, 0.05, p),
        "NULL wp_offsets": (world, p, p, None, 1, 0.05, p),
        "NULL clearance": (world, p, p, p, 1, 0.05, None),
    }
    for name, (w, T, Cf, off, n, dt, clr) in tracks.items():
        assert L.epp_traj_clearance_batch(w, T, Cf, off, n, dt, clr, p, p, p, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_traj_clearance_batch" in L.epp_last_error(), name
    assert L.epp_traj_clearance_batch(world, None, None, None, 0, 0.05, None, None, None, None, None) == capi.EPP_OK
    assert L.epp_traj_clearance_batch(world, p, p, p, 0, 0.05, p, p, p, p, None) == capi.EPP_OK


def _box(center, half, yaw, filling=0):
    o = np.zeros(1, capi.OBB_DTYPE)
    o["center"], o["half"], o["filling"] = center, half, filling
    c, s = np.cos(yaw), np.sin(yaw)
    o["rot"] = [c, -s, 0, s, c, 0, 0, 0, 1]
    return o


def test_restatement_hand_values():
    unit = _box([0, 0, 0], [0.5, 0.5, 0.5], 0.0)
    pts = np.array([[2.0, 0.0, 0.0],    # off a face: 1.5
                    [2.0, 2.5, 0.25],   # off an edge: (1.5, 2.0) -> 2.5
                    [1.5, 2.5, 2.5],    # off a corner: (1, 2, 2) -> 3
                    [0.25, -0.5, 0.1],  # inside / on a face: 0
                    [np.nan, 0.0, 0.0]])
    d2, near = cr.states(unit, pts)
    assert np.array_equal(np.sqrt(d2), [1.5, 2.5, 3.0, 0.0, np.inf]) and near.tolist() == [0, 0, 0, 0, -1]
    # yaw pi/4: the local axes are the diagonals
    q = _box([1.0, 1.0, 0.0], [0.5, 0.5, 0.5], np.pi / 4)
    r = np.sqrt(0.5)
    pts = np.array([[1.0 + 2 * r, 1.0 + 2 * r, 0.0],   # along local x: 2 - 0.5
                    [1.0, 1.0 + 2 * r * 2, 0.0],       # local (2, 2, 0): an edge, 1.5 sqrt 2
                    [1.0, 1.0 + 2 * r * 2, 2.0],       # local (2, 2, 2): a corner, 1.5 sqrt 3
                    [1.0 + 0.2 * r, 1.0, 0.3]])        # inside
    d2, near = cr.states(q, pts)
    assert np.allclose(np.sqrt(d2), [1.5, 1.5 * np.sqrt(2), 1.5 * np.sqrt(3), 0.0], rtol=0, atol=1e-14)
    assert d2[3] == 0.0 and near.tolist() == [0, 0, 0, 0]
    # a filling box is ignored, alone and before a collision box
    fill = _box([0, 0, 0], [0.5, 0.5, 0.5], 0.0, filling=1)
    d2, near = cr.states(fill, [[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    assert np.isinf(d2).all() and near.tolist() == [-1, -1]
    both = np.concatenate([fill, _box([4.0, 0, 0], [0.5, 0.5, 0.5], 0.0)])
    d2, near = cr.states(both, [[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    assert np.array_equal(np.sqrt(d2), [3.5, 0.5]) and near.tolist() == [1, 1]
    # a tie between two mirror-image boxes goes to the lower index
    pair = np.concatenate([_box([-2.0, 0, 0], [0.5, 0.5, 0.5], 0.0), _box([2.0, 0, 0], [0.5, 0.5, 0.5], 0.0)])
    d2, near = cr.states(pair, [[0.0, 0.3, 0.0], [0.25, 0.0, 0.0]])
    assert np.array_equal(np.sqrt(d2), [1.5, 1.25]) and near.tolist() == [0, 1]
    # no OBB at all
    d2, near = cr.states(pair[:0], [[0.0, 0.0, 0.0]])
    assert np.isinf(d2).all() and near.tolist() == [-1]


def test_restatement_rows_and_track_minimum():
    # x = -1 + t over 2 s at dt 0.5: rows at t = 0, .5, 1, 1.5 (and 2.0 is not < t_end)
    Cf = np.zeros((1, 3, 10))
    Cf[0, 0, :2] = (-1.0, 1.0)
    xyz, time = cr.sample_rows(np.array([2.0]), Cf, 0.5)
    assert time.tolist() == [0.0, 0.5, 1.0, 1.5] and xyz[:, 0].tolist() == [-1.0, -0.5, 0.0, 0.5]
    unit = _box([0, 0, 0], [0.5, 0.5, 0.5], 0.0)
    d2, row, t, near = cr.tracks(unit, [np.array([2.0])], [Cf], 0.5)
    # rows 1, 2 and 3 are inside or on the box: the earliest wins
    assert (d2[0], row[0], t[0], near[0]) == (0.0, 1, 0.5, 0)
    e = 2.0 ** -30
    assert (1.0 + e) * (1.0 - e) - 1.0 == 0.0 and cr.fma(1.0 + e, 1.0 - e, -1.0) == -(2.0 ** -60)  # (one rounding)
    assert cr.track_from_rows(np.zeros(0), np.zeros(0, np.int32), np.zeros(0)) == (np.inf, -1, -1.0, -1)
    assert cr.ulps(np.array([1.0, np.inf]), np.array([np.nextafter(1.0, 2.0), np.inf])).tolist() == [1.0, 0.0]
