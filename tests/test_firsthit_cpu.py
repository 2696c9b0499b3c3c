"""CPU: the argument checks of epp_motions_first_hit and epp_traj_first_hit_batch (they precede
every device call, so they run without a GPU), their symbols and wrappers, and hand values for
the restatement of the definition (firsthit_ref.py) the GPU tests compare against."""
import ctypes as C

import numpy as np

import firsthit_ref as fr
from eppamd import capi

EPP_ERR_INVALID_ARGUMENT = -1


def test_symbols_wrappers_and_argument_checks():
    L = capi.lib()
    for name in ("epp_motions_first_hit", "epp_traj_first_hit_batch"):
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.World.first_hits) and callable(capi.World.trajectory_first_hits)
    # stand-ins for device pointers: every case below is rejected before anything is read
    buf = np.zeros(64)
    p = buf.ctypes.data
    world = C.c_void_p(p)  # (a non-NULL handle; never dereferenced by a rejected call)
    motions = {
        "NULL world": (None, p, p, 1, 0, p),
        "n < 0": (world, p, p, -1, 0, p),
        "can_pass_gate 2": (world, p, p, 1, 2, p),
        "can_pass_gate -1": (world, p, p, 1, -1, p),
        "NULL s1": (world, None, p, 1, 0, p),
        "NULL s2": (world, p, None, 1, 1, p),
        "NULL t_hit": (world, p, p, 1, 0, None),
    }
    for name, (w, s1, s2, n, cp, t) in motions.items():
        assert L.epp_motions_first_hit(w, s1, s2, n, cp, t, p, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_motions_first_hit" in L.epp_last_error(), name
    assert L.epp_motions_first_hit(world, None, None, 0, 0, None, None, None) == capi.EPP_OK  # launches nothing
    assert L.epp_motions_first_hit(world, p, p, 0, 1, p, p, None) == capi.EPP_OK
    tracks = {
        "NULL world": (None, p, p, p, 1, 0.05, 0, p, p),
        "n_tracks < 0": (world, p, p, p, -1, 0.05, 0, p, p),
        "dt == 0": (world, p, p, p, 1, 0.0, 0, p, p),
        "dt < 0": (world, p, p, p, 1, -0.05, 0, p, p),
        "dt NaN": (world, p, p, p, 1, float("nan"), 0, p, p),
        "dt inf": (world, p, p, p, 1, float("inf"), 0, p, p),
        "can_pass_gate 2": (world, p, p, p, 1, 0.05, 2, p, p),
        "can_pass_gate -1": (world, p, p, p, 1, 0.05, -1, p, p),
        "NULL seg_times": (world, None, p, p, 1, 0.05, 0, p, p),
        "NULL coeffs": (world, p, None, p, 1, 0.05, 0, p, p),
        "NULL wp_offsets": (world, p, p, None, 1, 0.05, 1, p, p),
        "NULL chord": (world, p, p, p, 1, 0.05, 0, None, p),
        "NULL t_hit": (world, p, p, p, 1, 0.05, 0, p, None),
    }
    for name, (w, T, Cf, off, n, dt, cp, chord, t) in tracks.items():
        assert L.epp_traj_first_hit_batch(w, T, Cf, off, n, dt, cp, chord, t, p, p, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_traj_first_hit_batch" in L.epp_last_error(), name
    assert L.epp_traj_first_hit_batch(world, None, None, None, 0, 0.05, 0, None, None, None, None, None) == capi.EPP_OK
    assert L.epp_traj_first_hit_batch(world, p, p, p, 0, 0.05, 1, p, p, p, p, None) == capi.EPP_OK


def _box(center, half, yaw=0.0, filling=0, is_gate=0):
    o = np.zeros(1, capi.OBB_DTYPE)
    o["center"], o["half"], o["filling"], o["is_gate"] = center, half, filling, is_gate
    c, s = np.cos(yaw), np.sin(yaw)
    o["rot"] = [c, -s, 0, s, c, 0, 0, 0, 1]
    return o


RG, RO = 0.5, 0.25


def _both(obbs, s, e, can_pass=False):
    """(t, obb) of one edge from the scalar and the numpy form, which must agree."""
    w = fr.world(obbs, RG, RO)
    t, o = fr.first_hit(w, RG, RO, list(s), list(e), can_pass)
    tv, ov = fr.edges(w, RG, RO, [s], [e], can_pass)
    assert tv[0] == t and ov[0] == o
    m = fr.matrices(w, RG, RO, [s], [e], can_pass)
    tm, om = fr.reduce_min(m["t"])
    assert tm[0] == t and om[0] == o
    return t, o


def test_restatement_hand_values():
    unit = _box([0, 0, 0], [0.5, 0.5, 0.5])  # an obstacle's box: inflated by RO, 0.75 to a face
    w = fr.world(unit, RG, RO)
    assert w[0]["aabb_lo"] == [-0.75] * 3 and w[0]["aabb_hi"] == [0.75] * 3
    # a start inside the box gives 0, wherever the edge goes
    assert _both(unit, [0.1, 0.2, -0.3], [3.0, 0.0, 0.0]) == (0.0, 0)
    assert _both(unit, [0.7, 0.0, 0.0], [3.0, 0.0, 0.0]) == (0.0, 0)  # inside the inflated box only
    # a straight hit: from x = -2.75 to x = 1.25 (length 4), the face at -0.75: t = 2 / 4
    assert _both(unit, [-2.75, 0.0, 0.0], [1.25, 0.0, 0.0]) == (0.5, 0)
    # ... and by the operations: invD = 1 / 4, t1 = (-0.75 + 2.75) * 0.25
    assert _both(unit, [-2.75, 0.1, 0.2], [1.25, 0.1, 0.2]) == ((-0.75 - -2.75) * (1.0 / 4.0), 0)
    # a miss beside the box, inside its AABB's reach along x only; and one that the prefilter drops
    assert _both(unit, [-2.0, 1.0, 0.0], [2.0, 1.0, 0.0]) == (np.inf, -1)
    assert _both(unit, [5.0, 5.0, 5.0], [6.0, 5.0, 5.0]) == (np.inf, -1)
    # the edge stops short of the face: tMin = 2 / 1.5 > 1
    assert _both(unit, [-2.75, 0.0, 0.0], [-1.25, 0.0, 0.0]) == (np.inf, -1)
    # end-only through the parallel branch: |d_x| = 9e-7 < 1e-6, the start outside the face
    t, o = _both(unit, [0.75 + 5e-7, 0.0, 0.0], [0.75 - 4e-7, 0.0, 0.0])
    assert (t, o) == (1.0, 0)
    m = fr.matrices(w, RG, RO, [[0.75 + 5e-7, 0.0, 0.0]], [[0.75 - 4e-7, 0.0, 0.0]], False)
    assert (m["start"][0, 0], m["slab"][0, 0], m["end"][0, 0]) == (False, False, True)
    # zero-length edges
    assert _both(unit, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]) == (0.0, 0)
    assert _both(unit, [2.0, 0.0, 0.0], [2.0, 0.0, 0.0]) == (np.inf, -1)
    # two boxes in a row, the lower index the farther one: the minimum wins, not the first
    row = np.concatenate([_box([4.0, 0, 0], [0.5, 0.5, 0.5]), _box([0.0, 0, 0], [0.5, 0.5, 0.5])])
    assert _both(row, [-2.75, 0.0, 0.0], [5.25, 0.0, 0.0]) == (0.25, 1)
    assert _both(row, [5.25, 0.0, 0.0], [-2.75, 0.0, 0.0]) == (0.0625, 0)  # (0.5 / 8 from the other side)
    # the same box twice: the lower index wins the tie
    twice = np.concatenate([_box([9.0, 9.0, 9.0], [0.1, 0.1, 0.1]), unit, unit])
    assert _both(twice, [-2.75, 0.0, 0.0], [1.25, 0.0, 0.0]) == (0.5, 1)
    # a gate's box is inflated by RG: the face at -1.0, t = 1.75 / 4
    gate = _box([0, 0, 0], [0.5, 0.5, 0.5], is_gate=1)
    assert _both(gate, [-2.75, 0.0, 0.0], [1.25, 0.0, 0.0]) == (0.4375, 0)
    # a filling box: skipped with can_pass, else its slab is inflated but its endpoint tests are not
    fill = _box([0, 0, 0], [0.5, 0.5, 0.5], filling=1, is_gate=1)
    assert _both(fill, [-2.75, 0.0, 0.0], [1.25, 0.0, 0.0], True) == (np.inf, -1)
    assert _both(fill, [-2.75, 0.0, 0.0], [1.25, 0.0, 0.0], False) == (0.4375, 0)
    assert _both(fill, [0.7, 0.0, 0.0], [-3.0, 0.0, 0.0], False) == (0.0, 0)  # tMin = 0: the slab, not the start
    m = fr.matrices(fr.world(fill, RG, RO), RG, RO, [[0.7, 0.0, 0.0]], [[-3.0, 0.0, 0.0]], False)
    assert (m["start"][0, 0], m["slab"][0, 0]) == (False, True)
    # (its AABB is not inflated either: the same start, leaving the box, is dropped by the prefilter)
    assert _both(fill, [0.7, 0.0, 0.0], [3.0, 0.0, 0.0], False) == (np.inf, -1)
    # yaw pi / 2: the long side lies along y
    bar = _box([0, 0, 0], [2.0, 0.25, 0.25], np.pi / 2)
    assert _both(bar, [-2.5, 1.5, 0.0], [1.5, 1.5, 0.0])[0] == 0.5  # the face at x = -(0.25 + RO)
    # no OBB at all
    assert _both(unit[:0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]) == (np.inf, -1)
