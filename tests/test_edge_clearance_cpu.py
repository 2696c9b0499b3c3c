"""CPU: the numpy restatement of "edge clearance" (edge_clearance_ref.py, which the GPU tests
compare with bit for bit) against an independent truth, its two bit-exact consequences, hand
cases, and the argument checks of epp_motions_clearance and epp_traj_chord_clearance_batch
(they precede every device call, so they run without a GPU), their symbols and wrappers.

The tolerance is on d2, not on the distance (near zero the square root turns a 1e-14 error
of d2 into 1e-7 of the distance), and scaled by the size of the coordinates: an edge's scale
is max(1, L^2), L the largest coordinate difference between one of its endpoints and the
centre of its nearest box (the inputs reach 50 m from the boxes).  MEASURED is the restatement's
worst |d2 - truth| / scale over the committed inputs (worlds "1" and "T+1" of
edge_clearance_inputs.py, 257 edges each), BOUND four times that: headroom for new seeds, not
for the GPU, which must match the restatement exactly.
"""
import ctypes as C

import numpy as np

import clearance_ref as cr
import edge_clearance_inputs as ei
import edge_clearance_ref as er
from eppamd import capi

EPP_ERR_INVALID_ARGUMENT = -1
MEASURED = 5.04e-16
BOUND = 4 * MEASURED


def scale(obbs, s1, s2, near):
    """max(1, L^2) per edge; 1 where there is no nearest box."""
    c = obbs["center"][np.maximum(near, 0)] if len(obbs) else np.zeros((len(s1), 3))
    L = np.maximum(np.abs(s1 - c).max(axis=1), np.abs(s2 - c).max(axis=1))
    return np.where(near >= 0, np.maximum(1.0, L * L), 1.0)


def test_restatement_against_truth():
    worst = 0.0
    for name in ("1", "T+1"):
        ob = ei.obbs(name)
        s1, s2 = ei.edges(name, ei.BLOCK + 1)
        d2, t, near = ei.expected(name, ei.BLOCK + 1)
        fin = er.finite_edges(s1, s2)
        assert (~fin).sum() == ei.N_BAD
        assert np.isinf(d2[~fin]).all() and (t[~fin] == -1.0).all() and (near[~fin] == -1).all()
        assert np.isfinite(d2[fin]).all() and (near[fin] >= 0).all() and ((t[fin] >= 0) & (t[fin] <= 1)).all()
        truth = er.truth(ob, s1[fin], s2[fin], iters=120)
        err = np.abs(d2[fin].astype(np.longdouble) - truth).astype(np.float64)
        rel = err / scale(ob, s1[fin], s2[fin], near[fin])
        k = int(np.argmax(rel))
        print(f"{name}: worst |d2 - truth| {err.max():.3e}, scaled {rel.max():.3e} (d2 {d2[fin][k]:.6g}, t {t[fin][k]:.6g});"
              f" zero {int((d2 == 0).sum())}, inner t {int(((t > 0) & (t < 1)).sum())}")
        assert (rel <= BOUND).all()
        worst = max(worst, float(rel.max()))
        assert (d2 == 0).sum() >= 4 and ((t > 0) & (t < 1)).sum() >= 32  # (every kind of candidate wins somewhere)
    print(f"worst scaled error {worst:.4e}, MEASURED {MEASURED:.4e}, BOUND {BOUND:.4e}")
    assert worst <= MEASURED  # (the committed inputs: the figure quoted in DESIGN.md)


def test_bit_exact_consequences():
    for name in ("1", "T+1", "filling", "0"):
        ob = ei.obbs(name)
        s1, s2 = ei.edges(name, ei.BLOCK + 1)
        d2, t, near = ei.expected(name, ei.BLOCK + 1)
        fin = er.finite_edges(s1, s2)
        ds, de = cr.states(ob, s1)[0], cr.states(ob, s2)[0]
        assert (d2[fin] <= np.minimum(ds, de)[fin]).all()
        for p in (s1, s2):  # a zero-length edge is its point
            z2, zt, zn = er.edges(ob, p, p)
            p2, pn = cr.states(ob, p)
            ok = np.isfinite(p).all(axis=1)
            assert z2[ok].tobytes() == p2[ok].tobytes() and np.array_equal(zn[ok], pn[ok])
            assert (zt[ok & (zn >= 0)] == 0.0).all()
            assert np.isinf(z2[~ok]).all() and (zn[~ok] == -1).all() and (zt[~ok] == -1.0).all()
        if name in ("filling", "0"):
            assert np.isinf(d2).all() and (t == -1.0).all() and (near == -1).all()


def _one(ob, s, e):
    d2, t, near = er.edges(ob, np.array([s], float), np.array([e], float))
    return float(d2[0]), float(t[0]), int(near[0])


def test_hand_cases():
    box = ei.unit_box((0.5, 0.25, 1.0))
    assert _one(box, [0.1, 0.0, 0.0], [2.0, 0.0, 0.0]) == (0.0, 0.0, 0)       # the start inside
    assert _one(box, [2.0, 0.0, 0.0], [0.5, 0.25, -1.0]) == (0.0, 1.0, 0)     # the end on a corner
    d2, t, near = _one(box, [-2.0, 0.1, 0.0], [2.0, -0.1, 0.2])               # through, both ends outside
    assert 0.0 <= d2 <= BOUND * 4.0 and 0.0 < t < 1.0 and near == 0
    d2, t, near = _one(box, [-2.0, 1.25, 0.5], [3.0, 1.25, 0.5])              # parallel to x, 1 m off the face y
    assert d2 == 1.0 and 0.3 - 1e-12 <= t <= 0.5 + 1e-12
    d2, t, near = _one(box, [0.75, 0.0, -3.0], [0.75, 0.0, 3.0])              # parallel to z, 0.25 m off the face x
    assert d2 == 0.0625 and 1.0 / 3 - 1e-12 <= t <= 2.0 / 3 + 1e-12
    d2, t, near = _one(box, [-2.0, 0.1, 1.0], [2.0, 0.1, 1.0])                # in the face plane z = +h
    assert 0.0 <= d2 <= BOUND * 4.0 and 0.0 < t < 1.0
    d2, t, near = _one(box, [-2.0, 0.1, 1.5], [2.0, 0.1, 1.5])                # in a plane 0.5 above it
    assert d2 == 0.25
    d2, t, near = _one(box, [1.0, -0.25, 0.0], [0.0, 0.75, 0.0])              # grazes the edge x = y = +h
    assert 0.0 <= d2 <= BOUND * 1.0 and abs(t - 0.5) < 1e-9
    d2, t, near = _one(box, [1.1, -0.25, 0.0], [0.1, 0.75, 0.0])              # passes it 0.1 / sqrt 2 off
    assert abs(d2 - 0.005) <= BOUND * 1.21 and abs(t - 0.55) < 1e-9
    d2, t, near = _one(box, [1.5, 1.25, 2.0], [1.5, 1.25, 2.0])               # zero length, off a vertex
    assert (d2, t, near) == (3.0, 0.0, 0)
    d2, t, near = _one(box, [3.0, 0.0, 0.0], [2.0, 0.0, 0.0])                 # points at the box, stops short
    assert (d2, t, near) == (2.25, 1.0, 0)
    # NaN and infinite endpoints take part in nothing, whichever end and axis
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = [0.1, 0.0, 0.0]
            p[k] = bad
            assert _one(box, p, [2.0, 0.0, 0.0]) == (np.inf, -1.0, -1)
            assert _one(box, [2.0, 0.0, 0.0], p) == (np.inf, -1.0, -1)
    # a filling box is ignored, alone and before a collision box
    fill = ei.unit_box((0.5, 0.25, 1.0), filling=1)
    assert _one(fill, [0.1, 0.0, 0.0], [2.0, 0.0, 0.0]) == (np.inf, -1.0, -1)
    far = ei.unit_box((0.5, 0.5, 0.5))
    far["center"][0] = [4.0, 0.0, 0.0]
    assert _one(np.concatenate([fill, far]), [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]) == (0.25, 1.0, 1)
    # a tie between two mirror-image boxes goes to the lower index
    left = ei.unit_box((0.5, 0.5, 0.5))
    left["center"][0] = [-4.0, 0.0, 0.0]
    assert _one(np.concatenate([left, far]), [-3.0, 0.3, 0.0], [3.0, 0.3, 0.0]) == (0.25, 0.0, 0)
    assert _one(box[:0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]) == (np.inf, -1.0, -1)  # no OBB at all


def test_hand_cases_against_truth():
    box = ei.unit_box((0.5, 0.25, 1.0))
    box["rot"][0] = [np.cos(0.7), -np.sin(0.7), 0, np.sin(0.7), np.cos(0.7), 0, 0, 0, 1]
    rs = np.random.RandomState(77)
    s1, s2 = rs.uniform(-3, 3, (4000, 3)), rs.uniform(-3, 3, (4000, 3))
    s2[:500, 0] = s1[:500, 0]                       # in planes of constant world x, y, z
    s2[500:1000, 2] = s1[500:1000, 2]
    s2[1000:1200] = s1[1000:1200]                   # zero length
    s1[1200:1400, 2] = s2[1200:1400, 2] = 1.0       # in the face plane z = +h
    d2, t, near = er.edges(box, s1, s2)
    truth = er.truth(box, s1, s2, iters=120)
    err = np.abs(d2.astype(np.longdouble) - truth).astype(np.float64) / scale(box, s1, s2, near)
    print(f"4000 random and degenerate edges: worst scaled |d2 - truth| {err.max():.3e}")
    assert (err <= BOUND).all()


def test_track_minimum_prefers_the_earliest_chord():
    d = np.array([2.0, 1.0, np.nan, 1.0, 3.0])
    t = np.array([0.0, 0.25, -1.0, 0.5, 1.0])
    time = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5])
    near = np.array([4, 5, -1, 6, 7], np.int32)
    assert er.chords_min(d, t, near, time) == (1.0, 1, 0.25, 0.1 + 0.25 * (0.2 - 0.1), 5)
    assert er.chords_min(np.full(2, np.inf), np.full(2, -1.0), np.full(2, -1), np.zeros(3)) == (np.inf, -1, -1.0, -1.0, -1)
    assert er.chords_min(np.zeros(0), np.zeros(0), np.zeros(0, np.int32), np.zeros(1)) == (np.inf, -1, -1.0, -1.0, -1)


def test_symbols_wrappers_and_argument_checks():
    L = capi.lib()
    for name in ("epp_motions_clearance", "epp_traj_chord_clearance_batch"):
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.World.edge_clearances) and callable(capi.World.trajectory_chord_clearances)
    argument_errors(L)


def argument_errors(L):
    """Every case is rejected before anything is read: stand-ins for device pointers do."""
    buf = np.zeros(64)
    p = buf.ctypes.data
    world = C.c_void_p(p)  # (a non-NULL handle; never dereferenced by a rejected call)
    edges = {
        "NULL world": (None, p, p, 1, p),
        "n < 0": (world, p, p, -1, p),
        "NULL s1": (world, None, p, 1, p),
        "NULL s2": (world, p, None, 1, p),
        "NULL dist": (world, p, p, 1, None),
    }
    for name, (w, s1, s2, n, dist) in edges.items():
        assert L.epp_motions_clearance(w, s1, s2, n, dist, p, p, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_motions_clearance" in L.epp_last_error(), name
    assert L.epp_motions_clearance(world, None, None, 0, None, None, None, None) == capi.EPP_OK  # launches nothing
    assert L.epp_motions_clearance(world, p, p, 0, p, p, p, None) == capi.EPP_OK
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
        rc = L.epp_traj_chord_clearance_batch(w, T, Cf, off, n, dt, clr, p, p, p, p, None)
        assert rc == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_traj_chord_clearance_batch" in L.epp_last_error(), name
    assert L.epp_traj_chord_clearance_batch(world, None, None, None, 0, 0.05, None, None, None, None, None,
                                            None) == capi.EPP_OK
    assert L.epp_traj_chord_clearance_batch(world, p, p, p, 0, 0.05, p, p, p, p, p, None) == capi.EPP_OK
