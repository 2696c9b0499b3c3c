"""CPU: every input set of the gate-passage tests (gatepass_inputs.py) really holds the outcome
it claims, by the restatement (gatepass_ref.py) on rows sampled by the CPU oracle.  The hand-built
tracks have exact times and positions (DT and V are powers of two), so the oracle's rows are the
device's rows."""
import numpy as np

import gatepass_inputs as gi
import gatepass_ref as gr
import oracle as O


def _rows(T, Cf):
    if len(T) == 0 or not np.isfinite(T).all():
        return np.zeros((0, 10))
    return O.sample_traj(T, Cf, gi.DT)


def _chords(frames, T, Cf):
    return gr.passes(frames, gi.HE, _rows(T, Cf))[0]


def test_single_gate_tracks_hold_their_claims():
    names, Ts, Cs, want = gi.single_gate_tracks()
    assert names[:4] == ["chord 0", "last chord", "lane group edge 7|8", "inside a lane's group 3|4"]
    assert gi.FR1[0].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0]  # yaw 0: c = 1, s = 0 exactly
    n_rows = {}
    for name, T, Cf, w in zip(names, Ts, Cs, want):
        rows = _rows(T, Cf)
        n_rows[name] = len(rows)
        if len(rows):  # exact: times j * DT, positions on the half-metre grid (or the offset given)
            assert np.array_equal(rows[:, 9], np.arange(len(rows)) * gi.DT), name
            assert np.array_equal(rows[:, 3] * 2, np.round(rows[:, 3] * 2)), name
        assert _chords(gi.FR1, T, Cf).tolist() == [w], name
    assert n_rows["1 row"] == 1 and n_rows["2 rows"] == 2
    assert n_rows["512 rows, last chord"] == gi.ROW_CHUNK and n_rows["513 rows, last chord"] == gi.ROW_CHUNK + 1
    assert n_rows["NaN times"] == 0
    assert len(Ts[names.index(f"{gi.K_SEG_LDS + 1} segments")]) == gi.K_SEG_LDS + 1
    # the segment boundary: row 5 in segment 0, row 6 in segment 1
    T = Ts[names.index("segment boundary 5|6")]
    assert 5 * gi.DT <= T[0] < 6 * gi.DT

    def at(name):
        k = names.index(name)
        rows = _rows(Ts[k], Cs[k])
        xyz = rows[:, [0, 3, 6]]
        return gr.cross(gi.FR1, gi.HE, xyz[:-1], xyz[1:])

    # why each negative case is negative: exactly one term of the predicate fails at the chord
    r = at("wrong direction")
    assert (r["g1y"][3, 0], r["g2y"][3, 0]) == (0.5, -0.5) and abs(r["mx"][3, 0]) <= gi.HE >= abs(r["mz"][3, 0])
    r = at("outside in x")
    assert (r["g1y"][3, 0], r["g2y"][3, 0], r["mx"][3, 0], r["mz"][3, 0]) == (-0.5, 0.5, 0.5, 0.0)
    r = at("outside in z")
    assert (r["g1y"][3, 0], r["g2y"][3, 0], r["mx"][3, 0], r["mz"][3, 0]) == (-0.5, 0.5, 0.0, -0.5)
    r = at("x offset == half edge")
    assert r["mx"][3, 0] == gi.HE and r["crossed"][3, 0]  # == counts as inside
    r = at("z offset == -half edge")
    assert r["mz"][3, 0] == -gi.HE and r["crossed"][3, 0]
    r = at("x offset just past the half edge")
    assert r["mx"][3, 0] == np.nextafter(gi.HE, 1.0) and not r["crossed"].any()
    r = at("z offset just past the half edge")
    assert r["mz"][3, 0] == -np.nextafter(gi.HE, 1.0) and not r["crossed"].any()
    # the row on the plane: g.y == 0 exactly ends chord 1 and starts chord 2; neither crosses,
    # and either would with a non-strict inequality
    r = at("a row on the gate plane")
    assert (r["g1y"][1, 0], r["g2y"][1, 0]) == (-1.0, 0.0) and (r["g1y"][2, 0], r["g2y"][2, 0]) == (0.0, 1.0)
    assert not r["crossed"].any()
    assert (r["mx"][1:3, 0] == 0).all() and (r["mz"][1:3, 0] == 0).all()


def test_multi_gate_cases_hold_their_claims():
    cases = {name: (frames, Ts, Cs, want) for name, frames, Ts, Cs, want in gi.multi_gate_cases()}
    for name, (frames, Ts, Cs, want) in cases.items():
        got = np.array([_chords(frames, T, Cf) for T, Cf in zip(Ts, Cs)])
        assert np.array_equal(got, want), (name, got)
    w = cases["two gates passed by the same chord"][3][0]
    assert w[0] == w[1] >= 0
    w = cases["two gates whose crossings lie in different chunks"][3][0]
    assert w[0] // gi.ROW_CHUNK != w[1] // gi.ROW_CHUNK
    # gate 1 is crossed (chord 3), but only before gate 0 is (chord 13)
    frames, Ts, Cs, want = cases["gate 1's only crossing before gate 0's"]
    assert _chords(frames[[1]], Ts[0], Cs[0]).tolist() == [3] and want.tolist() == [[13, -1]]
    # the two-lap track passes each of the two gates twice, at different chords
    frames, Ts, Cs, want = cases["a gate listed twice on a two-lap track"]
    assert np.array_equal(frames[0], frames[2]) and np.array_equal(frames[1], frames[3])
    assert len(set(want[0].tolist())) == 4 and (np.diff(want[0]) > 0).all()
    # the later gate alone is passed; behind a gate that never is, nothing is
    frames, Ts, Cs, want = cases["a later gate crossed while an earlier one never is"]
    assert _chords(frames[[1]], Ts[0], Cs[0]).tolist() == [3] and (want == -1).all()


def test_short_tracks():
    Ts, Cs, want = gi.short_tracks(4)
    assert [len(_rows(T, Cf)) for T, Cf in zip(Ts, Cs)] == [2, 2, 2, 2]
    assert [int(_chords(gi.FR1, T, Cf)[0]) for T, Cf in zip(Ts, Cs)] == want.tolist() == [0, -1, 0, -1]


def test_exact_edges_hold_their_claims():
    s1, s2, want = gi.exact_edges()
    r = gr.cross(gi.FR1, gi.HE, s1, s2)
    assert np.array_equal(r["crossed"][:, 0], want)
    assert want.sum() == 4 and len(want) == 13


def test_random_edges_cover_every_gate_and_keep_off_the_thresholds():
    for G in gi.GATE_COUNTS:
        frames = gi.random_frames(G)
        assert frames.shape == (G, 5)
        for n in gi.EDGE_COUNTS:
            s1, s2 = gi.random_edges(n, G)
            assert s1.shape == s2.shape == (n, 3)
            r = gr.cross(frames, gi.HE, s1, s2)
            near = np.minimum.reduce([np.abs(r["g1y"]), np.abs(r["g2y"]), np.abs(np.abs(r["mx"]) - gi.HE),
                                      np.abs(np.abs(r["mz"]) - gi.HE)])
            assert near.min() > 1e-9, (G, n, near.min())
        # the largest set: every gate's bit is set for some edge and clear for some
        assert r["crossed"].any(axis=0).all() and not r["crossed"].all(axis=0).any()
        m = gr.masks(r["crossed"])
        assert m.dtype == np.uint64 and ((m != 0).sum() > 16)
        if G == 64:
            assert (m >> np.uint64(63)).any()  # the top bit is used
