"""CPU: the symbols, wrappers and argument checks of epp_gates_crossed and
epp_traj_gate_pass_batch (the checks precede every device call, so they run without a GPU),
and the restatement of the crossing predicate (gatepass_ref.py) against the oracle's
check_gate_passed (oracle/track_planner.py: OnlineTrajGenerator::checkGatePassed)."""
import ctypes as C

import numpy as np

import gatepass_inputs as gi
import gatepass_ref as gr
from eppamd import capi

EPP_ERR_INVALID_ARGUMENT = -1


def test_symbols_and_wrappers():
    L = capi.lib()
    for name in ("epp_gates_crossed", "epp_traj_gate_pass_batch"):
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.gate_frames) and callable(capi.gates_crossed) and callable(capi.trajectory_gate_passes)
    f = capi.gate_frames([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], [0.0, 0.5])
    assert f.shape == (2, 5) and f.dtype == np.float64
    assert f[0].tolist() == [1.0, 2.0, 3.0, 1.0, 0.0]
    assert f[1].tolist() == [4.0, 5.0, 6.0, np.cos(0.5), np.sin(0.5)]
    import online_traj_planner as otp
    assert hasattr(otp.PathPlanner, "gate_frames") and hasattr(otp.PathPlanner, "candidate_gate_passes")
    assert hasattr(otp.OnlineTrajGenerator, "get_gate_passes")


def test_argument_checks():
    L = capi.lib()
    # stand-ins for device pointers: every case below is rejected before anything is read
    buf = np.zeros(64)
    p = buf.ctypes.data
    nan, inf = float("nan"), float("inf")
    edges = {
        "n_gates < 0": (p, -1, 0.425, p, p, 1, p),
        "n_gates 65": (p, 65, 0.425, p, p, 1, p),
        "half_edge < 0": (p, 1, -0.1, p, p, 1, p),
        "half_edge NaN": (p, 1, nan, p, p, 1, p),
        "half_edge inf": (p, 1, inf, p, p, 1, p),
        "n < 0": (p, 1, 0.425, p, p, -1, p),
        "NULL gates": (None, 1, 0.425, p, p, 1, p),
        "NULL s1": (p, 1, 0.425, None, p, 1, p),
        "NULL s2": (p, 1, 0.425, p, None, 1, p),
        "NULL mask": (p, 1, 0.425, p, p, 1, None),
    }
    for name, a in edges.items():
        assert L.epp_gates_crossed(*a, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_gates_crossed" in L.epp_last_error(), name
    assert L.epp_gates_crossed(None, 0, 0.425, None, None, 0, None, None) == capi.EPP_OK  # launches nothing
    assert L.epp_gates_crossed(p, 64, 0.0, p, p, 0, p, None) == capi.EPP_OK
    tracks = {
        "n_gates < 0": (p, -1, 0.425, p, p, p, 1, 0.05, p, p, p, p),
        "n_gates 65": (p, 65, 0.425, p, p, p, 1, 0.05, p, p, p, p),
        "half_edge < 0": (p, 1, -0.1, p, p, p, 1, 0.05, p, p, p, p),
        "half_edge NaN": (p, 1, nan, p, p, p, 1, 0.05, p, p, p, p),
        "half_edge inf": (p, 1, inf, p, p, p, 1, 0.05, p, p, p, p),
        "n_tracks < 0": (p, 1, 0.425, p, p, p, -1, 0.05, p, p, p, p),
        "dt == 0": (p, 1, 0.425, p, p, p, 1, 0.0, p, p, p, p),
        "dt < 0": (p, 1, 0.425, p, p, p, 1, -0.05, p, p, p, p),
        "dt NaN": (p, 1, 0.425, p, p, p, 1, nan, p, p, p, p),
        "dt inf": (p, 1, 0.425, p, p, p, 1, inf, p, p, p, p),
        "NULL gates": (None, 1, 0.425, p, p, p, 1, 0.05, p, p, p, p),
        "NULL seg_times": (p, 1, 0.425, None, p, p, 1, 0.05, p, p, p, p),
        "NULL coeffs": (p, 1, 0.425, p, None, p, 1, 0.05, p, p, p, p),
        "NULL wp_offsets": (p, 1, 0.425, p, p, None, 1, 0.05, p, p, p, p),
        "NULL chord": (p, 1, 0.425, p, p, p, 1, 0.05, None, p, p, p),
        "NULL n_passed": (p, 1, 0.425, p, p, p, 1, 0.05, p, p, p, None),
    }
    for name, a in tracks.items():
        assert L.epp_traj_gate_pass_batch(*a, None) == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_traj_gate_pass_batch" in L.epp_last_error(), name
    assert L.epp_traj_gate_pass_batch(None, 0, 0.425, None, None, None, 0, 0.05, None, None, None, None, None) == capi.EPP_OK
    assert L.epp_traj_gate_pass_batch(p, 64, 0.425, p, p, p, 0, 0.05, p, None, None, p, None) == capi.EPP_OK


def test_restatement_hand_values():
    r = gr.cross(gi.FR1, gi.HE, [[0.25, -1.5, 0.125]], [[0.75, 0.5, -0.375]])
    assert (r["g1y"][0, 0], r["g2y"][0, 0]) == (-1.5, 0.5)
    assert (r["mx"][0, 0], r["mz"][0, 0]) == (0.5, -0.125)
    assert r["u"][0, 0] == 0.75 and not r["crossed"][0, 0]  # (x offset 0.5 > 0.425)
    assert gr.cross(gi.FR1, 0.5, [[0.25, -1.5, 0.125]], [[0.75, 0.5, -0.375]])["crossed"][0, 0]
    # yaw pi / 2: g = R(yaw) t, so world +x is the gate frame's +y
    f = capi.gate_frames([[1.0, 2.0, 3.0]], [np.pi / 2])
    r = gr.cross(f, gi.HE, [[0.0, 2.0, 3.0]], [[2.0, 2.0, 3.0]])
    assert r["crossed"][0, 0] and r["u"][0, 0] == 0.5
    assert not gr.cross(f, gi.HE, [[2.0, 2.0, 3.0]], [[0.0, 2.0, 3.0]])["crossed"][0, 0]
    assert gr.masks(np.array([[True, False, True], [False, False, False]])).tolist() == [5, 0]
    assert gr.masks(np.eye(64, dtype=bool)[63:]).tolist() == [1 << 63]
    # the ordered resolution
    T, F = True, False
    assert gr.ordered(np.array([[F, T], [T, F], [F, F], [F, T]])).tolist() == [1, 3]
    assert gr.ordered(np.array([[T, T], [F, F]])).tolist() == [0, 0]       # the same chord, both gates
    assert gr.ordered(np.array([[F, T], [F, F], [T, F]])).tolist() == [2, -1]  # gate 1 only before gate 0
    assert gr.ordered(np.array([[F, T, T], [F, F, T]])).tolist() == [-1, -1, -1]
    assert gr.ordered(np.zeros((0, 2), bool)).tolist() == [-1, -1]


def test_restatement_equals_oracle_check_gate_passed(geom):
    from track_planner import OnlineTrajGeneratorCPU
    G = 16
    rs = np.random.RandomState(77)
    gates = np.zeros((G, 7))
    gates[:, :2] = rs.uniform(-6, 6, size=(G, 2))
    gates[:, 5] = rs.uniform(-np.pi, np.pi, G)
    gates[:, 6] = rs.randint(0, len(geom.gate_height), G)
    centres = np.column_stack([gates[:, 0] + 0.0, gates[:, 1] + 0.0,
                               gates[:, 2] + np.array([float(geom.gate_height[int(t)]) for t in gates[:, 6]])])
    frames = capi.gate_frames(centres, gates[:, 5])
    oracle = object.__new__(OnlineTrajGeneratorCPU)  # (check_gate_passed reads the gates and the heights only)
    oracle.geom, oracle.gates = geom, gates
    # edges across the gates' planes (gatepass_inputs.random_edges' construction, on these frames)
    n = 400
    g = np.arange(n) % G
    c, s = frames[g, 3], frames[g, 4]
    ga = np.column_stack([rs.uniform(-0.6, 0.6, n), -rs.uniform(0.05, 0.4, n), rs.uniform(-0.6, 0.6, n)])
    gb = np.column_stack([rs.uniform(-0.6, 0.6, n), rs.uniform(0.05, 0.4, n), rs.uniform(-0.6, 0.6, n)])
    flip = rs.uniform(size=n) < 0.25
    ga[flip], gb[flip] = gb[flip].copy(), ga[flip].copy()
    s1 = np.column_stack([c * ga[:, 0] + s * ga[:, 1], -s * ga[:, 0] + c * ga[:, 1], ga[:, 2]]) + frames[g, :3]
    s2 = np.column_stack([c * gb[:, 0] + s * gb[:, 1], -s * gb[:, 0] + c * gb[:, 1], gb[:, 2]]) + frames[g, :3]
    r = gr.cross(frames, gi.HE, s1, s2)
    # no value within 1e-9 of a threshold: math.cos (the oracle's) against numpy's cannot decide
    near = np.minimum.reduce([np.abs(r["g1y"]), np.abs(r["g2y"]), np.abs(np.abs(r["mx"]) - gi.HE),
                              np.abs(np.abs(r["mz"]) - gi.HE)])
    assert near.min() > 1e-9
    want = np.array([[oracle.check_gate_passed(s1[i], s2[i], k) for k in range(G)] for i in range(n)])
    assert np.array_equal(r["crossed"], want)
    own = r["crossed"][np.arange(n), g]
    assert 40 < own.sum() < n - 40  # both outcomes, many times
