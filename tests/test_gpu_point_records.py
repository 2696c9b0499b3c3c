"""k_states_v5's plain point test on the 128-byte point records (thresholds inflated by the
host index build, "filling" from bit 15 of the list id): flags bit-exact against the oracle.

  - n = 3, 4, 255, 256, 257, 4099 (no full group, one group, a wave of groups -1 / 0 / +1 and
    the n % 4 tail lanes, which walk their lists on the same records);
  - can_pass_gate 0 and 1;
  - a world with filling OBBs (rotated and unrotated ones of every kind) and the C2 world;
  - EPP_V5_BLOCK unset, 512, 1024;
  - states exactly on |lx| = tx, |ly| = ty, |dz| = tz and up to 3 ulps to either side, on and
    an ulp around the AABB bounds, and inside / outside a filling OBB within r of its faces
    (point_record_inputs, with the constructions of small_path_inputs).

After a gate-pose update (epp_world_update, what PathPlanner::update_gate_pos issues) the
index, and the point-record image with it, is rebuilt: the same comparison on the moved world.
The minDistance variant still stages the 17-double records: one case at n = 257.
"""
import numpy as np
import pytest

from eppamd import capi

import point_record_inputs as P

pytestmark = pytest.mark.gpu

SHAPES = ("", "512", "1024")


@pytest.fixture
def forced(monkeypatch):
    def f(shape):
        monkeypatch.setenv("EPP_STATES_KERNEL", "v5")  # (also keeps n <= 4096 off the brute-force kernel)
        monkeypatch.setenv("EPP_V5_BLOCK", shape)
    return f


def test_states_hold_both_outcomes_and_the_flag_decides():
    """(no launch) The constructed states: both answers, and in the filling world states whose
    flag depends on can_pass_gate (the filling boxes decide them)."""
    for name in ("filling", "c2"):
        e0, e1 = P.expected(name, 0), P.expected(name, 1)
        for n in P.N_EDGES:
            assert 0 < e0[:n].sum() < n, (name, n)
        assert (e1 >= e0).all()
        assert ((e1 > e0).sum() >= 20) == (name == "filling")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("can_pass", [0, 1])
@pytest.mark.parametrize("name", ["filling", "c2"])
def test_point_records_bit_exact(name, can_pass, shape, forced):
    forced(shape)
    _, rg, ro = P.setup(name)
    w = capi.World(P.world(name)[0], rg, ro)
    pts, exp = P.states(name), P.expected(name, can_pass)
    for n in P.N_EDGES:
        got = w.check_states(pts[:n], can_pass)
        assert np.array_equal(got, exp[:n]), (n, np.flatnonzero(got != exp[:n])[:10])


@pytest.mark.parametrize("name", ["filling", "c2"])
def test_gate_update_rebuilds_the_point_records(name, forced):
    forced("")
    _, rg, ro = P.setup(name)
    w = capi.World(P.world(name)[0], rg, ro)
    pts = P.states(name)
    assert np.array_equal(w.check_states(pts, 0), P.expected(name, 0))  # (the index is built and used)
    w.update(P.world(name, moved=True)[0])
    changed = False
    for can_pass in (0, 1):
        exp = P.expected(name, can_pass, moved=True)
        changed |= not np.array_equal(exp, P.expected(name, can_pass))
        for n in P.N_EDGES:
            got = w.check_states(pts[:n], can_pass)
            assert np.array_equal(got, exp[:n]), (can_pass, n, np.flatnonzero(got != exp[:n])[:10])
    assert changed  # the move changes answers: a stale image would be seen


def test_mindist_still_stages_the_old_records(forced):
    forced("")
    _, rg, ro = P.setup("filling")
    w = capi.World(P.world("filling")[0], rg, ro)
    got = w.check_states_mindist(P.states("filling")[:257], P.MIN_DISTANCE)
    exp = P.expected("filling", "md")[:257]
    assert 0 < exp.sum() < 257
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
