"""The inputs of test_gpu_small_path.py, checked with the oracle and epp_build_obbs alone:
the worlds have the OBB counts the tests are named after, and every expectation holds both
outcomes, so that a kernel answering all-valid or all-invalid (or ignoring can_pass) fails."""
import numpy as np
import pytest

import small_path_inputs as S


def test_obb_counts_cover_the_branches():
    """The counts sit on both sides of every size at which the small kernels change path."""
    rec_doubles, block = 17, 256  # kRecDoubles, kSmallBlock
    staged = 5 * block * 2 // rec_doubles  # records covered by stage_records' register copy (kQ = 5)
    assert staged == 150 and {staged, staged + 1} <= set(S.SMALL_OBB_COUNTS)
    assert max(S.SMALL_OBB_COUNTS) == 256 and S.INDEX_OBB_COUNT == 257  # kSmallMaxObbs
    # slice lengths o1 - o0 of the OBB loops: states 1, 2 or 4 slices (unrolled by 4), motions 16
    # (unrolled by 2)
    lengths = {(sl + 1) * n // slices - sl * n // slices
               for n in S.SMALL_OBB_COUNTS for slices in (1, 2, 4, 16) for sl in range(slices)}
    assert {0, 1, 2, 3, 5} <= lengths
    motion = {(sl + 1) * n // 16 - sl * n // 16 for n in S.SMALL_OBB_COUNTS for sl in range(16)}
    assert {0, 1, 2, 3} <= motion and any(m % 2 for m in motion if m > 2)
    assert [S.small_per(n) for n in S.STATE_PREFIXES] == [64, 64, 64, 128, 128, 256, 256, 256]


@pytest.mark.parametrize("n_obb", S.OBB_COUNTS + (72,))
def test_world_has_exactly_n_obbs(n_obb):
    obbs, ref = S.world(n_obb)  # (asserts both counts)
    assert len(obbs) == n_obb == len(ref)
    obbs2, ref2 = S.world(n_obb, True)
    assert len(obbs2) == n_obb and not np.array_equal(ref["center"], ref2["center"])


@pytest.mark.parametrize("n_obb", S.OBB_COUNTS)
def test_state_expectations_hold_both_outcomes(n_obb):
    pts = S.state_points(n_obb)
    assert pts.shape == (S.N_STATES + 1, 3)
    for cp in (0, 1):
        e = S.exp_states(n_obb, cp)[:S.N_STATES]
        assert e.min() == 0 and e.max() == 1, cp
    for md in S.MIN_DISTANCES:
        e = S.exp_mindist(n_obb, md)[:S.N_STATES]
        assert e.min() == 0 and e.max() == 1, md
    if S.n_gates_for(n_obb):  # points inside an opening: invalid unless the gate may be passed
        assert (S.exp_states(n_obb, 1) > S.exp_states(n_obb, 0)).sum() >= 20


@pytest.mark.parametrize("n_obb", S.OBB_COUNTS)
def test_motion_expectations_hold_both_outcomes(n_obb):
    s1, s2 = S.motion_edges(n_obb)
    assert s1.shape == s2.shape == (S.N_MOTIONS + 1, 3)
    for mode in (0, 1):
        for cp in (0, 1):
            e = S.exp_motions(n_obb, cp, mode)[:S.N_MOTIONS]
            assert e.min() == 0 and e.max() == 1, (mode, cp)
    # The worlds of 1, 2 and 3 OBBs are exempt from the can_pass condition: they are obstacles
    # only, without a filling record, so can_pass cannot change an answer there.
    differ = int((S.exp_motions(n_obb, 1, 0) != S.exp_motions(n_obb, 0, 0))[:S.N_MOTIONS].sum())
    if S.n_gates_for(n_obb):
        assert differ >= 20
    else:
        assert n_obb in (1, 2, 3) and differ == 0


@pytest.mark.parametrize("n_obb", S.BOTH_OBB_COUNTS)
def test_both_answers_expectation_holds_every_value(n_obb):
    s1, s2 = S.both_rays(n_obb)
    assert s1.shape == s2.shape == (S.N_BOTH, 3)
    e = S.exp_both(n_obb)
    counts = np.bincount(e, minlength=4)
    # 1 (valid with the fillings, invalid without) cannot occur
    assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) >= 20, counts
    # ... and already among the first 1024 (the small path's batch)
    c = np.bincount(e[:1024], minlength=4)
    assert min(c[0], c[2], c[3]) >= 20, c
    q = S.query_points(n_obb)
    assert q.shape == (S.N_BOTH, 3)


@pytest.mark.parametrize("n_obb", S.FUSED_OBB_COUNTS)
def test_fused_check_expectations(n_obb):
    """The fused check's flags on the world and on its moved version (the update) hold both
    outcomes, and the update changes some of them."""
    for md in S.MIN_DISTANCES:
        for moved in (False, True):
            e = S.exp_mindist(n_obb, md, moved)[:S.N_STATES]
            assert e.min() == 0 and e.max() == 1, (md, moved)
    assert not np.array_equal(S.exp_mindist(n_obb, 0.2, False), S.exp_mindist(n_obb, 0.2, True))


def test_fused_tracks():
    assert len(S.fused_track("2wp")) == 2 and len(S.fused_track("12seg")) == 13 and len(S.fused_track("41seg")) == 42
    for name in ("2wp", "12seg", "41seg"):
        assert len(S.fused_rows(name)) > 0
