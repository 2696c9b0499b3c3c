"""GPU parity of the brute-force small-query kernels (small.hip, small_body.h, and the fused
check of k_check_refit in minsnap_refit.hip) against the CPU oracle, bit for bit, across OBB counts
and batch sizes at which that code changes path:

  OBB count   1..256 run the small kernels, 257 the index kernels; stage_records copies 150
              records through registers and the rest in a tail loop; a workgroup splits the
              list into 1, 2 or 4 (states) or 16 (motions) slices, whose lengths here include
              0, 1, 2, 3 and 5 (loops unrolled by 4 and by 2)
  batch size  64 / 128 / 256 queries per workgroup, one and many workgroups; 4096 | 4097 states
              and 1024 | 1025 edges (small path | index kernels), 16384 | 16385 (World::query's
              zero-copy | DMA-staged route)

Every call runs in the default environment and once more with EPP_STATES_KERNEL /
EPP_MOTIONS_KERNEL forcing the index kernels: both must give the oracle's flags.  Worlds,
queries and expectations: small_path_inputs.py (checked on their own by
test_small_path_inputs_cpu.py).
"""
import numpy as np
import pytest

import oracle as O
from eppamd import capi

import small_path_inputs as S

pytestmark = pytest.mark.gpu


def _routes(monkeypatch):
    """The default route, then the index kernels forced (a test hook of small.hip)."""
    yield "default"
    monkeypatch.setenv("EPP_STATES_KERNEL", "v5")
    monkeypatch.setenv("EPP_MOTIONS_KERNEL", "v5")
    yield "index"
    monkeypatch.delenv("EPP_STATES_KERNEL")
    monkeypatch.delenv("EPP_MOTIONS_KERNEL")


def _same(got, exp, what):
    assert np.array_equal(got, exp), (what, np.flatnonzero(np.asarray(got) != np.asarray(exp))[:10])


# ---- 1. states --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obb", S.OBB_COUNTS)
def test_states(n_obb, monkeypatch):
    """k_states_small<false, false>, <false, true> (compacting) and <true, false> (minDistance)
    at every prefix, both can_pass values and minDistance 0.0 and 0.2; 4097 states (and 100 on
    the 257-OBB world) take the index kernels and get the same comparison."""
    _, rg, ro = S.setup()
    obbs, _ = S.world(n_obb)
    pts = S.state_points(n_obb)
    w = capi.World(obbs, rg, ro)
    sizes = S.STATE_PREFIXES + (S.N_STATES + 1,) + ((100,) if n_obb == S.INDEX_OBB_COUNT else ())
    for route in _routes(monkeypatch):
        for n in sizes:
            for cp in (0, 1):
                exp = S.exp_states(n_obb, cp)[:n]
                _same(w.check_states(pts[:n], cp), exp, (route, n, cp))
                valid, idx = w.check_states(pts[:n], cp, compact=True)
                _same(valid, exp, (route, n, cp, "compact flags"))
                assert len(idx) == int(exp.sum()), (route, n, cp)
                _same(np.sort(idx), np.flatnonzero(exp), (route, n, cp, "compact idx"))
            for md in S.MIN_DISTANCES:
                _same(w.check_states_mindist(pts[:n], md), S.exp_mindist(n_obb, md)[:n], (route, n, md))
    w.close()


# ---- 2. motions -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obb", S.OBB_COUNTS)
def test_motions(n_obb, monkeypatch):
    """k_motions_small<0> (analytic) and <1> (32-step discretised) at every prefix and both
    can_pass values; 1025 edges (and everything on the 257-OBB world) take the index kernels."""
    _, rg, ro = S.setup()
    obbs, _ = S.world(n_obb)
    s1, s2 = S.motion_edges(n_obb)
    w = capi.World(obbs, rg, ro)
    for route in _routes(monkeypatch):
        for n in S.MOTION_PREFIXES + (S.N_MOTIONS + 1,):
            for mode in (0, 1):
                for cp in (0, 1):
                    _same(w.check_motions(s1[:n], s2[:n], cp, mode), S.exp_motions(n_obb, cp, mode)[:n],
                          (route, n, mode, cp))
    w.close()


# ---- 3. both answers of a ray in one pass -----------------------------------------------------
def _planner(n_obb):
    import online_traj_planner as otp
    gates, obstacles = S.poses(n_obb)
    return otp.PathPlanner(np.array(gates), np.array(obstacles), S.FILLING_CONFIG)


@pytest.mark.parametrize("n_obb", S.BOTH_OBB_COUNTS)
def test_check_rays_both(n_obb, monkeypatch):
    """World::checkRaysBoth: up to 1024 rays on <= 256 OBBs in one launch of k_motions_small<0>
    (can_pass == kCanPassBoth; 4 to 16 records per slice here, so the in-slice short-circuits see
    further records after a hit), else the two checkRays calls (zero-copy up to 16384 rays,
    DMA-staged above).  Bit 0 = the oracle's checkRayValid(.., false), bit 1 = (.., true)."""
    pp = _planner(n_obb)
    s1, s2 = S.both_rays(n_obb)
    exp = S.exp_both(n_obb)
    for route in _routes(monkeypatch):
        for n in S.BOTH_PREFIXES:
            _same(np.asarray(pp.check_rays_both(s1[:n], s2[:n])), exp[:n], (route, n))


# ---- 4. World::query's routes, per element ----------------------------------------------------
@pytest.mark.parametrize("n_obb", [72, 256])
def test_world_query_routes_per_element(n_obb, monkeypatch):
    """World::checkPoints / checkRays on host arrays: the small route (<= 4096 points, <= 1024
    rays), zero-copy + index kernel (<= 16384) and DMA-staged (above), one flag per query vs the
    oracle; again after two gate updates, where the index is stale: the small route (called
    first) reads the pinned records of the new version, the large routes rebuild the index."""
    fgeom, rg, ro = S.setup()
    gates, obstacles = S.poses(n_obb)
    pp = _planner(n_obb)
    pts = S.query_points(n_obb)
    s1, s2 = S.both_rays(n_obb)
    g = np.array(gates)
    for version in range(2):
        if version:
            for k, (dx, dyaw) in ((1, (0.2, -0.15)), (6, (-0.25, 0.2))):
                g[k, 0] += dx
                g[k, 5] += dyaw
                pp.update_gate_pos(k, list(g[k, :6]))
        ref = O.world_build(fgeom, g, obstacles, rg, ro)
        exp_p = [O.check_states(ref, rg, ro, pts, bool(cp), threads=8) for cp in (0, 1)]
        exp_r = [O.check_motions(ref, rg, ro, s1, s2, bool(cp), 0, threads=8) for cp in (0, 1)]
        if version:
            assert not np.array_equal(exp_p[0][:S.N_STATES], S.exp_states(n_obb, 0)[:S.N_STATES])
        for e in exp_p + exp_r:
            assert e[:1024].min() == 0 and e[:1024].max() == 1
        for route in _routes(monkeypatch):
            # (the small sizes first: after an update they run on the stale index)
            for n_p, n_r in zip((S.N_STATES, S.N_STATES + 1, 16384, 16385), (S.N_MOTIONS, S.N_MOTIONS + 1, 16384, 16385)):
                for cp in (0, 1):
                    _same(np.asarray(pp.check_points(pts[:n_p], bool(cp))), exp_p[cp][:n_p], (version, route, n_p, cp))
                    _same(np.asarray(pp.check_rays(s1[:n_r], s2[:n_r], bool(cp))), exp_r[cp][:n_r],
                          (version, route, n_r, cp))


# ---- 5. the fused check of the online step ----------------------------------------------------
@pytest.mark.parametrize("track", ["2wp", "12seg", "41seg"])
@pytest.mark.parametrize("n_obb", S.FUSED_OBB_COUNTS)
def test_fused_check(n_obb, track):
    """epp_check_and_generate_trajectory_host: the minDistance flags of k_check_refit's check
    workgroups (states_small_body<true, false>) vs the oracle, bit for bit, beside a refit of 2
    waypoints (the dynamic LDS is then sized by the records of the larger worlds), of 12 segments
    and of 41 (k_check_refit<false>: segment scratch in global memory); the rows equal those of
    generate_trajectory (bit for bit) and the oracle's (time column exact, the rest within 1e-6).
    Once on the current index and once after an update (records read from pinned memory)."""
    _, rg, ro = S.setup()
    v_max, a_max, dt, t0, v0, a0 = S.FUSED_ARGS
    wp = S.fused_track(track)
    rows0 = S.fused_rows(track)
    sep = capi.generate_trajectory(wp, v_max, a_max, dt, t0, v0, a0)
    assert sep.shape == rows0.shape and np.array_equal(sep[:, 9], rows0[:, 9])
    assert np.abs(sep[:, :9] - rows0[:, :9]).max() < 1e-6
    pts = S.state_points(n_obb)
    w = capi.World(S.world(n_obb)[0], rg, ro)
    for version in range(2):
        if version:
            w.update(S.world(n_obb, True)[0])  # index stale: pinned records
        for md in S.MIN_DISTANCES:
            exp = S.exp_mindist(n_obb, md, bool(version))
            for n in S.FUSED_N_CHECK:
                flags, rows = capi.check_and_generate_trajectory(w, pts[:n], md, wp, v_max, a_max, dt, t0, v0, a0)
                _same(flags, exp[:n], (version, md, n))
                assert np.array_equal(rows, sep), (version, md, n)
    w.close()


@pytest.mark.parametrize("track", ["2wp", "41seg"])
def test_fused_check_unsupported_past_256_obbs(track):
    """257 OBBs: not the small path's world, EPP_ERR_UNSUPPORTED (the caller makes the two calls)."""
    _, rg, ro = S.setup()
    v_max, a_max, dt, t0, v0, a0 = S.FUSED_ARGS
    w = capi.World(S.world(S.INDEX_OBB_COUNT)[0], rg, ro)
    with pytest.raises(capi.EppError) as e:
        capi.check_and_generate_trajectory(w, S.state_points(S.INDEX_OBB_COUNT)[:64], 0.2, S.fused_track(track),
                                           v_max, a_max, dt, t0, v0, a0)
    assert e.value.code == capi.EPP_ERR_UNSUPPORTED
    w.close()
