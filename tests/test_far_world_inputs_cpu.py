"""The inputs of test_gpu_far_worlds.py and the host index build on worlds far from the origin,
checked without a GPU: with the oracle, the host-only debug entries of world_index.cpp
(epp_dbg_cull_grid, epp_dbg_build_blob, epp_dbg_class_layout) and a float32 numpy restatement
of fine_coord.

The property: the cull grid's upper cut lim[k] is no lower than the fine coordinate of any AABB
top face.  It used to be 4 n (1 + 2^-20), argued from a float extent (float)g1 - (float)g0
within ulps of the extent; it is within ulps of |g0| and |g1|, and a state just under the top
face of a far world then had a fine coordinate beyond the cut: declared valid without a test.
The other checks pin the inputs to that hole (so the GPU tests are sharp) and show that the far
worlds still run the kernels the GPU tests name.

Run with -s for the figures.
"""
import numpy as np
import pytest

from eppamd import capi

import far_world_inputs as I

ALL_OFFSETS = tuple(I.OFFSETS[w] for w in I.WORLDS) + tuple((o, -o) for o in I.BUILD_ONLY_OFFSETS)


@pytest.mark.parametrize("name", I.WORLDS)
def test_both_outcomes_everywhere(name):
    _, kind, _ = I.states(name)
    for v in (0, 1) + I.MIN_DISTANCES:
        exp = I.exp_states(name, v)
        share = exp[kind == 0].mean()
        print(f"\n{name} states variant {v}: {exp.mean():.3f} valid, of the uniform ones {share:.3f}")
        assert 0 < exp.sum() < len(exp)
        assert 0.05 <= share <= 0.95
    _, _, ek = I.edges(name)
    for mode in (0, 1):
        for cp in (0, 1):
            exp = I.exp_motions(name, mode, cp)
            print(f"{name} motions mode {mode} can_pass {cp}: {exp.mean():.3f} valid")
            assert 0 < exp.sum() < len(exp)
            assert 0 < exp[ek == 0].sum() < (ek == 0).sum()
    for md in I.MIN_DISTANCES:
        exp = I.exp_hover_mindist(name, md)
        assert 0 < exp.sum() < len(exp)
    assert 0 < I.exp_hover_chords(name, 0).sum() < len(I.hover_points(name)[0])


@pytest.mark.parametrize("name", I.WORLDS)
def test_counts_stay_off_the_brute_force_path(name):
    pts, kind, lad = I.states(name)
    s, e, ek = I.edges(name)
    assert len(pts) % 4 == 3 and 4096 < len(pts) <= 8192
    assert len(s) % 4 == 3 and 1024 < len(s) <= 8192
    assert (kind[:257] == 2).sum() >= 5 and (ek[:513] == 2).sum() >= 20  # the small-path prefixes hold ladder entries
    L = I.ladder(name)
    assert np.array_equal(pts[kind == 2], L["p"][lad[kind == 2]])
    assert np.isnan(pts).any() and np.isinf(pts).any() and (np.abs(pts) == 1e30).any()


@pytest.mark.parametrize("name", I.WORLDS)
def test_sliver_ladder_is_in_collision(name):
    """The oracle calls at most 10 % of the ladder states valid (a 1-ulp rung may fall outside the
    OBB threshold by rounding); every rung of >= 4 ulps on a cap face (x, y) is invalid at
    can_pass = 0; every face-parallel ladder edge is invalid in mode 1, and keeps p[k]."""
    pts, kind, lad = I.states(name)
    L = I.ladder(name)
    row = lad[kind == 2]
    for v in (0, 1) + I.MIN_DISTANCES:
        assert I.exp_states(name, v)[kind == 2].mean() <= 0.10
    e0 = I.exp_states(name, 0)[kind == 2]
    cap_rung = (L["axis"][row] < 2) & (L["ulps"][row] >= 4)
    assert cap_rung.sum() >= 4 * I.LADDER_REPS * I.POW_RUNGS and not e0[cap_rung].any()
    s, e, ek = I.edges(name)
    par = ek == 2
    assert (s[par] != e[par]).any(axis=1).all()
    assert ((s[par] == e[par]).sum(axis=1) >= 1).all()
    for cp in (0, 1):
        assert not I.exp_motions(name, 1, cp)[par].any()
    # the discrete32 samples of a parallel edge keep the ladder coordinate exactly
    k = np.argmax(s[par] == e[par], axis=1)
    for t in np.arange(1, 33) / 32.0:
        q = s[par] + (e[par] - s[par]) * t
        assert (q[np.arange(len(k)), k] == s[par][np.arange(len(k)), k]).all()


@pytest.mark.parametrize("off", ALL_OFFSETS, ids=lambda o: f"{o[0]:g}")
def test_cull_limit_covers_every_aabb_top(off):
    """(a) fine_coord(aabb_hi[i][k]) <= lim[k] for every OBB i and axis k; and the cut is never
    below the earlier 4 n (1 + 2^-20)."""
    obbs, ref = I.world_at(*off)
    g = I.cull_grid(obbs)
    assert np.array_equal(g["g0"], ref["aabb_lo"].min(axis=0)) and np.array_equal(g["g1"], ref["aabb_hi"].max(axis=0))
    assert np.array_equal(g["of"], g["g0"].astype(np.float32))
    assert np.array_equal(g["fmax"], (4 * g["n"] - 1).astype(np.float32))
    bad = []
    for k in range(3):
        f = I.fine_coord(ref["aabb_hi"][:, k], g["of"][k], g["i4"][k])
        assert (I.fine_coord(ref["aabb_lo"][:, k], g["of"][k], g["i4"][k]) >= 0).all()
        print(f"\noffset {off} axis {k}: n {g['n'][k]}, lim {g['lim'][k]!r}, largest fine coordinate of a top face "
              f"{f.max()!r}, 4n(1 + 2^-20) {I.old_limit(g['n'][k])!r}")
        assert g["lim"][k] >= I.old_limit(g["n"][k])
        if not (f <= g["lim"][k]).all():
            bad.append((k, int(np.argmax(f)), float(f.max()), float(g["lim"][k])))
    assert not bad, f"(axis, OBB, fine coordinate of its top face, lim): {bad}"


@pytest.mark.parametrize("name", I.FAR)
def test_ladder_reaches_the_sliver(name):
    """(b) on the +x and +y faces at least three ladder rungs have a fine coordinate above
    4 n (1 + 2^-20), the bound that was not enough; all of them are within the present cut."""
    obbs, _ = I.world(name)
    g = I.cull_grid(obbs)
    L = I.ladder(name)
    for k in (0, 1):
        sel = (L["axis"] == k) & (L["top"] == 1)
        f = I.fine_coord(L["p"][sel, k], g["of"][k], g["i4"][k])
        over = f > I.old_limit(g["n"][k])
        rungs = np.unique(L["d"][sel][over])
        print(f"\n{name} +{'xy'[k]}: {len(rungs)} rungs beyond 4n(1 + 2^-20), the widest {I.sliver_width(name, k):.2e} m,"
              f" overshoot {float(f.max()) / float(4 * g['n'][k]) - 1:.2e}")
        assert len(rungs) >= 3
        assert (f <= g["lim"][k]).all()
    near = I.cull_grid(I.world("near")[0])
    Ln = I.ladder("near")
    for k in (0, 1):  # the control has no sliver
        sel = (Ln["axis"] == k) & (Ln["top"] == 1)
        assert (I.fine_coord(Ln["p"][sel, k], near["of"][k], near["i4"][k]) <= I.old_limit(near["n"][k])).all()


def test_index_builds_far_away_and_in_time():
    """The index build of every world, and at offsets up to 1e8, returns EPP_OK; none takes more
    than 20x the "near" build of the same run (the class grid's widening loop iterates far
    away).  Host timing is noisy: the factor is loose on purpose, and the best of three counts."""
    offs = ALL_OFFSETS + ((1e8, -1e8),)

    def best(off):
        us = []
        for _ in range(3):
            st, out = I.build_blob(I.world_at(*off)[0], reps=1)
            assert st == capi.EPP_OK, (off, st)
            us.append(out["us"])
        return min(us)

    near = best(I.OFFSETS["near"])
    times = {off: best(off) for off in offs[1:]}
    msg = f"near {near:.0f} us; " + ", ".join(f"{o[0]:g}: {t:.0f} us" for o, t in times.items())
    print("\nindex build: " + msg)
    assert all(t <= 20 * near for t in times.values()), msg


@pytest.mark.parametrize("name", I.WORLDS)
def test_far_worlds_run_the_kernels_the_gpu_tests_name(name):
    """k_states_v5 takes a world whose staged bytes are <= 64 KiB (kStageBudget), the tile kernel
    k_motions_v5 one that has tiles."""
    obbs, _ = I.world(name)
    lay = I.class_layout(obbs)
    st, blob = I.build_blob(obbs)
    print(f"\n{name}: class grid {lay['bnx']} x {lay['bny']} x {lay['bnz']}, staged {lay['staged']} bytes, "
          f"tiles T {blob['tile_n']:.0f} W {blob['slab_w']:.0f} S {blob['slab_n']:.0f}")
    assert st == capi.EPP_OK
    assert 0 < lay["staged"] <= 64 * 1024
    assert blob["tile_n"] >= 1 and blob["slab_n"] >= 4 and blob["slab_w"] >= 1
