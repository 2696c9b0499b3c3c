"""The inputs of test_gpu_motion_tile_shapes.py, checked with the oracle and the host-only index
build (epp_dbg_build_blob) alone: the worlds reach the tile shapes the GPU test is about, fit
the tile kernel's LDS, set the upper words of their tile rows, and every expectation holds
both outcomes, so that the GPU test cannot pass vacuously.

Run with -s to see the table of shapes and the valid / invalid shares.
"""
import ctypes as C

import numpy as np
import pytest

from eppamd import capi

import tile_shape_inputs as I


def test_shape_witnesses():
    """Together the worlds reach every W > 1, a world of T >= 3 at W > 1, and two S < 64."""
    shapes = {name: I.shape(name) for name in I.WORLDS}
    print()
    for name, s in shapes.items():
        print(f"{name:6s} n={s['n']:4d} T={s['T']:2d} W={s['W']:2d} S={s['S']:2d} LDS={s['lds']:7,d} bytes")
    assert {s["W"] for s in shapes.values()} >= {2, 4, 8, 16, 32}
    assert any(s["T"] >= 3 and s["W"] > 1 for s in shapes.values())
    assert len({s["S"] for s in shapes.values() if s["S"] < 64}) >= 2
    assert all(s["S"] >= 4 and s["T"] >= 1 for s in shapes.values())
    g = shapes[I.GATE_CLUSTER]
    assert g["W"] >= 4


@pytest.mark.parametrize("name", I.WORLDS)
def test_world_fits_the_tile_kernels_lds(name):
    """launch_motions_tile declines a world whose records, tile rows and wave queues exceed
    kLdsBudget; the world would then run on the cell-list kernel and the GPU test would say
    nothing about k_motions_v5."""
    s = I.shape(name)
    # This restates tile_lds() in csrc/motions_tile.hip:
    #   align16(136 n) + 4 T^2 tile_words + 16 (256 * 4 + 64) <= 150 * 1024
    lds = ((136 * s["n"] + 15) & ~15) + 4 * s["T"] ** 2 * s["tile_words"] + 16 * (256 * 4 + 64)
    assert lds == s["lds"] and lds <= 150 * 1024, (name, lds)
    # tile_words of build_blob: 6 S rows of slab_row_stride(W) = W + 1 words (W even), the FX,
    # FY and FILL rows, 32 W u16 ids; rounded up to 4 words
    assert s["tile_words"] == (6 * s["S"] * (s["W"] + 1) + 3 * s["W"] + 16 * s["W"] + 3) & ~3


def _sure_tile_members(name):
    """Per tile (ty, tx) the ids, ascending, of the OBBs that are in it whichever way the
    builder's float slab index rounds: the AABB (of the oracle) overlaps the tile of the T x T
    tiling of the world's bounding box shrunk by a hundredth of its side.  A subset of the
    tile's OBBs in the tile's own order, so an OBB's position in it is a lower bound of its
    slot (bit j & 31 of word j >> 5) and the length a lower bound of the tile's population."""
    t = I.shape(name)["T"]
    _, ref = I.world(name)
    lo, hi = I.extent(name)
    side = (hi[:2] - lo[:2]) / t
    out = {}
    for ty in range(t):
        for tx in range(t):
            tlo = lo[:2] + side * [tx, ty] + 0.01 * side
            thi = lo[:2] + side * [tx + 1, ty + 1] - 0.01 * side
            m = ((ref["aabb_lo"][:, :2] <= thi) & (ref["aabb_hi"][:, :2] >= tlo)).all(axis=1)
            out[ty, tx] = np.flatnonzero(m)
    return out


@pytest.mark.parametrize("name", I.WORLDS)
def test_some_tile_sets_the_upper_words(name):
    """Computed directly, from the oracle's AABBs and the T x T tiling of the world's bounding
    box: some tile holds more than 32 (W / 2) OBBs, so its rows have bits in words W / 2 and up
    (with fewer, a kernel that read only the lower half of every row would pass)."""
    w = I.shape(name)["W"]
    pop = max(len(ids) for ids in _sure_tile_members(name).values())
    print(f"\n{name}: largest tile holds >= {pop} OBBs, W = {w}")
    assert 32 * (w // 2) < pop <= 32 * w


def test_first_tile_rows_are_mixed_past_the_first_word():
    """For W = 4, 8 and 16 some world has a tile (not in the first column / row) in which,
    among the slots of 32 and more, some OBBs start in that tile and others come in from the
    tile before it: the FX / FY rows then hold zeros and ones in their upper words.  (W = 32
    leaves no LDS for a second tile.)"""
    mixed = {}
    for name in I.WORLDS:
        s = I.shape(name)
        _, ref = I.world(name)
        lo, hi = I.extent(name)
        side = (hi[:2] - lo[:2]) / s["T"]
        for (ty, tx), ids in _sure_tile_members(name).items():
            for ax, t in ((0, tx), (1, ty)):
                if t == 0:
                    continue
                edge = lo[ax] + side[ax] * t
                upper = ids[32:]
                starts_here = (ref["aabb_lo"][upper, ax] > edge + 0.01 * side[ax]).sum()
                comes_in = (ref["aabb_lo"][upper, ax] < edge - 0.01 * side[ax]).sum()
                if min(starts_here, comes_in) >= 8:
                    mixed.setdefault(s["W"], set()).add((name, "xy"[ax]))
    print("\nmixed FX / FY rows past the first word:", {w: sorted(v) for w, v in mixed.items()})
    assert {4, 8, 16} <= set(mixed)
    assert all({ax for _, ax in mixed[w]} == {"x", "y"} for w in (4, 8, 16))


def test_gate_cluster_has_fillings_past_the_first_word():
    """On the gate cluster some opening sits at a tile slot of 32 or more: the FILL row is
    used beyond its first word, and not only in the last word."""
    _, ref = I.world(I.GATE_CLUSTER)
    assert int(ref["filling"].sum()) == I.N_CLUSTER_GATES
    words = set()
    for ids in _sure_tile_members(I.GATE_CLUSTER).values():
        words |= {int(j) >> 5 for j in np.flatnonzero(ref["filling"][ids] != 0)}
    print("\nFILL words used (at least):", sorted(words))
    assert max(words) >= 1 and len(words) >= 2


@pytest.mark.parametrize("name", I.WORLDS)
def test_edges_hold_every_kind(name):
    s1, s2 = I.motion_edges(name)
    kind = I.edge_kind(name)
    assert s1.shape == s2.shape == (I.N_EDGES, 3) and I.N_EDGES > 1024  # kSmallMotions
    d = s2 - s1
    length = np.linalg.norm(d, axis=1)
    k = {n: kind == i for i, n in enumerate(I.KINDS)}
    assert length.max() <= I.MAX_LEN * (1 + 1e-12)
    assert length[k["short"]].max() <= 0.5 and (length[k["long"]] > 6.0).sum() > 100
    assert (length[k["zero"]] == 0.0).all() and k["zero"].sum() >= 100
    # outside: beyond the bounding box of the inflated AABBs, on each of its six sides
    lo, hi = I.extent(name)
    for ax in range(3):
        below = k["outside"] & (np.maximum(s1[:, ax], s2[:, ax]) < lo[ax])
        above = k["outside"] & (np.minimum(s1[:, ax], s2[:, ax]) > hi[ax])
        assert below.sum() >= 100 and above.sum() >= 100, (name, ax)
    # parallel: one component on either side of the 1e-6 threshold, per axis
    p = np.abs(d[k["parallel"]])
    for ax in range(3):
        assert ((p[:, ax] > 0) & (p[:, ax] < 1e-6)).sum() >= 100 and ((p[:, ax] > 1e-6) & (p[:, ax] < 1.1e-6)).sum() >= 100
    # the long edges cross every tile boundary
    t = I.shape(name)["T"]
    for ax in range(2):
        for b in range(1, t):
            x = lo[ax] + (hi[ax] - lo[ax]) * b / t
            crossing = (np.minimum(s1[:, ax], s2[:, ax]) < x) & (np.maximum(s1[:, ax], s2[:, ax]) > x)
            assert (crossing & (k["long"] | k["through"])).sum() >= 100, (name, ax, b)
    # Candidates per wave: the (edge, OBB) pairs whose AABBs overlap (closed, the rtree query)
    # are a subset of the tile filter's candidates.  Some wave of 64 consecutive edges has more
    # of them than the wave's queue holds (kQueueV5), some lane alone more than 64.
    _, ref = I.world(name)
    elo, ehi = np.minimum(s1, s2), np.maximum(s1, s2)
    pairs = np.zeros(I.N_EDGES, np.int64)
    for o in ref:
        pairs += ((elo <= o["aabb_hi"]) & (ehi >= o["aabb_lo"])).all(axis=1)
    per_wave = np.add.reduceat(pairs, np.arange(0, I.N_EDGES, 64))
    print(f"\n{name}: pairs per wave {per_wave.min()} .. {per_wave.max()}, per edge up to {pairs.max()}")
    assert per_wave.max() > I.K_QUEUE_V5 and per_wave.min() == 0
    assert pairs.max() > min(64, len(ref) // 2)


@pytest.mark.parametrize("name", I.WORLDS)
def test_motion_expectations_hold_both_outcomes(name):
    """At least 10 % valid and 10 % invalid edges in every (mode, can_pass); on the gate
    cluster can_pass changes the answer of at least 1 % of the edges."""
    print()
    for mode in (0, 1):
        for cp in (0, 1):
            e = I.exp_motions(name, mode, cp)
            share = float(e.mean())
            print(f"{name:6s} mode={mode} can_pass={cp} valid {share:6.1%} invalid {1 - share:6.1%}")
            assert e.shape == (I.N_EDGES,) and 0.10 <= share <= 0.90, (name, mode, cp, share)
        differ = float((I.exp_motions(name, mode, 0) != I.exp_motions(name, mode, 1)).mean())
        if name == I.GATE_CLUSTER:
            print(f"{name:6s} mode={mode} can_pass changes {differ:6.2%}")
            assert differ >= 0.01, (mode, differ)
        else:
            assert differ == 0.0  # (obstacles only: no filling record)


@pytest.mark.parametrize("name", I.WORLDS)
def test_knn_table(name):
    nodes, nbr = I.knn_table(name)
    assert nodes.shape == (I.KNN_NODES, 3) and nbr.shape == (I.KNN_NODES, I.KNN_K) and nbr.dtype == np.int32
    assert I.KNN_K == 8 and nbr.size > 1024  # kSmallMotions
    assert 20 <= (nbr == -1).sum() and nbr.min() == -1 and nbr.max() < I.KNN_NODES
    s1, s2 = I.knn_table_edges(name)
    assert np.array_equal(s1[:I.KNN_K], np.repeat(nodes[:1], I.KNN_K, axis=0))
    missing = nbr.reshape(-1) < 0
    assert np.array_equal(s2[missing], s1[missing]) and not np.array_equal(s2[~missing], s1[~missing])
    for mode in (0, 1):
        for cp in (0, 1):
            e = I.exp_knn_motions(name, mode, cp)
            assert 0.10 <= e.mean() <= 0.90, (name, mode, cp, float(e.mean()))


def test_state_kernels_on_both_sides_of_the_staging_budget():
    """The part k_states_v5 stages (epp_dbg_class_layout: from the point records on) is within
    kStageBudget = 64 KiB on some worlds and past it on others, which go to k_states_v4."""
    f = capi.lib().epp_dbg_class_layout
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    staged = {}
    for name in I.WORLDS:
        _, rg, ro = I.setup(name)
        obbs, _ = I.world(name)
        out = np.zeros(12, np.int64)
        capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, out.ctypes.data))
        staged[name] = int(out[11])
    print("\nstaged bytes:", staged)
    assert min(staged.values()) <= 32 * 1024 and max(staged.values()) > 64 * 1024
    assert sum(v <= 64 * 1024 for v in staged.values()) >= 2 and sum(v > 64 * 1024 for v in staged.values()) >= 2


@pytest.mark.parametrize("name", I.WORLDS)
def test_state_expectations_hold_both_outcomes(name):
    pts = I.state_points(name)
    assert len(pts) > I.N_POINTS
    for e in (I.exp_states(name, 0), I.exp_states(name, 1), I.exp_mindist(name)):
        assert e.shape == (len(pts),) and 0.10 <= e.mean() <= 0.90, (name, float(e.mean()))
    if name == I.GATE_CLUSTER:
        assert (I.exp_states(name, 1) > I.exp_states(name, 0)).sum() >= 20
