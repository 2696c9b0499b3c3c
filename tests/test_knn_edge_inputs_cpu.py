"""The k-NN edge cases (knn_edge_inputs.py) reach the branches they are for: no GPU needed.

What test_gpu_knn_edges.py compares is only worth as much as its inputs: a lattice whose
squared distances are exact and attain the squared radius, a line whose far end is clamped
into the last cell, clouds that crowd one halo, radii on both sides of the tile's reach.
"""
import numpy as np
import pytest

import knn_edge_inputs as I
from knn_ref import knn_ref


def test_case_shapes():
    for name, c in I.cases().items():
        n = len(c["nodes"])
        assert c["nodes"].shape == (n, 3) and c["nodes"].dtype == np.float64, name
        assert 1 <= n <= 2200, name
        assert np.isfinite(c["nodes"]).all(), name
        if c["box"] is not None:  # epp.h: every node inside the caller's box
            assert (c["nodes"] >= c["box"][0]).all() and (c["nodes"] <= c["box"][1]).all(), name
    assert len(I.lattice()) == 2156
    assert len(I.cases()["switch_2048"]["nodes"]) == I.BRUTE_MAX
    assert len(I.cases()["switch_2049"]["nodes"]) == I.BRUTE_MAX + 1
    assert np.array_equal(I.cases()["switch_2049"]["nodes"][:I.BRUTE_MAX], I.cases()["switch_2048"]["nodes"])


def _lattice_ints(nodes):
    q = nodes * 4.0
    assert np.array_equal(q, np.round(q)), "every coordinate a multiple of 2^-2"
    return q.astype(np.int64)


@pytest.mark.parametrize("name", I.LATTICE_RADIUS + ("lattice_shuffled",))
def test_lattice_distances_are_exact(name):
    """The double expression of every pair's squared distance equals the integer one (in units
    of 2^-4): the double reference is the exact answer, ties and radius included."""
    nodes = I.cases()[name]["nodes"]
    q = _lattice_ints(nodes)
    for i in range(len(nodes)):
        d = q - q[i]
        exact = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]  # int64, < 2^10
        assert np.array_equal(I.sq_dists(nodes, i) * 16.0, exact)
    for i in (0, 1077, len(nodes) - 1):  # and with Python ints
        qi = [int(v) for v in q[i]]
        for j in range(0, len(nodes), 7):
            e = sum((int(q[j, a]) - qi[a]) ** 2 for a in range(3))
            assert I.sq_dists(nodes, i)[j] == e / 16 and (e / 16) * 16 == e


@pytest.mark.parametrize("name", I.LATTICE_RADIUS)
def test_lattice_radius_is_attained(name):
    """At least half of the queries have another node at exactly max_dist^2, and the rows of an
    inclusive radius differ from the reference's."""
    c = I.cases()[name]
    nodes, r2 = c["nodes"], c["max_dist"] * c["max_dist"]
    q = _lattice_ints(nodes)
    r2_int = round(r2 * 16)
    assert r2_int / 16 == r2
    on = 0
    for i in range(len(nodes)):
        d = q - q[i]
        on += bool(((d * d).sum(1) == r2_int).any())
    assert 2 * on >= len(nodes), on
    ref = I.reference(name)
    incl = knn_ref(nodes, 32, float(np.nextafter(c["max_dist"], np.inf)))  # d <= max_dist^2
    differ = int((ref != incl).any(1).sum())
    print(f"{name}: {on} queries with a node at the radius, {differ} rows differ under <=")
    assert differ > 0  # (r3: only where fewer than 32 nodes are in range, at the lattice's rim)


def test_lines_are_capped_and_clamped():
    for axis, name in enumerate("xyz"):
        c = I.cases()[f"line_{name}"]
        g = I.grid_of(c)
        dims = [1, 1, 1]
        dims[axis] = I.AXIS_CELLS
        assert g["dims"] == tuple(dims), (name, g["dims"])
        beyond = int((I.knn_cell_unclamped(c["nodes"][:, axis], g, axis) > I.AXIS_CELLS - 1).sum())
        print(f"line_{name}: h {g['h']:.4f}, {beyond} nodes beyond the last cell")
        assert beyond >= 100
        assert abs(g["h"] - 0.0894) < 1e-4
    # two_points: the second point lies beyond the capped axis too
    c = I.cases()["two_points"]
    g = I.grid_of(c)
    assert g["dims"] == (I.AXIS_CELLS, 1, 1)
    assert int((I.knn_cell_unclamped(c["nodes"][:, 0], g, 0) > I.AXIS_CELLS - 1).sum()) == I.N // 2


@pytest.mark.parametrize("name", ["all_same", "wide_box", "blob_outliers"])
def test_crowded_cases_overflow_the_halo(name):
    """All nodes (blob_outliers: the blob) within 2 cells per axis, and more than kTileCap of them
    in one halo: the tile pass sends every such query to the retry pass."""
    c = I.cases()[name]
    g = I.grid_of(c)
    nodes = c["nodes"][:I.N - 10] if name == "blob_outliers" else c["nodes"]
    cells = I.cells_of(nodes, g)
    span = cells.max(0) - cells.min(0) + 1
    assert (span <= 2).all(), span
    assert I.max_halo_count(c["nodes"], g) > I.TILE_CAP
    if name == "all_same":
        assert g["h"] == 1e-12 and g["dims"] == (1, 1, 1)


def test_radius_regimes():
    c = I.cases()
    g = I.grid_of(c["radius_h"])
    h = g["h"]
    assert c["radius_sub_h"]["max_dist"] == 0.5 * h and c["radius_h"]["max_dist"] == h
    # beyond the tile's reach: the cube of kTileH shells guarantees at most kTileH h
    assert c["radius_3h"]["max_dist"] > I.TILE_H * h
    assert I.max_halo_count(c["radius_h"]["nodes"], g) <= I.TILE_CAP  # the tile pass does run
    assert (I.reference("radius_none_in_range") == -1).all()
    sub = I.reference("radius_sub_h")[:, :16]
    ragged = ((sub >= 0).any(1) & (sub < 0).any(1)).sum()
    assert ragged >= len(sub) // 4 and (sub < 0).all(1).any(), ragged
    # radius_h: about 6 nodes in range, so for K = 4 some rows fill (the K-th is a node) and some
    # do not (the K-th stays r2max: what the tile pass hands the retry as its bound); radius_3h:
    # about 170 in range, rows fill but at the cloud's corners for K = 32
    for name in ("radius_h", "radius_3h"):
        for k in I.KS:
            r = I.reference(name)[:, :k]
            print(f"{name} k {k}: {int((r >= 0).all(1).sum())} full rows of {len(r)}")
    rh = I.reference("radius_h")[:, :4]
    assert (rh >= 0).all(1).sum() >= 100 and (rh < 0).any(1).sum() >= 100
    assert (I.reference("radius_3h") < 0).any() and (I.reference("radius_3h")[:, :16] >= 0).all()


def test_tiny_n_covers_k():
    ns = set(I.TINY_N)
    for k in I.KS:
        assert any(n <= k for n in ns) and k + 1 in ns, k
    assert {63, 64, 65} <= ns  # cap = max(64, n) on both sides of 64
    for n in I.TINY_N:
        assert len(I.cases()[f"tiny_n_{n}"]["nodes"]) == n


def test_far_clouds_keep_their_shape():
    """The translated clouds resolve the margins: the ulp of a coordinate is far below h 1e-6, and
    the grid is the control's."""
    g0 = I.grid_of(I.cases()["far_origin"])
    for name, off in I.FAR_OFFSETS.items():
        c = I.cases()[name]
        g = I.grid_of(c)
        assert g["dims"] == g0["dims"] and abs(g["h"] - g0["h"]) < 1e-9 * g0["h"]
        assert np.spacing(np.abs(c["nodes"]).max()) < 1e-3 * (g["h"] * 1e-6)
        assert abs(c["nodes"][:, 1].min() + off) < 1e-9 + 1e-12 * off or off == 0.0


def test_diagonal_is_mostly_empty():
    c = I.cases()["diagonal"]
    g = I.grid_of(c)
    cells = I.cells_of(c["nodes"], g)
    used = len(np.unique(cells, axis=0))
    assert min(g["dims"]) >= 8 and used * 10 <= g["ncell"], (g["dims"], used)


def test_plane_is_flat():
    g = I.grid_of(I.cases()["plane_xz"])
    assert g["dims"][1] == 1 and g["dims"][0] > 8 and g["dims"][2] > 8


@pytest.mark.parametrize("name", ["radius_sub_h", "tiny_n_9"])
def test_reference_slices(name):
    c = I.cases()[name]
    for k in I.KS:
        assert np.array_equal(I.reference(name)[:, :k], knn_ref(c["nodes"], k, c["max_dist"])), k


def test_shape_helper_matches_spilled_block_test():
    """test_gpu_planner.py::test_knn_tile_spilled_block places its extra nodes by this grid: 20064
    nodes over (0, 0, 0) .. (8, 8, 8)."""
    g = I.knn_grid_shape([0.0, 0.0, 0.0], [8.0, 8.0, 8.0], 20000 + 64)
    assert g["h"] == np.cbrt(1.5 * 512.0 / (20000 + 64))
    assert g["dims"] == (24, 24, 24) and g["ncell"] <= 20064
