"""Named, deterministic node sets at the edges of the exact k-NN's argument, and a Python
restatement of its grid (test_knn_edge_inputs_cpu.py, test_gpu_knn_edges.py).

The k-NN has four kernels with one answer (knn_kernels.h): k_knn over all pairs, k_knn_grid
walking shells of cells, and k_knn_tile + k_knn_retry.  The bulk -- random clouds with some
duplicates -- is covered in test_gpu_planner.py.  The cases here stand where the argument is
under load; each is a dict of `nodes`, `max_dist`, an optional `box` and a note `for`:

    lattice_r1/r2/r3   14 x 14 x 11 lattice of spacing 2^-2 (2156 nodes), max_dist 1, 2, 3
                       spacings: the squared radii 1, 4, 9 x 2^-4 are attained exactly, so
                       the radius rule (in range iff d < max_dist^2, exclusive) decides rows
    lattice_shuffled   the same lattice in a permuted order, max_dist 2 spacings
    switch_2048/2049   one uniform cloud cut on both sides of kKnnBruteMax (knn.hip)
    tiny_n_<n>         n in TINY_N: n <= K, n = K + 1, and cap = max(64, n) around 64
    all_same           2100 copies of one point: h = 1e-12, one cell
    two_points         1050 copies each of two points 1 m apart along x
    line_x/y/z         2100 nodes on a 100 m segment along one axis: that axis is capped at
                       1024 cells and what lies beyond is clamped into the last cell
    plane_xz           a plane: y extent 0
    diagonal           a line along (1, 1, 1): most cells empty
    blob_outliers      2090 nodes from N(0, 0.05) and 10 nodes 50 .. 200 m away
    radius_sub_h, radius_h, radius_3h, radius_none_in_range
                       the uniform cloud with max_dist 0.5, 1 and 3 cell edges of its own grid,
                       and 1e-6
    far_origin, far_1km, far_100km
                       the uniform cloud as it is (the control), and translated by
                       (2^10, -2^10, 2^10) and by (2^17, -2^17, 2^17)
    wide_box           the uniform cloud under a caller box 100 x its bounding box per axis

Everything is built once per process, shared, and read-only.
"""
import functools

import numpy as np

from knn_ref import knn_ref

# knn_kernels.h / knn_tile.hip / knn.hip
NODES_PER_CELL = 1.5
TILE_B, TILE_H = 4, 2
TILE_CAP = 1344
BRUTE_MAX = 2048
AXIS_CELLS = 1024

KS = (4, 8, 16, 32)
N = 2100
TINY_N = (1, 2, 3, 4, 5, 9, 17, 33, 63, 64, 65)
LATTICE_DIMS = (14, 14, 11)
LATTICE_STEP = 0.25
CLOUD_LO, CLOUD_HI = (0.0, 0.0, 0.0), (4.0, 4.0, 2.0)
FAR_OFFSETS = {"far_origin": 0.0, "far_1km": 2.0 ** 10, "far_100km": 2.0 ** 17}


# ---- the grid, restated ------------------------------------------------------------------------
def knn_grid_shape(lo, hi, n, cap=None, npc=NODES_PER_CELL):
    """knn_grid.h's knn_grid_shape over the box [lo, hi] for n nodes: dict of lo, h, inv_h,
    dims, ncell.  cap: knn_layout's max(64, n)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    cap = max(64, n) if cap is None else cap
    ext = hi - lo
    floor_ext = max(float(ext.max()), 1e-9) * 1e-3
    vol = 1.0
    for d in range(3):
        vol *= max(float(ext[d]), floor_ext)
    h = max(float(np.cbrt(npc * vol / float(n if n > 1 else 1))), 1e-12)
    while True:
        dims = tuple(int(min(float(ext[d]) / h, AXIS_CELLS - 1.0)) + 1 for d in range(3))
        if dims[0] * dims[1] * dims[2] <= cap:
            break
        h *= 1.25
    return {"lo": lo.copy(), "h": h, "inv_h": 1.0 / h, "dims": dims, "ncell": dims[0] * dims[1] * dims[2]}


def knn_cell_unclamped(v, g, d):
    """(int)((v - lo[d]) * inv_h) of knn_cell_axis before its clamp (v: array of coordinates)."""
    return np.trunc((np.asarray(v, np.float64) - g["lo"][d]) * g["inv_h"]).astype(np.int64)


def knn_cell_axis(v, g, d):
    """knn_grid.h's knn_cell_axis: the cell of coordinate v on axis d, clamped into the grid."""
    return np.clip(knn_cell_unclamped(v, g, d), 0, g["dims"][d] - 1)


def grid_of(case):
    """The grid a case's nodes get: over the caller's box where it has one, else over the
    nodes' bounding box."""
    nodes = case["nodes"]
    lo, hi = case["box"] if case.get("box") is not None else (nodes.min(0), nodes.max(0))
    return knn_grid_shape(lo, hi, len(nodes))


def cells_of(nodes, g):
    """(n, 3) clamped cell coordinates."""
    return np.stack([knn_cell_axis(nodes[:, d], g, d) for d in range(3)], 1)


def max_halo_count(nodes, g):
    """The most nodes any k_knn_tile block with a query has in its halo: blocks of TILE_B^3 cells,
    TILE_H cells of halo on every side (over TILE_CAP: the block's queries all retry)."""
    c = cells_of(nodes, g)
    best = 0
    for b in np.unique(c // TILE_B, axis=0):
        o = b * TILE_B - TILE_H
        inside = np.all((c >= o) & (c < o + TILE_B + 2 * TILE_H), axis=1)
        best = max(best, int(inside.sum()))
    return best


# ---- the node sets -----------------------------------------------------------------------------
def _frozen(a):
    a = np.ascontiguousarray(a, np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lattice():
    """The lattice in x-fastest order: exact dyadic coordinates."""
    nx, ny, nz = LATTICE_DIMS
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return _frozen(np.stack([x, y, z], -1).reshape(-1, 3) * LATTICE_STEP)


@functools.lru_cache(maxsize=None)
def cloud(n=N, seed=20):
    """n nodes uniform in CLOUD_LO .. CLOUD_HI; nodes 0 and 1 are the box's corners, so every cut
    of it from 2 nodes up has the same bounding box."""
    rs = np.random.RandomState(seed)
    p = rs.uniform(CLOUD_LO, CLOUD_HI, (n, 3))
    p[0], p[1] = CLOUD_LO, CLOUD_HI
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def _segment():
    """N coordinates uniform on 0 .. 100 m, both ends present."""
    t = np.random.RandomState(21).uniform(0.0, 100.0, N)
    t[0], t[1] = 0.0, 100.0
    return t


def _line(axis):
    p = np.empty((N, 3))
    p[:] = (1.5, -0.5, 0.75)
    p[:, axis] = _segment()
    return p


def _case(nodes, max_dist, what, box=None):
    if box is not None:
        box = (_frozen(box[0]), _frozen(box[1]))
    return {"nodes": _frozen(nodes), "max_dist": float(max_dist), "box": box, "for": what}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, in a fixed order."""
    c = {}
    lat = lattice()
    for r in (1, 2, 3):
        c[f"lattice_r{r}"] = _case(lat, r * LATTICE_STEP, f"squared radius {r * r} x 2^-4 attained exactly")
    perm = np.random.RandomState(22).permutation(len(lat))
    c["lattice_shuffled"] = _case(lat[perm], 2 * LATTICE_STEP, "index ties and visiting order permuted")
    big = cloud(BRUTE_MAX + 1)
    c["switch_2048"] = _case(big[:BRUTE_MAX], 0.0, "the largest table of the all-pairs kernel")
    c["switch_2049"] = _case(big, 0.0, "the smallest table of the grid pipeline")
    for n in TINY_N:
        c[f"tiny_n_{n}"] = _case(cloud(65, 23)[:n], 0.0, "n <= K, n = K + 1, cap = max(64, n)")
    pt = np.array([0.3, -1.7, 2.9])
    c["all_same"] = _case(np.tile(pt, (N, 1)), 0.0, "h = 1e-12, one cell, every query crowded, ties by index only")
    two = np.tile(pt, (N, 1))
    two[1::2, 0] += 1.0
    c["two_points"] = _case(two, 0.0, "two cells 1023 apart, 1050 nodes each")
    for axis, name in enumerate("xyz"):
        c[f"line_{name}"] = _case(_line(axis), 0.0, f"axis {name} capped at 1024 cells, the rest clamped")
    rs = np.random.RandomState(24)
    plane = rs.uniform((-3.0, 0.0, -3.0), (3.0, 0.0, 3.0), (N, 3))
    plane[:, 1] = 0.4
    c["plane_xz"] = _case(plane, 0.0, "y extent 0")
    t = rs.uniform(0.0, 10.0, N)
    t[0], t[1] = 0.0, 10.0
    c["diagonal"] = _case(np.stack([t + 0.5, t - 2.0, t + 1.0], 1), 0.0, "a line along (1, 1, 1): most cells empty")
    blob = rs.normal(0.0, 0.05, (N, 3))
    u = rs.normal(0.0, 1.0, (10, 3))
    blob[N - 10:] = u / np.linalg.norm(u, axis=1, keepdims=True) * np.linspace(50.0, 200.0, 10)[:, None]
    c["blob_outliers"] = _case(blob, 0.0, "one or two crowded cells; the outliers walk out to rmax")
    uni = cloud()
    h = knn_grid_shape(uni.min(0), uni.max(0), N)["h"]
    for name, md in (("radius_sub_h", 0.5 * h), ("radius_h", 1.0 * h), ("radius_3h", 3.0 * h),
                     ("radius_none_in_range", 1e-6)):
        c[name] = _case(uni, md, "radius against Dcut, in_range, knn_done and the retry's bound")
    for name, off in FAR_OFFSETS.items():
        c[name] = _case(uni + np.array([off, -off, off]), 0.0, "h 1e-6 margins and block-centre floats off the origin")
    lo, hi = uni.min(0), uni.max(0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    c["wide_box"] = _case(uni, 0.0, "every node in one or two cells per axis of the caller's grid",
                          box=(mid - 100.0 * half, mid + 100.0 * half))
    return c


NAMES = tuple(cases())
LATTICE_RADIUS = ("lattice_r1", "lattice_r2", "lattice_r3")
TIGHT_BOX = ("line_x", "far_100km")  # additionally run under their tight bounding box


def tight_box(name):
    nodes = cases()[name]["nodes"]
    return nodes.min(0), nodes.max(0)


def sq_dists(nodes, i):
    """(dx^2 + dy^2) + dz^2 in double from node i to every node: the kernels' expression."""
    d = nodes - nodes[i]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


@functools.lru_cache(maxsize=None)
def reference(name):
    """knn_ref(nodes, 32, max_dist) of a case; columns [:K] are knn_ref(nodes, K, max_dist)."""
    c = cases()[name]
    ref = knn_ref(c["nodes"], max(KS), c["max_dist"])
    ref.setflags(write=False)
    return ref
