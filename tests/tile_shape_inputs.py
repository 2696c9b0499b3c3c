"""Worlds, edges, k-NN tables and state points of the tile-shape tests
(test_gpu_motion_tile_shapes.py) and of the CPU test of those inputs
(test_tile_shape_inputs_cpu.py).

k_motions_v5 (csrc/motions_tile.hip) is compiled per row width W in {1, 2, 4, 8, 16, 32} (words
of OBB bits per tile row); build_blob (csrc/world_index.cpp) picks the smallest W, then the
fewest tiles T per axis, for which no tile holds more than 32 W OBBs, then S local slabs per
tile by the LDS budget.  The suite's other worlds are spread out and all come out at W = 1,
S = 64.  The worlds here are cluttered: a patch where more than 32 W / 2 inflated AABBs overlap
one tile, so that the builder has to choose W = 2 ... 32, and with it T >= 3 and S < 64.

Every world is built from the project's own geometry (configs/config.json; the gate cluster
from configs/config_filling.json) with capi.build_obbs, so that O.world_build gives the
oracle's world from the same poses.

Everything is input data and oracle output: built once per process, shared, read-only.
"""
import ctypes as C
import functools
import os

import numpy as np

import oracle as O
from eppamd import capi, config

from knn_ref import knn_ref
from small_path_inputs import adversarial_points  # noqa: F401  (the state tests' edge points)

_CONFIGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "configs")

# name: (obstacles of the cluster, their x / y within +-span, further obstacles within +-6)
CLUSTERS = {
    "n40": (40, 0.05, 0),
    "n180": (120, 0.05, 60),
    "n500": (500, 1.0, 0),
    "n350": (250, 0.05, 100),
    "n600": (500, 0.05, 100),
    "n700": (700, 6.0, 0),
    # T = 2 at W = 16: the tile boundaries run through the cluster, so in every tile the FX / FY
    # rows ("this OBB starts in this tile") differ from word to word (with the cluster inside
    # one tile, as in n180, those rows are all ones wherever the cluster's bits are)
    "n520": (280, 0.05, 240),
}
GATE_CLUSTER = "gates"  # config_filling.json: N_CLUSTER_GATES gates around one point
N_CLUSTER_GATES = 24
# The gate centres lie within +-GATE_SPREAD of the origin.  The frames' bars stand 0.25 m from
# their gate's centre and block, inflated, everything from 0.125 m outwards; a column of about
# 0.08 m around the origin stays free of bars, and between the small portals' top bars (up to
# z = 0.9) and the large portals' (from 1.125) only the large portals' openings fill it.
GATE_SPREAD = 0.03
GATE_COLUMN = (np.array([-0.07, -0.07, 0.88]), np.array([0.07, 0.07, 1.15]))
WORLDS = tuple(CLUSTERS) + (GATE_CLUSTER,)
SEED = 5

N_EDGES = 20_000  # > kSmallMotions = 1024: not the brute-force small path
KNN_NODES, KNN_K = 640, 8  # 5120 table entries > kSmallMotions
N_POINTS = 20_000
MIN_DISTANCE = 0.15
Z_RANGE = (0.0, 2.0)
FAR = 6.0  # the obstacles outside the cluster are uniform in +-FAR
MAX_LEN = 12.0  # of an edge

K_QUEUE_V5 = 256                            # kQueueV5 (motions_tile.hip)
LDS_BUDGET = 150 * 1024                     # kLdsBudget (launch_helpers.h)
REC_BYTES = 17 * 8                          # kRecDoubles doubles per OBB record
WAVE_QUEUES = 16 * (K_QUEUE_V5 * 4 + 64)    # 16 waves: queue + flags


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def setup(name):
    """(geometry, r_gate, r_obstacle) of the world's config."""
    cfg = config.load(os.path.join(_CONFIGS, "config_filling.json" if name == GATE_CLUSTER else "config.json"))
    return (config.geometry(cfg),) + tuple(config.inflate_radii(cfg))


@functools.lru_cache(maxsize=None)
def poses(name):
    """(gates (g, 7), obstacles (o, 6)): obstacle rows (x, y, 0, 0, 0, yaw), gate rows
    (x, y, 0, 0, 0, yaw, type) as synth.track_world writes them."""
    rs = np.random.RandomState(SEED)
    if name == GATE_CLUSTER:
        g = np.zeros((N_CLUSTER_GATES, 7))
        g[:, :2] = rs.uniform(-GATE_SPREAD, GATE_SPREAD, size=(N_CLUSTER_GATES, 2))
        g[:, 5] = rs.uniform(-3.0, 3.0, N_CLUSTER_GATES)
        g[:, 6] = np.arange(N_CLUSTER_GATES) % 2  # large and small portals: two opening heights
        return _frozen(g, np.zeros((0, 6)))
    n, span, far = CLUSTERS[name]
    obst = np.zeros((n + far, 6))
    obst[:n, :2] = rs.uniform(-span, span, size=(n, 2))
    obst[n:, :2] = rs.uniform(-FAR, FAR, size=(far, 2))
    obst[:, 5] = rs.uniform(-3.0, 3.0, n + far)
    return _frozen(np.zeros((0, 7)), obst)


@functools.lru_cache(maxsize=None)
def world(name):
    """(OBBs for capi.World, the oracle's world) of poses(name)."""
    geom, rg, ro = setup(name)
    gates, obstacles = poses(name)
    obbs = capi.build_obbs(geom, gates, obstacles)
    ref = O.world_build(geom, gates, obstacles, rg, ro)
    assert len(obbs) == len(ref) == 6 * len(gates) + len(obstacles)
    return _frozen(obbs, ref)


@functools.lru_cache(maxsize=None)
def shape(name):
    """The tile shape build_blob gives the world, from the host-only entry epp_dbg_build_blob
    (no device): n OBBs, T tiles per axis, W words per row, S slabs per tile, words per tile,
    and the dynamic LDS of k_motions_v5 on it."""
    _, rg, ro = setup(name)
    obbs, _ = world(name)
    f = capi.lib().epp_dbg_build_blob
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]
    f.restype = C.c_int32
    out = np.zeros(6)
    capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, 1, out.ctypes.data))
    n, t, tw, w, s = len(obbs), int(out[2]), int(out[3]), int(out[4]), int(out[5])
    return {"n": n, "T": t, "W": w, "S": s, "tile_words": tw, "lds": tile_lds_bytes(n, t, tw)}


def tile_lds_bytes(n, t, tile_words):
    """The dynamic LDS of k_motions_v5: records, tile rows, the 16 waves' queues.  This
    restates tile_lds() in csrc/motions_tile.hip."""
    return ((REC_BYTES * n + 15) & ~15) + 4 * t * t * tile_words + WAVE_QUEUES


def extent(name):
    """(lo, hi) of the union of the inflated AABBs: the box the tiles divide."""
    _, ref = world(name)
    return ref["aabb_lo"].min(axis=0), ref["aabb_hi"].max(axis=0)


def cluster_box(name):
    """(lo, hi) in x / y of the cluster's inflated AABBs (the whole world where the cluster
    is the world), z over Z_RANGE."""
    _, ref = world(name)
    n = len(ref) if name == GATE_CLUSTER else CLUSTERS[name][0]
    lo, hi = ref["aabb_lo"][:n].min(axis=0), ref["aabb_hi"][:n].max(axis=0)
    return np.array([lo[0], lo[1], Z_RANGE[0]]), np.array([hi[0], hi[1], Z_RANGE[1]])


def _unit(rs, n, zscale=0.4):
    d = rs.normal(size=(n, 3)) * [1.0, 1.0, zscale]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def corner_pairs(name, rs, k, out=0.04, into=0.06, among=None):
    """k pairs of points (a, b) across a vertical edge of an inflated OBB: a up to `out` m
    outside the corner along the box's diagonal, b up to `into` m inside, both jittered by a
    centimetre, at a height within the box.  Three of four OBBs are drawn from the cluster
    (or all from the ids `among`).

    In a cluster the boxes lie on top of each other, and an edge through its middle hits
    dozens of them: an answer of "invalid" survives the loss of almost any one candidate.
    The corners are where one box sticks out of the others, so that the edge's answer hangs
    on that OBB alone being among the candidates."""
    _, rg, ro = setup(name)
    _, ref = world(name)
    n_cl = len(ref) if name == GATE_CLUSTER else CLUSTERS[name][0]
    if among is not None and len(among):
        i = among[rs.randint(0, len(among), k)]
    else:
        i = np.where(rs.rand(k) < 0.75, rs.randint(0, n_cl, k), rs.randint(0, len(ref), k))
    o = ref[i]
    r = np.where(o["filling"] != 0, 0.0, np.where(o["is_gate"] != 0, rg, ro))
    sx, sy = rs.choice([-1.0, 1.0], k), rs.choice([-1.0, 1.0], k)
    lx, ly = sx * (o["half"][:, 0] + r), sy * (o["half"][:, 1] + r)
    c, s = o["rot"][:, 0], o["rot"][:, 3]
    corner = np.stack([o["center"][:, 0] + c * lx - s * ly, o["center"][:, 1] + s * lx + c * ly,
                       rs.uniform(np.maximum(o["aabb_lo"][:, 2], Z_RANGE[0]), o["aabb_hi"][:, 2])], 1)
    u = np.stack([c * lx - s * ly, s * lx + c * ly, np.zeros(k)], 1)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = corner + u * rs.uniform(0.0, out, (k, 1)) + rs.uniform(-0.01, 0.01, (k, 3))
    b = corner - u * rs.uniform(0.0, into, (k, 1)) + rs.uniform(-0.01, 0.01, (k, 3))
    return a, b


KINDS = ("short", "corner", "long", "through", "outside", "zero", "parallel")
N_SHORT, N_CORNER, N_LONG, N_THROUGH, N_OUT, N_ZERO, N_PAR = 5000, 4400, 3000, 3000, 1800, 400, 2400
assert N_SHORT + N_CORNER + N_LONG + N_THROUGH + N_OUT + N_ZERO + N_PAR == N_EDGES


@functools.lru_cache(maxsize=None)
def _edges(name):
    """N_EDGES edges (s1, s2) and their kinds:
      short     <= 0.5 m, starting in a box 0.4 m around the cluster: many start, end or pass
                inside it;
      corner    across a vertical edge of an inflated OBB (corner_pairs): a decimetre at most,
                or ending just inside the corner from up to 0.8 m away;
      long      up to 12 m between two points of the whole world (+-FAR at least): they cross
                every tile boundary and collect more candidates per wave than kQueueV5;
      through   long edges aimed through a point of the cluster;
      outside   entirely beyond the world's bounding box, on each of its six sides;
      zero      zero-length, in the cluster box;
      parallel  0.8 m along x beside the cluster with |d_y| = 9.9e-7 / 1.01e-6, the two sides
                of the 1e-6 parallel threshold (as test_motions_bit_exact makes them); a
                third of them with |d_z| so, a third along y with |d_x| so.
    On the gate cluster an eighth of the short edges lie in GATE_COLUMN, where only openings
    are in the way: valid only when the gates may be passed."""
    rs = np.random.RandomState(1000 + WORLDS.index(name))
    clo, chi = cluster_box(name)
    wlo, whi = extent(name)
    wlo = np.minimum(np.array([wlo[0], wlo[1], Z_RANGE[0]]), [-FAR, -FAR, 0.0])
    whi = np.maximum(np.array([whi[0], whi[1], Z_RANGE[1]]), [FAR, FAR, 0.0])
    pad = np.array([0.4, 0.4, 0.0])
    # short
    a = rs.uniform(clo - pad, chi + pad, size=(N_SHORT, 3))
    b = a + _unit(rs, N_SHORT) * rs.uniform(0.0, 0.5, (N_SHORT, 1))
    if name == GATE_CLUSTER:
        k = N_SHORT // 8
        a[:k] = rs.uniform(*GATE_COLUMN, size=(k, 3))
        b[:k] = np.clip(a[:k] + _unit(rs, k, 1.0) * rs.uniform(0.0, 0.1, (k, 1)), *GATE_COLUMN)
    s1, s2 = [a], [b]
    # corner; every other one from up to 0.8 m away in any direction, and of those every other
    # one at an OBB within 0.4 m of a boundary between two tiles (where there is one): edges
    # that enter a second tile and there depend on one OBB, which the FX / FY rows must keep
    a, b = corner_pairs(name, rs, N_CORNER)
    t = shape(name)["T"]
    if t > 1:
        _, ref = world(name)
        lo, hi = extent(name)
        near = np.zeros(len(ref), bool)
        for ax in range(2):
            for j in range(1, t):
                x = lo[ax] + (hi[ax] - lo[ax]) * j / t
                near |= (ref["aabb_lo"][:, ax] < x + 0.4) & (ref["aabb_hi"][:, ax] > x - 0.4)
        k = N_CORNER // 4
        a[1:4 * k:4], b[1:4 * k:4] = corner_pairs(name, rs, k, among=np.flatnonzero(near))
    far = np.arange(N_CORNER) % 2 == 1
    a[far] = b[far] + _unit(rs, int(far.sum()), 0.2) * rs.uniform(0.05, 0.8, (int(far.sum()), 1))
    s1.append(a)
    s2.append(b)

    def capped(a, b):  # b pulled towards a where the edge is longer than MAX_LEN
        length = np.linalg.norm(b - a, axis=1, keepdims=True)
        return a + (b - a) * np.minimum(1.0, MAX_LEN / np.maximum(length, 1e-300))

    # long
    a = rs.uniform(wlo, whi, size=(N_LONG, 3))
    s1.append(a)
    s2.append(capped(a, rs.uniform(wlo, whi, size=(N_LONG, 3))))
    # through the cluster
    a = rs.uniform(wlo, whi, size=(N_THROUGH, 3))
    p = rs.uniform(clo, chi, size=(N_THROUGH, 3))
    s1.append(a)
    s2.append(capped(a, a + (p - a) * rs.uniform(1.0, 2.0, (N_THROUGH, 1))))
    # outside, per side
    lo, hi = extent(name)
    a = rs.uniform(lo - 1.0, hi + 1.0, size=(N_OUT, 3))
    b = rs.uniform(lo - 1.0, hi + 1.0, size=(N_OUT, 3))
    side = np.arange(N_OUT) % 6
    for ax in range(3):
        for sgn, bound in ((0, lo[ax]), (1, hi[ax])):
            m = side == 2 * ax + sgn
            off = rs.uniform(1e-3, 3.0, size=(int(m.sum()), 2))
            a[m, ax] = bound + (off[:, 0] if sgn else -off[:, 0])
            b[m, ax] = bound + (off[:, 1] if sgn else -off[:, 1])
    s1.append(a)
    s2.append(capped(a, b))  # (still beyond the same side)
    # zero length
    a = rs.uniform(clo - pad, chi + pad, size=(N_ZERO, 3))
    s1.append(a)
    s2.append(a.copy())
    # near-parallel
    a = rs.uniform(clo - [1.0, 0.5, 0.0], chi + [0.2, 0.5, 0.0], size=(N_PAR, 3))
    b = a.copy()
    eps = np.where(np.arange(N_PAR) % 2, 9.9e-7, 1.01e-6) * np.where(np.arange(N_PAR) % 4 < 2, 1.0, -1.0)
    kind = np.arange(N_PAR) % 3
    b[kind == 0, 0] += 0.8
    b[kind == 0, 1] += eps[kind == 0]
    b[kind == 1, 0] += 0.8
    b[kind == 1, 2] += eps[kind == 1]
    b[kind == 2, 1] += 0.8
    b[kind == 2, 0] += eps[kind == 2]
    s1.append(a)
    s2.append(b)
    # The even-numbered edges of every kind stay together, kind after kind: waves (64
    # consecutive edges) of one kind, from no candidate at all to hundreds per lane.  The
    # odd-numbered ones follow shuffled: waves that mix the kinds.
    s1, s2 = np.vstack(s1), np.vstack(s2)
    order = np.concatenate([np.arange(0, N_EDGES, 2), 1 + 2 * rs.permutation(N_EDGES // 2)])
    kind = np.repeat(np.arange(len(KINDS)), [N_SHORT, N_CORNER, N_LONG, N_THROUGH, N_OUT, N_ZERO, N_PAR])
    return _frozen(np.ascontiguousarray(s1[order]), np.ascontiguousarray(s2[order]), kind[order])


def motion_edges(name):
    return _edges(name)[:2]


def edge_kind(name):
    """Per edge of motion_edges(name) its kind, an index into KINDS."""
    return _edges(name)[2]


@functools.lru_cache(maxsize=None)
def knn_table(name):
    """(nodes (KNN_NODES, 3), nbr (KNN_NODES, KNN_K) int32): half of the nodes are
    corner_pairs (each other's near neighbours: edges whose answer hangs on one OBB), a
    quarter lie in and around the cluster box, the rest anywhere in the world; the exact k-NN
    (knn_ref), a tenth of the entries replaced by a random node (long edges across the tiles)
    and a twentieth by -1 (no neighbour: the degenerate edge from the node to itself)."""
    rs = np.random.RandomState(2000 + WORLDS.index(name))
    clo, chi = cluster_box(name)
    pairs = np.vstack(corner_pairs(name, rs, KNN_NODES // 4))
    near = rs.uniform(clo - [0.5, 0.5, 0.0], chi + [0.5, 0.5, 0.0], size=(KNN_NODES // 4, 3))
    far = rs.uniform([-FAR, -FAR, Z_RANGE[0]], [FAR, FAR, Z_RANGE[1]], size=(KNN_NODES - len(pairs) - len(near), 3))
    nodes = np.ascontiguousarray(np.vstack([pairs, near, far])[rs.permutation(KNN_NODES)])
    nbr = knn_ref(nodes, KNN_K)
    u = rs.rand(KNN_NODES, KNN_K)
    nbr = np.where(u < 0.10, rs.randint(0, KNN_NODES, size=nbr.shape), nbr)
    nbr = np.where(u > 0.95, -1, nbr).astype(np.int32)
    assert (nbr < 0).any() and nbr.size > 1024
    return _frozen(nodes, np.ascontiguousarray(nbr))


@functools.lru_cache(maxsize=None)
def knn_table_edges(name):
    """The edges the table denotes, built on the host as epp_knn_edges lays them out: edge
    i * k + j from node i to node nbr[i, j], a missing neighbour from the node to itself."""
    nodes, nbr = knn_table(name)
    src = np.repeat(np.arange(KNN_NODES), KNN_K)
    dst = np.where(nbr.reshape(-1) < 0, src, nbr.reshape(-1))
    return _frozen(np.ascontiguousarray(nodes[src]), np.ascontiguousarray(nodes[dst]))


@functools.lru_cache(maxsize=None)
def state_points(name):
    """N_POINTS points in and 0.4 m around the cluster box, then adversarial_points: on and
    an ulp around every AABB face and corner."""
    rs = np.random.RandomState(3000 + WORLDS.index(name))
    clo, chi = cluster_box(name)
    pad = np.array([0.4, 0.4, 0.0])
    pts = rs.uniform(clo - pad, chi + pad, size=(N_POINTS, 3))
    return _frozen(np.ascontiguousarray(np.vstack([pts, adversarial_points(world(name)[1])])))


# ---- the oracle's answers (computed once, shared, read-only) ---------------------------------
@functools.lru_cache(maxsize=None)
def exp_motions(name, mode, can_pass):
    _, rg, ro = setup(name)
    s1, s2 = motion_edges(name)
    return _frozen(O.check_motions(world(name)[1], rg, ro, s1, s2, bool(can_pass), mode, threads=8))


@functools.lru_cache(maxsize=None)
def exp_knn_motions(name, mode, can_pass):
    _, rg, ro = setup(name)
    s1, s2 = knn_table_edges(name)
    return _frozen(O.check_motions(world(name)[1], rg, ro, s1, s2, bool(can_pass), mode, threads=8))


@functools.lru_cache(maxsize=None)
def exp_states(name, can_pass):
    _, rg, ro = setup(name)
    return _frozen(O.check_states(world(name)[1], rg, ro, state_points(name), bool(can_pass), threads=8))


@functools.lru_cache(maxsize=None)
def exp_mindist(name):
    return _frozen(O.check_states_mindist(world(name)[1], state_points(name), MIN_DISTANCE))
