"""Worlds, k-NN tables, packed rows and prefills of the tests of k_motions_v5's MotionMask tail
(test_gpu_knn_mask.py on the device, test_knn_mask_inputs_cpu.py for the inputs themselves;
knn_mask_ref.py restates the tail).

Worlds: the cluttered worlds of tile_shape_inputs that reach another tile shape each -- n40
(W 2), n180 (W 4, S 32), n700 (W 2, S 16), n520 (W 16, S 32), n600 (W 32), the gate cluster
(W 4, fillings: can_pass_gate matters) -- and plan_batch_inputs' c1 world (W 1, S 64).

Two kinds of special nodes make the answers of chosen edges certain without the oracle (the
CPU test then confirms them with it): "sky" nodes above every inflated AABB, between which
every edge is valid, and "inside" nodes in the interior of a solid OBB, from or into which
every edge fails.

The masked entry's tables (masked_case) have m = n k = 3 * 1024 + 37 entries -- 3109 is prime,
so that table is n = 3109 rows of k = 1 -- and, at the planner's k = 8, 389 rows (3 * 1024 + 40
entries).  Either way four workgroups with a ragged last wave; the 1024 edges of workgroup 1
start at inside nodes, so that workgroup's share of every counter is 0.

The rows entry's cases (rows_case) pack rows of up to 64 problems, global node ids
p << 16 | node as in the product: interleaved so that one wave's 64 edges mix problems, ids
not ascending, rows of problem 63, edges into node 1 (the goal) of every problem, one edge
into global id 1 from a row of problem 2, a row whose every edge fails, a row of -1 only.

Everything is input data and oracle output: built once per process, shared, read-only.
"""
import ctypes as C
import functools

import numpy as np

import oracle as O
from eppamd import capi, config, synth

from conftest import CONFIG

import plan_batch_inputs as PB
import tile_shape_inputs as T
from knn_ref import knn_ref

C1 = "c1"
WORLDS = (C1, "n40", "n180", "n700", "n520", "n600", T.GATE_CLUSTER)

BLOCK = 1024                      # k_motions_v5's workgroup: 1024 consecutive edges
SMALL_MOTIONS = 1024              # kSmallMotions: at most so many edges (<= 256 OBBs) are the small path's
M_EDGES = 3 * BLOCK + 37          # 3109, a prime
LAYOUTS = {"k1": (M_EDGES, 1), "k8": (389, 8)}
assert LAYOUTS["k8"][0] * 8 == 3 * BLOCK + 40
FAIL_WG = 1                       # the workgroup whose edges all fail: edges [1024, 2048)
TARGET = 1                        # the planner's target: node 1, the goal

NS_LOG = 16                       # the product's: node ids p << 16 | node
NLOC = T.KNN_NODES                # nodes per problem that hold a position (640)
LOC_GOAL, LOC_SKY, LOC_INSIDE, LOC_FAIL0 = 1, 2, 3, 4  # per problem: node 1 and 2 sky, 3 inside,
N_FAIL = 128                                           # 4 .. 131 inside (the all-fail workgroup's rows)
LOC_ORD0 = LOC_FAIL0 + N_FAIL     # 132 .. 639: the base table's nodes
COLUMN_NODES = np.arange(300, 340)  # gate cluster: base nodes in tile_shape_inputs.GATE_COLUMN
ROT = 37                       # problem p's ordinary node l is base node (l + ROT p) % NLOC
MAX_PROB = 64
COUNTERS = MAX_PROB + 2           # pkept / pgoal slots the tests hold: two past the largest nprob


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# ---- worlds -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(name):
    """(OBBs for capi.World, the oracle's world, r_gate, r_obstacle)."""
    if name == C1:
        ref, rg, ro = PB.world()
        gates, obstacles, _, _ = synth.c1_world()
        obbs = capi.build_obbs(config.geometry(config.load(CONFIG)), gates, obstacles)
        assert len(obbs) == len(ref)
        return _frozen(obbs), ref, rg, ro
    _, rg, ro = T.setup(name)
    obbs, ref = T.world(name)
    return obbs, ref, rg, ro


def device_world(name):
    obbs, _, rg, ro = world(name)
    return capi.World(obbs, rg, ro)


def empty_world():
    """A world without OBBs: no tile tables, so neither entry can run on it."""
    _, _, rg, ro = world(C1)
    return capi.World(np.zeros(0, capi.OBB_DTYPE), rg, ro)


@functools.lru_cache(maxsize=None)
def shape(name):
    """tile_shape_inputs.shape for any world here: n, T, W, S, tile_words and k_motions_v5's
    dynamic LDS, from the host-only index build."""
    obbs, _, rg, ro = world(name)
    f = capi.lib().epp_dbg_build_blob
    f.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]
    f.restype = C.c_int32
    out = np.zeros(6)
    capi.check(f(obbs.ctypes.data, len(obbs), rg, ro, 1, out.ctypes.data))
    n, t, tw, w, s = len(obbs), int(out[2]), int(out[3]), int(out[4]), int(out[5])
    return {"n": n, "T": t, "W": w, "S": s, "tile_words": tw, "lds": T.tile_lds_bytes(n, t, tw)}


def _box(name):
    """(lo, hi): x / y of the patch the nodes concentrate on, z over every inflated AABB."""
    _, ref, _, _ = world(name)
    if name == C1:
        lo, hi = (b.copy() for b in synth.C1_BOUNDS)
    else:
        lo, hi = T.cluster_box(name)
    lo[2], hi[2] = ref["aabb_lo"][:, 2].min(), ref["aabb_hi"][:, 2].max()
    return lo, hi


def sky_points(name, rs, n):
    """Points above every inflated AABB: an edge between two of them is valid."""
    lo, hi = _box(name)
    p = rs.uniform(lo, hi, size=(n, 3))
    p[:, 2] = hi[2] + rs.uniform(0.3, 0.6, n)
    return p


def inside_points(name, rs, n):
    """Points in the interior of a solid (not filling) OBB, within 0.8 of its half extents:
    an edge from or into one fails, whatever can_pass_gate is."""
    _, ref, _, _ = world(name)
    solid = np.flatnonzero(ref["filling"] == 0)
    o = ref[solid[rs.randint(0, len(solid), n)]]
    local = rs.uniform(-0.8, 0.8, (n, 3)) * o["half"]
    return o["center"] + np.einsum("nij,nj->ni", o["rot"].reshape(n, 3, 3), local)


@functools.lru_cache(maxsize=None)
def base_table(name):
    """(nodes (NLOC, 3), nbr (NLOC, 8)): tile_shape_inputs.knn_table; for c1 the same recipe on
    nodes uniform in its bounds."""
    if name == T.GATE_CLUSTER:
        # COLUMN_NODES of the nodes moved into the column that only openings fill, their rows
        # pointing at each other: edges that are valid only when the gates may be passed
        rs = np.random.RandomState(2998)
        nodes, nbr = (a.copy() for a in T.knn_table(name))
        nodes[COLUMN_NODES] = rs.uniform(*T.GATE_COLUMN, size=(len(COLUMN_NODES), 3))
        nbr[COLUMN_NODES] = COLUMN_NODES[rs.randint(0, len(COLUMN_NODES), (len(COLUMN_NODES), T.KNN_K))]
        return _frozen(nodes, nbr)
    if name != C1:
        return T.knn_table(name)
    rs = np.random.RandomState(2999)
    nodes = np.ascontiguousarray(rs.uniform(*synth.C1_BOUNDS, size=(NLOC, 3)))
    nbr = knn_ref(nodes, T.KNN_K)
    u = rs.rand(NLOC, T.KNN_K)
    nbr = np.where(u < 0.10, rs.randint(0, NLOC, size=nbr.shape), nbr)
    nbr = np.where(u > 0.95, -1, nbr).astype(np.int32)
    return _frozen(nodes, np.ascontiguousarray(nbr))


# ---- the masked entry's tables ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked_case(name, layout):
    """dict(nodes (n, 3), nbr (n, k), target, fail_row, empty_row, sky_rows): the base table
    cut (k = 8) or unrolled (k = 1: row i is entry i // NLOC of base row i % NLOC, the nodes
    past the first NLOC jittered copies) to n rows, then
      rows of workgroup FAIL_WG   inside nodes: its 1024 edges all fail;
      fail_row                    an inside node with k real entries, one of them the target;
      empty_row                   -1 only;
      sky_rows                    sky nodes, the target among them, each with an entry equal to
                                  the target: kept edges into it, in the first and the last
                                  workgroup (the ragged wave) and in the one after FAIL_WG;
      a dozen more entries equal to the target, from ordinary rows and from the all-fail rows."""
    n, k = LAYOUTS[layout]
    assert n * k > SMALL_MOTIONS
    rs = np.random.RandomState(4000 + 10 * WORLDS.index(name) + k)
    bn, bnbr = base_table(name)
    i = np.arange(n)
    nodes = bn[i % NLOC] + np.where(i[:, None] >= NLOC, rs.uniform(-0.02, 0.02, (n, 3)), 0.0)
    if k == 8:
        nbr = np.where(bnbr[:n] < 0, -1, bnbr[:n] % n).astype(np.int32)
    else:
        nbr = bnbr[i % NLOC, (i // NLOC) % T.KNN_K].reshape(n, 1).astype(np.int32)
    r0, r1 = FAIL_WG * BLOCK // k, (FAIL_WG + 1) * BLOCK // k
    nodes[r0:r1] = inside_points(name, rs, r1 - r0)
    fail_row, empty_row = 5, 7
    nodes[fail_row] = inside_points(name, rs, 1)[0]
    nbr[fail_row] = rs.randint(8, r0, k)
    nbr[fail_row, 0] = TARGET
    nbr[empty_row] = -1
    sky_rows = np.array([TARGET, 2, 3, r1 + 3, n - 2, n - 1])
    nodes[sky_rows] = sky_points(name, rs, len(sky_rows))
    nbr[sky_rows[1:], np.arange(len(sky_rows) - 1) % k] = TARGET
    free = np.setdiff1d(np.arange(8, n), np.concatenate([np.arange(r0, r1), sky_rows]))
    pick = rs.choice(free, 10, replace=False)
    nbr[pick, rs.randint(0, k, 10)] = TARGET
    nbr[[r0 + 1, r1 - 1], [0, k - 1]] = TARGET
    return dict(nodes=_frozen(np.ascontiguousarray(nodes)), nbr=_frozen(np.ascontiguousarray(nbr)), target=TARGET,
                fail_row=fail_row, empty_row=empty_row, sky_rows=_frozen(sky_rows))


def table_edges(nodes, nbr):
    """The edges a table denotes, as epp_knn_edges lays them out: edge i k + c from node i to
    node nbr[i, c], a missing neighbour (-1) the degenerate edge from the node to itself."""
    n, k = nbr.shape
    src = np.repeat(np.arange(n), k)
    j = nbr.reshape(-1)
    return nodes[src], nodes[np.where(j < 0, src, j)]


@functools.lru_cache(maxsize=None)
def masked_flags(name, layout, can_pass):
    """The oracle's answer (mode 0) on the table's edges."""
    _, ref, rg, ro = world(name)
    c = masked_case(name, layout)
    s1, s2 = table_edges(c["nodes"], c["nbr"])
    return _frozen(O.check_motions(ref, rg, ro, s1, s2, bool(can_pass), 0, threads=8))


def masked_prefill(case, counters):
    """What every output holds before the call; counters: the two counts."""
    m = case["nbr"].size
    return dict(valid=np.full(m, 0xA5, np.uint8), out16=np.full(m, 0xBEEF, np.uint16),
                count=np.array(counters, np.int64))


COUNTER_PREFILLS = ((0, 0), (7, 1 << 40))


# ---- the rows entry's cases -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem_nodes(name):
    """(MAX_PROB, NLOC, 3): the position of node l of problem p.  Ordinary nodes are the base
    table's, rotated by ROT per problem (so the same local id is another point in every
    problem); nodes 0 .. 2 are sky points, LOC_INSIDE and the N_FAIL after it inside points."""
    rs = np.random.RandomState(5000 + WORLDS.index(name))
    bn, _ = base_table(name)
    pos = np.stack([np.roll(bn, -ROT * p, axis=0) for p in range(MAX_PROB)])
    pos[:, :LOC_INSIDE] = sky_points(name, rs, MAX_PROB * LOC_INSIDE).reshape(MAX_PROB, LOC_INSIDE, 3)
    pos[:, LOC_INSIDE:LOC_ORD0] = inside_points(name, rs, MAX_PROB * (1 + N_FAIL)).reshape(MAX_PROB, 1 + N_FAIL, 3)
    return _frozen(np.ascontiguousarray(pos))


def node_positions(name, ids):
    """Positions of global node ids p << NS_LOG | l."""
    ids = np.asarray(ids, np.int64)
    return problem_nodes(name)[ids >> NS_LOG, ids & ((1 << NS_LOG) - 1)]


# name: nprob, cap, k, rows_n; the outputs left out (NULL)
ROWS_CASES = {
    "p1": dict(nprob=1, cap=389, k=8, rows_n=389),
    "p3": dict(nprob=3, cap=389, k=8, rows_n=389),
    "p64": dict(nprob=64, cap=389, k=8, rows_n=389),
    "p3_rows0": dict(nprob=3, cap=389, k=8, rows_n=0),
    "p3_rows1": dict(nprob=3, cap=389, k=8, rows_n=1),
    "p3_rows_cap_m1": dict(nprob=3, cap=389, k=8, rows_n=388),
    "p3_rows_cap_p5": dict(nprob=3, cap=389, k=8, rows_n=394),
    "k4_below_1024": dict(nprob=3, cap=255, k=4, rows_n=255),
    "k8_at_1024": dict(nprob=3, cap=128, k=8, rows_n=128),
    "k16_above_1024": dict(nprob=3, cap=65, k=16, rows_n=65),
    "p3_no_count": dict(nprob=3, cap=389, k=8, rows_n=389, without=("count",)),  # (the product's call)
    "p3_no_out16": dict(nprob=3, cap=389, k=8, rows_n=389, without=("out16", "mark")),
    "p1_no_mark": dict(nprob=1, cap=389, k=8, rows_n=389, without=("mark",)),
}
assert 255 * 4 < BLOCK == 128 * 8 < 65 * 16


@functools.lru_cache(maxsize=None)
def rows_table(name, nprob, cap, k):
    """dict(rows32 (cap, k), ids32 (cap,), goal_rows (per problem), fail_row, empty_row,
    cross (row, column) or None, fail_block (r0, r1) or None).

    Row r belongs to problem (7 r + r // 5) % nprob -- consecutive rows, and so the 64 edges of
    a wave, differ in problem -- and is an ordinary node drawn without order; its entries are
    the base table's row in that problem's numbering.  Then, by row:
      fail_block   cap k >= 2048: the rows of workgroup FAIL_WG are inside nodes;
      goal_rows    per problem its first row outside the block: node LOC_SKY, entry 0 its goal
                   p << 16 | 1 (both sky: a kept edge into the goal);
      cross        nprob >= 3: entry 1 of problem 2's goal row is global id 1, problem 0's goal.
                   Its low bits are 1, so it counts for pgoal[2]; it is entry == target (1) for
                   count[1], which the goals of problems > 0 are not;
      fail_row     node LOC_INSIDE with k real entries: every edge fails, the node is marked;
      empty_row    -1 only;
      20 entries of ordinary rows point at their problem's goal."""
    rs = np.random.RandomState(6000 + 100 * WORLDS.index(name) + 10 * nprob + k)
    _, bnbr = base_table(name)
    r = np.arange(cap)
    prob = (7 * r + r // 5) % nprob
    n_ord = NLOC - LOC_ORD0
    loc = LOC_ORD0 + rs.permutation(n_ord)[:cap]
    b = bnbr[(loc + ROT * prob) % NLOC][:, :k] if k <= T.KNN_K else np.concatenate(
        [bnbr[(loc + ROT * prob) % NLOC], bnbr[(loc + 1 + ROT * prob) % NLOC]], axis=1)[:, :k]
    ent = np.where(b < 0, -1, (b - ROT * prob[:, None]) % NLOC)

    def ordinary(shape):
        return LOC_ORD0 + rs.randint(0, n_ord, shape)

    block = None
    special = np.zeros(cap, bool)
    if cap * k >= (FAIL_WG + 1) * BLOCK:
        r0, r1 = FAIL_WG * BLOCK // k, (FAIL_WG + 1) * BLOCK // k
        assert r1 - r0 <= N_FAIL
        block = (r0, r1)
        loc[r0:r1] = LOC_FAIL0 + np.arange(r1 - r0)
        ent[r0:r1] = np.where(rs.rand(r1 - r0, k) < 0.1, -1, ordinary((r1 - r0, k)))
        special[r0:r1] = True
    goal_rows = []
    for p in range(nprob):
        g = int(np.flatnonzero((prob == p) & ~special)[0])
        goal_rows.append(g)
        special[g] = True
        loc[g] = LOC_SKY
        ent[g] = ordinary(k)
        ent[g, 0] = LOC_GOAL
    rest = np.flatnonzero(~special)
    fail_row, empty_row = int(rest[len(rest) // 3]), int(rest[2 * len(rest) // 3])
    special[[fail_row, empty_row]] = True
    loc[fail_row] = LOC_INSIDE
    ent[fail_row] = ordinary(k)
    ent[empty_row] = -1
    pick = rs.choice(np.flatnonzero(~special), 20, replace=False)
    ent[pick, rs.randint(0, k, 20)] = LOC_GOAL
    ids32 = (prob << NS_LOG | loc).astype(np.int32)
    rows32 = np.where(ent < 0, -1, prob[:, None] << NS_LOG | ent).astype(np.int32)
    cross = None
    if nprob >= 3:
        cross = (goal_rows[2], 1)
        rows32[cross] = 1
    assert len(np.unique(ids32)) == cap
    return dict(rows32=_frozen(rows32), ids32=_frozen(ids32), goal_rows=tuple(goal_rows), fail_row=fail_row,
                empty_row=empty_row, cross=cross, fail_block=block)


def rows_case(name, case):
    """ROWS_CASES[case] on world `name`: the table of rows_table, rows_n, target and which
    outputs are given."""
    c = dict(ROWS_CASES[case])
    without = c.pop("without", ())
    t = rows_table(name, c["nprob"], c["cap"], c["k"])
    return dict(t, **c, target=TARGET, ns_log=NS_LOG, without=tuple(without))


def rows_edges(name, rows32, ids32):
    """The edges of every row, live or not: from node ids32[r] to each entry, -1 to itself."""
    cap, k = rows32.shape
    src = np.repeat(np.asarray(ids32, np.int64), k)
    j = rows32.reshape(-1).astype(np.int64)
    return node_positions(name, src), node_positions(name, np.where(j < 0, src, j))


@functools.lru_cache(maxsize=None)
def rows_flags(name, nprob, cap, k, can_pass):
    """The oracle's answer (mode 0) on the edges of every row of rows_table."""
    _, ref, rg, ro = world(name)
    t = rows_table(name, nprob, cap, k)
    s1, s2 = rows_edges(name, t["rows32"], t["ids32"])
    return _frozen(O.check_motions(ref, rg, ro, s1, s2, bool(can_pass), 0, threads=8))


def rows_prefill(case):
    """What every output holds before the call (None: the case leaves it out).  Every counter
    holds a value of its own; mark holds zeros and, every 97th byte, a 2; it is 64 bytes longer
    than the nprob problems' ids."""
    m = case["cap"] * case["k"]
    mark = np.zeros((case["nprob"] << NS_LOG) + 64, np.uint8)
    mark[::97] = 2
    pre = dict(valid=np.full(m, 0xA5, np.uint8), out16=np.full(m, 0xBEEF, np.uint16),
               count=np.array([7, 1 << 40], np.int64), mark=mark,
               pkept=(1000 + np.arange(COUNTERS)).astype(np.uint64),
               pgoal=((1 << 33) + np.arange(COUNTERS)).astype(np.uint64))
    for name in case["without"]:
        pre[name] = None
    return pre


def upload_problem_nodes(name, buf):
    """The positions of problem_nodes(name) into the device buffer buf (MAX_PROB << NS_LOG
    nodes of 3 doubles, zeroed by the caller once): only the NLOC nodes per problem that hold a
    position are written."""
    pos = problem_nodes(name)
    stride = 24 << NS_LOG
    for p in range(MAX_PROB):
        capi.check(capi.lib().epp_memcpy_h2d(buf.ptr + p * stride, pos[p].ctypes.data, pos[p].nbytes, None))
