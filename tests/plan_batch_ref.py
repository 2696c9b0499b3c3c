"""A plain reference of the batched planner's device stages (csrc/plan_batch.hip): numpy
plus the oracle's state and motion checks.

For one batch (what epp_dbg_plan_batch takes) it computes per problem: the samples, their
validity, the nodes (start, goal, the valid samples in order), the queries (the nodes inside
the row ellipsoid), every query's exact k-NN row over all of the problem's nodes, the
outcome of pb_query_row's control flow (which radius, which ranking branch, or which exit),
the masked row, the referenced nodes and the words the emit writes from them.

Only pb_query_row's *control flow* is restated (radius growth, the ellipsoid gate, the list
capacity, the branch taken); the row itself comes from the exact k-NN (knn_ref.knn_row), so a
ranking branch that orders or cuts wrongly disagrees with it.

compare() checks an emitted block against the reference, rows keyed by their node (the order
of a problem's rows depends on the order of k_pb_compact's atomics).
"""
import numpy as np

import oracle as O
from eppamd import synth

from knn_ref import knn_row

NONE16 = 0xFFFF
K_CAP = 512  # pb_query_row's list capacity
BRANCHES = ("lane", "bisect_lane", "bisect_lds", "rank_all")
EXITS = ("gate", "overflow", "rounds")


def ellipse(nodes, s, g):
    """pb_ellipse: |x - s| + |x - g| in its operation order."""
    ds = nodes - s
    dg = nodes - g
    a = np.sqrt((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2])
    b = np.sqrt((dg[:, 0] * dg[:, 0] + dg[:, 1] * dg[:, 1]) + dg[:, 2] * dg[:, 2])
    return a + b


def grid_cell(q, ns):
    """k_pb_sample's cell-count loop: (h_eff, dims)."""
    l_cap = max(64, ns + 2)  # knn_layout(ns + 2).cap
    h = float(q["h"])
    while True:
        dims = [int(min((float(q["ghi"][d]) - float(q["glo"][d])) / h, 1023.0)) + 1 for d in range(3)]
        if dims[0] * dims[1] * dims[2] <= l_cap:
            return h, dims
        h *= 1.25


def query_outcome(d2, self_i, f, gbound, h_eff, K):
    """pb_query_row's control flow for one query: d2 = its squared distances to every node.
    Returns (outcome, rounds, count, margin, gate_margin): outcome one of BRANCHES or EXITS,
    rounds the radii tried, count the last list's length, margin the smallest relative
    distance of a candidate to a threshold that decided (a radius r^2 or a bisection
    midpoint), gate_margin the smallest distance of the ellipsoid gate's sum to gbound."""
    other = np.ones(len(d2), bool)
    other[self_i] = False
    dd = d2[other]
    r = 1.6 * h_eff
    margin = np.inf
    gate_margin = np.inf
    cnt = 0
    for it in range(4):
        lhs = f + 2.0 * r * (1.0 + 1e-9) + 1e-9
        gate_margin = min(gate_margin, abs(lhs - gbound))
        if not (lhs <= gbound):
            return "gate", it + 1, cnt, margin, gate_margin
        b2 = r * r
        margin = min(margin, float(np.min(np.abs(dd - b2))) / b2)
        cnt = int(np.count_nonzero(dd <= b2))
        if cnt > K_CAP:
            return "overflow", it + 1, cnt, margin, gate_margin
        if cnt < K:
            r *= 1.5
            continue
        if cnt <= 64:
            return "lane", it + 1, cnt, margin, gate_margin
        if cnt > 256:
            return "rank_all", it + 1, cnt, margin, gate_margin
        lst = dd[dd <= b2]
        lo, hi = 0.0, b2
        for _ in range(10):
            mid = 0.5 * (lo + hi)
            margin = min(margin, float(np.min(np.abs(lst - mid))) / mid)
            if np.count_nonzero(lst <= mid) >= K:
                hi = mid
            else:
                lo = mid
        m = int(np.count_nonzero(lst <= hi))
        return ("bisect_lane" if m <= 64 else "bisect_lds"), it + 1, cnt, margin, gate_margin
    return "rounds", 4, cnt, margin, gate_margin


def problem_ref(world, can_pass, lo, hi, ns, k, q):
    """One problem of a batch.  world = (w, r_gate, r_obst) of the oracle."""
    w, rg, ro = world
    s, g = np.asarray(q["s"], float), np.asarray(q["g"], float)
    xyz = synth.sample_states(int(q["seed"]), lo, hi, ns)
    valid = O.check_states(w, rg, ro, xyz, can_pass).astype(bool)
    nodes = np.ascontiguousarray(np.vstack([s, g, xyz[valid]]))
    n = len(nodes)
    out = dict(nodes=nodes, n=n, valid=valid, cap=max(0, int(q["cap"])), queries=np.zeros(0, np.int64), rows={},
               outcome={}, info={}, thr_margin=np.inf)
    if out["cap"] == 0:
        return out
    f = ellipse(nodes, s, g)
    thr = float(q["bound"]) * (1.0 + 1e-8) + 1e-6
    out["thr_margin"] = float(np.min(np.abs(f - thr)))
    queries = np.nonzero(f <= thr)[0]
    h_eff, dims = grid_cell(q, ns)
    out.update(queries=queries, h_eff=h_eff, dims=dims, f=f)
    rows = {}
    for i in queries:
        row, d2 = knn_row(nodes, int(i), k)
        oc = query_outcome(d2, int(i), float(f[i]), float(q["gbound"]), h_eff, k)
        out["outcome"][int(i)] = oc[0]
        out["info"][int(i)] = oc[1:]
        if oc[0] in EXITS:
            row = np.full(k, -1, np.int32)
        rows[int(i)] = row
    # the motion check of every row entry at once
    qi = np.array(sorted(rows), np.int64)
    tab = np.array([rows[int(i)] for i in qi], np.int64).reshape(len(qi), k)
    src = np.repeat(qi, k)
    dst = tab.reshape(-1)
    ok = np.zeros(len(dst), bool)
    have = dst >= 0
    if have.any():
        ok[have] = O.check_motions(w, rg, ro, nodes[src[have]], nodes[dst[have]], can_pass, 0).astype(bool)
    masked = np.where(ok, dst, -1).reshape(len(qi), k)
    out["rows"] = {int(i): masked[r].astype(np.int64) for r, i in enumerate(qi)}
    out["motions"] = (int(np.count_nonzero(ok)), int(np.count_nonzero(have & ~ok)))
    return out


def batch_ref(world, can_pass, lo, hi, ns, k, segs):
    return [problem_ref(world, can_pass, np.asarray(lo, float), np.asarray(hi, float), ns, k, q) for q in segs]


def expected_words(ref, k):
    """The determined case (queries <= cap) of one problem: its header values (queries, kept,
    goal, nodes, need, inexact), the referenced nodes (node ids, ascending) and per query its
    (compact index, row in compact indices, 0xFFFF none)."""
    if ref["cap"] == 0:
        return dict(hdr=(0, 0, 0, ref["n"], 0, 0), need=np.zeros(0, np.int64), rows={})
    marked = set(int(i) for i in ref["queries"])
    kept = goal = 0
    for i, row in ref["rows"].items():
        for j in row:
            if j >= 0:
                marked.add(int(j))
                kept += 1
                goal += int(j) == 1
    need = np.array(sorted(marked), np.int64)
    index = {int(v): c for c, v in enumerate(need)}
    rows = {i: (index[i], np.array([index[int(j)] if j >= 0 else NONE16 for j in row], np.uint16))
            for i, row in ref["rows"].items()}
    inexact = int(any(o in EXITS for o in ref["outcome"].values()))
    return dict(hdr=(len(ref["queries"]), kept, goal, ref["n"], len(need), inexact), need=need, rows=rows)


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compare(em, refs, k):
    """Asserts that the emitted block em (capi.dbg_plan_batch) is what the reference gives.
    Every comparison is an equality."""
    S = len(refs)
    hdr = em["hdr"].astype(np.int64)

    def hv(field, p):
        return int(hdr[3 + field * S + p])

    first = 0
    for p, ref in enumerate(refs):
        tagp = f"problem {p}"
        # the nodes: sample, state check, ordered compaction
        assert hv(3, p) == ref["n"], f"{tagp}: node count {hv(3, p)} != {ref['n']}"
        assert _same_bits(em["nodes"][p], ref["nodes"]), f"{tagp}: node list differs"
        nq = len(ref["queries"])
        assert hv(0, p) == nq, f"{tagp}: queries {hv(0, p)} != {nq}"
        nrow = min(nq, ref["cap"])
        sl = em["slots"][first:first + nrow].astype(np.int64)
        rw = em["rows"][first:first + nrow]
        first += nrow
        assert np.all(sl >> 16 == p), f"{tagp}: a slot names another problem"
        cidx = sl & 0xFFFF
        no, nc = int(em["need_off"][p]), int(em["need_cap"][p])
        nneed = hv(4, p)
        assert 0 <= nneed <= nc, f"{tagp}: referenced nodes {nneed} outside the capacity {nc}"
        need_xyz = em["need"][no:no + nneed]
        if nq <= ref["cap"]:  # fully determined
            exp = expected_words(ref, k)
            got_hdr = tuple(hv(fld, p) for fld in range(6))
            assert got_hdr == exp["hdr"], f"{tagp}: header {got_hdr} != {exp['hdr']}"
            assert _same_bits(need_xyz, ref["nodes"][exp["need"]]), f"{tagp}: referenced coordinates differ"
            by_c = {c: (i, row) for i, (c, row) in exp["rows"].items()}
            assert len(set(cidx.tolist())) == nrow, f"{tagp}: a row's node is listed twice"
            for r in range(nrow):
                c = int(cidx[r])
                assert c in by_c, f"{tagp}: row {r} names compact index {c}, not a query"
                i, row = by_c[c]
                assert np.array_equal(rw[r], row), (
                    f"{tagp}: row of node {i} ({ref['outcome'][i]}, {ref['info'][i][:2]}): "
                    f"{rw[r].tolist()} != {row.tolist()}")
        else:  # which queries were listed is not determined: resolve through the coordinates
            assert nrow == ref["cap"]
            key = {ref["nodes"][i].tobytes(): i for i in range(ref["n"])}
            assert len(key) == ref["n"], "inputs of a capped problem need distinct coordinates"
            assert np.all(cidx < nneed), f"{tagp}: a slot's index is past the referenced nodes"
            node_of = np.array([key.get(need_xyz[c].tobytes(), -1) for c in range(nneed)], np.int64)
            assert np.all(node_of >= 0), f"{tagp}: a referenced coordinate is no node"
            listed = node_of[cidx]
            assert len(set(listed.tolist())) == nrow, f"{tagp}: a row's node is listed twice"
            used = set(listed.tolist())
            kept = goal = 0
            inexact = 0
            for r in range(nrow):
                i = int(listed[r])
                assert i in ref["rows"], f"{tagp}: row {r} names node {i}, not a query"
                ent = rw[r].astype(np.int64)
                assert np.all((ent == NONE16) | (ent < nneed)), f"{tagp}: row of node {i} has an index past the list"
                got = np.where(ent == NONE16, -1, node_of[np.minimum(ent, max(nneed - 1, 0))])
                assert np.array_equal(got, ref["rows"][i]), (
                    f"{tagp}: row of node {i} ({ref['outcome'][i]}): {got.tolist()} != {ref['rows'][i].tolist()}")
                used.update(int(j) for j in got if j >= 0)
                kept += int(np.count_nonzero(got >= 0))
                goal += int(np.count_nonzero(got == 1))
                inexact |= int(ref["outcome"][i] in EXITS)
            assert node_of.tolist() == sorted(used), f"{tagp}: referenced nodes are not the rows' nodes in node order"
            assert (hv(1, p), hv(2, p), hv(5, p)) == (kept, goal, inexact), f"{tagp}: kept / goal / inexact words"
    assert int(hdr[1]) == first, f"rows word {int(hdr[1])} != {first}"
    assert np.all(em["done"] == em["seq"]), "a completion slot does not hold the launch's seq"


def emitted_equal(a, b, refs, k):
    """Two emitted blocks of one batch hold the same result (rows keyed by node: positions
    may differ).  Both have passed compare(); what is left is the capped problems' choice
    of rows, which may differ, so only the determined parts are compared word for word."""
    S = len(refs)
    words = [1] + list(range(3, 3 + 6 * S))
    if all(len(r["queries"]) <= r["cap"] for r in refs):
        assert np.array_equal(a["hdr"][words], b["hdr"][words])
    first = 0
    for p, ref in enumerate(refs):
        nrow = min(len(ref["queries"]), ref["cap"])
        if len(ref["queries"]) <= ref["cap"]:
            oa = np.argsort(a["slots"][first:first + nrow], kind="stable")
            ob = np.argsort(b["slots"][first:first + nrow], kind="stable")
            assert np.array_equal(a["slots"][first:first + nrow][oa], b["slots"][first:first + nrow][ob])
            assert np.array_equal(a["rows"][first:first + nrow][oa], b["rows"][first:first + nrow][ob])
            no, nn = int(a["need_off"][p]), int(a["hdr"][3 + 4 * S + p])
            assert _same_bits(a["need"][no:no + nn], b["need"][no:no + nn])
        assert _same_bits(a["nodes"][p], b["nodes"][p])
        first += nrow
