"""What k_motions_v5's MotionMask tail must write, restated in numpy from the validity flags.

The flags themselves are the oracle's (knn_mask_inputs); this file is only the tail.  The rule
is the comment block at csrc/motions_tile.hip:36-39 and the MotionMask struct with its comment
at csrc/epp_internal.h:70-89 (CITED below; test_knn_mask_inputs_cpu.py checks that those lines
still say it):

    valid    the flag of every edge; a -1 entry is the degenerate edge from the row's node to
             itself, and has a flag like any other
    keep     = valid & (j >= 0)
    table    where(valid, j, -1): a failed motion's entry becomes -1 (a -1 entry stays -1)
    out16    where(keep, j & 0xFFFF, 0xFFFF): the masked table as u16, 0xFFFF for no edge
    count    [0] += keep.sum(), [1] += (keep & (j == target)).sum(); j the whole entry, so in
             the batch the goal p << ns_log | 1 of a problem p > 0 is not `target` 1
    packed rows (rowmap / rows_n): row r is node ids32[r]; only rows r < min(rows_n, cap) are
             live; everything past them keeps what it held
    marks    mark[ids32[r]] = 1 for every live row, kept edges or none; mark[j] = 1 for every
             kept j; pkept[ids32[r] >> ns_log] += the row's kept edges; pgoal[the same] += those
             of them with (j & (2^ns_log - 1)) == 1 -- the entry's low bits, not its problem:
             an edge from a row of problem 2 into global id 1 counts for pgoal[2]
    untouched   valid / table / out16 of rows that are not live, every other mark byte,
             pkept / pgoal from nprob on; and whatever is NULL is not written

Counts are added to what the counters hold.  Everything is exact: compare() knows no
tolerance.
"""
import numpy as np

# (file, first line, last line): patterns the lines must still match, whitespace-insensitive
CITED = {
    ("csrc/motions_tile.hip", 36, 39): [
        r"MotionMask \(IDX, count or out16 given\)", r"failed motion's table entry becomes -1",
        r"out16 \(if given\) receives the masked table as u16 \(0xFFFF: no edge\)",
        r"count\[0\] / count\[1\] gain the kept edges / those into node `target` \(one atomic per workgroup\)"],
    ("csrc/epp_internal.h", 70, 89): [
        r"failed entries of nbr_w -> -1", r"\+= kept edges / kept edges into node `target`",
        r"Neither count nor out16: no mask", r"struct MotionMask \{",
        r"row r of the table is node rowmap\[r\], and only rows r < \*rows_n are checked",
        r"node ids p << ns_log \| node", r"mark\[row's node\] and mark\[each kept entry\] = 1",
        r"kept edges \(pkept\[p\]\) and those into its node 1, the goal \(pgoal\[p\]\); nprob <= 64",
        r"int32_t ns_log = 0, nprob = 0;"],
}


def _tail(j, valid, target, live, pre, out):
    """The mask, out16 and count of the live entries (flat arrays; live: per entry)."""
    keep = live & (valid != 0) & (j >= 0)
    out["valid"] = np.where(live, valid, pre["valid"]).astype(np.uint8)
    out["table"] = np.where(live & (valid == 0), -1, j).astype(np.int32)
    if pre.get("out16") is not None:
        out["out16"] = np.where(live, np.where(keep, j & 0xFFFF, 0xFFFF), pre["out16"]).astype(np.uint16)
    if pre.get("count") is not None:
        out["count"] = pre["count"] + np.array([keep.sum(), (keep & (j == target)).sum()], np.int64)
    return keep


def masked_ref(nbr, valid, target, pre):
    """check_knn_motions_masked: dict(nbr, valid, out16, count) after the call on the table nbr
    (n, k) whose edges have the flags `valid`, the outputs prefilled with pre."""
    j = nbr.reshape(-1).astype(np.int64)
    out = {}
    _tail(j, np.asarray(valid).reshape(-1), target, np.ones(j.size, bool), pre, out)
    out["nbr"] = out.pop("table").reshape(nbr.shape)
    out.setdefault("out16", None)
    return out


def rows_ref(rows32, ids32, rows_n, valid, target, ns_log, nprob, pre):
    """check_knn_motions_rows: dict(rows32, ids32, rows_n, valid, out16, count, mark, pkept,
    pgoal) after the call; valid: the flags of every row's edges (those of rows that are not
    live are not used); pre: the prefill, None for an output that is not given.  Without mark
    the per-problem counters are not written either."""
    cap, k = rows32.shape
    j = rows32.reshape(-1).astype(np.int64)
    n_live = min(max(int(rows_n), 0), cap)
    live = np.repeat(np.arange(cap) < n_live, k)
    out = dict(ids32=np.array(ids32, np.int32), rows_n=np.array([rows_n], np.int64))
    keep = _tail(j, np.asarray(valid).reshape(-1), target, live, pre, out)
    out["rows32"] = out.pop("table").reshape(cap, k)
    for name in ("out16", "count"):
        out.setdefault(name, None)
    out["mark"] = None
    out["pkept"], out["pgoal"] = pre["pkept"], pre["pgoal"]
    if pre.get("mark") is not None:
        mark = pre["mark"].copy()
        mark[np.asarray(ids32, np.int64)[:n_live]] = 1
        mark[j[keep]] = 1
        prob = np.repeat(np.asarray(ids32, np.int64) >> ns_log, k)
        goal = keep & ((j & ((1 << ns_log) - 1)) == 1)
        assert (prob[keep] < nprob).all()
        out["mark"] = mark
        out["pkept"] = pre["pkept"] + np.bincount(prob[keep], minlength=len(pre["pkept"])).astype(np.uint64)
        out["pgoal"] = pre["pgoal"] + np.bincount(prob[goal], minlength=len(pre["pgoal"])).astype(np.uint64)
    return out


def compare(got, exp):
    """[] when every output of got equals exp's, whole; else one line per output that differs."""
    bad = []
    for name, e in exp.items():
        g = got.get(name)
        if e is None or g is None:
            if e is not None or g is not None:
                bad.append(f"{name}: {'missing' if g is None else 'unexpected'}")
            continue
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape or g.dtype != e.dtype:
            bad.append(f"{name}: shape / type {g.shape} {g.dtype}, expected {e.shape} {e.dtype}")
            continue
        d = np.flatnonzero(g.reshape(-1) != e.reshape(-1))
        if len(d):
            bad.append(f"{name}: {len(d)} of {e.size} differ; first at {d[:8].tolist()}: got "
                       f"{g.reshape(-1)[d[:8]].tolist()}, expected {e.reshape(-1)[d[:8]].tolist()}")
    return bad
