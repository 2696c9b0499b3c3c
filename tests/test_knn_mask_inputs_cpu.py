"""The inputs and the restatement of test_gpu_knn_mask.py, checked without a GPU: the cited
source lines still state the rule knn_mask_ref restates, every case has the properties it is
named for (from the oracle's flags alone), and the comparison rejects each mistake the GPU test
is meant to catch.

Run with -s to see the shapes and the valid / kept shares.
"""
import os
import re

import numpy as np
import pytest

import knn_mask_inputs as I
import knn_mask_ref as R

from conftest import PKG

MASKED = [(name, layout, cp) for name in I.WORLDS for layout in I.LAYOUTS for cp in (0, 1)]


def test_cited_lines_still_state_the_rule():
    for (path, first, last), patterns in R.CITED.items():
        lines = open(os.path.join(PKG, path)).read().split("\n")[first - 1:last]
        text = " ".join(re.sub(r"^\s*//\s?", "", ln).strip() for ln in lines)
        text = re.sub(r"\s+", " ", text)
        for pat in patterns:
            assert re.search(pat, text), (path, first, last, pat)
    # the numbers restated in knn_mask_inputs
    src = open(os.path.join(PKG, "csrc", "motions_tile.hip")).read()
    assert re.search(r"__launch_bounds__\(1024\) void k_motions_v5", src) and I.BLOCK == 1024
    assert re.search(r"__shared__ uint32_t s_pcnt\[2\]\[64\];", src) and I.MAX_PROB == 64
    m = re.search(r"kSmallMotions = (\d+);", open(os.path.join(PKG, "csrc", "collision_common.h")).read())
    assert m and int(m.group(1)) == I.SMALL_MOTIONS


def test_worlds_reach_their_tile_shapes_and_fit_the_lds():
    """c1 is W = 1, S = 64; the others are the shapes test_tile_shape_inputs_cpu.py asserts.
    All fit the tile kernel's LDS, so knn_motions_rows_supported must be true on each."""
    want = {I.C1: (1, 64), "n40": (2, 64), "n180": (4, 32), "n700": (2, 16), "n520": (16, 32), "n600": (32, 64)}
    print()
    for name in I.WORLDS:
        s = I.shape(name)
        print(f"{name:6s} n={s['n']:4d} T={s['T']:2d} W={s['W']:2d} S={s['S']:2d} LDS={s['lds']:7,d} bytes")
        assert 0 < s["lds"] <= 150 * 1024, name
        if name in want:
            assert (s["W"], s["S"]) == want[name], (name, s)
    g = I.shape("gates")
    assert g["W"] >= 4 and int(I.world("gates")[1]["filling"].sum()) == 24
    assert I.shape(I.C1)["T"] == 1 and I.shape(I.C1)["n"] <= 256  # (the small path's world)


def _wg_sums(x, block=I.BLOCK):
    return np.add.reduceat(x.astype(np.int64), np.arange(0, len(x), block))


@pytest.mark.parametrize("name,layout,can_pass", MASKED)
def test_masked_case_has_its_properties(name, layout, can_pass):
    c = I.masked_case(name, layout)
    nbr, tgt = c["nbr"], c["target"]
    n, k = nbr.shape
    m = n * k
    assert (n, k) == I.LAYOUTS[layout] and m > I.SMALL_MOTIONS and m < 4000
    if layout == "k1":
        assert m == 3 * 1024 + 37
    assert m // 1024 == 3 and 0 < m % 64 < 64  # four workgroups, a ragged last wave
    assert nbr.min() == -1 and nbr.max() < n and (nbr == -1).sum() >= 10
    v = I.masked_flags(name, layout, can_pass).astype(bool)
    j = nbr.reshape(-1)
    keep = v & (j >= 0)
    print(f"\n{name} {layout} can_pass={can_pass}: valid {v.mean():.1%}, kept per workgroup {_wg_sums(keep).tolist()}, "
          f"into target {_wg_sums(keep & (j == tgt)).tolist()}")
    # the all-fail workgroup, and the others not
    kept = _wg_sums(keep)
    assert not v[I.FAIL_WG * 1024:(I.FAIL_WG + 1) * 1024].any()
    assert kept[I.FAIL_WG] == 0 and kept[0] >= 20 and kept[2] >= 20 and kept[3] >= 2  # (the last has ~40 edges)
    assert keep.sum() >= 100 and (~v).sum() >= 100  # (the dense worlds leave ~5 % valid)
    # the fully failing row has real entries; the empty row's degenerate edges have flags too
    f = c["fail_row"]
    assert (nbr[f] >= 0).all() and not v[f * k:(f + 1) * k].any()
    assert (nbr[c["empty_row"]] == -1).all()
    # -1 entries on both sides: valid (stay -1, not kept) and failed
    assert (v & (j < 0)).any() and (~v & (j < 0)).any()
    # kept edges into the target in the first, third and last workgroup; failed ones too
    into = _wg_sums(keep & (j == tgt))
    assert into[0] >= 1 and into[2] >= 1 and into[3] >= 2 and into[1] == 0
    assert (~v & (j == tgt)).sum() >= 3
    for r in c["sky_rows"][1:]:
        assert (keep[r * k:(r + 1) * k] & (nbr[r] == tgt)).any(), r
    # the last, ragged wave holds a kept edge into the target: lanes past the end count nothing
    assert (keep & (j == tgt))[m - m % 64:].any()
    if name == "gates":
        assert (I.masked_flags(name, layout, 1) != I.masked_flags(name, layout, 0)).sum() >= 10


ROWS = [(name, case, cp) for name in I.WORLDS for case in I.ROWS_CASES for cp in (0, 1)]


def _rows_expected(name, case, cp):
    c = I.rows_case(name, case)
    pre = I.rows_prefill(c)
    v = I.rows_flags(name, c["nprob"], c["cap"], c["k"], cp)
    return c, pre, v, R.rows_ref(c["rows32"], c["ids32"], c["rows_n"], v, c["target"], c["ns_log"], c["nprob"], pre)


@pytest.mark.parametrize("name,case,can_pass", ROWS)
def test_rows_case_has_its_properties(name, case, can_pass):
    c, pre, v, exp = _rows_expected(name, case, can_pass)
    rows32, ids32, k, cap, nprob = c["rows32"], c["ids32"], c["k"], c["cap"], c["nprob"]
    v = v.astype(bool)
    assert cap * k < 4000 and c["ns_log"] == 16
    prob = ids32 >> 16
    assert prob.min() == 0 and prob.max() == nprob - 1 and (ids32 & 0xFFFF).max() < I.NLOC
    if nprob > 1:
        assert (np.diff(ids32) < 0).sum() >= cap // 10  # not ascending
        per_wave = [len(set(np.repeat(prob, k)[w:w + 64].tolist())) for w in range(0, cap * k, 64)]
        assert min(per_wave[:-1]) >= 2  # every wave mixes problems
    inside = (rows32 >> 16 == prob[:, None]) | (rows32 < 0)
    if c["cross"]:
        r, col = c["cross"]
        assert prob[r] == 2 and rows32[r, col] == 1 and v[r * k + col]  # kept, by the oracle
        inside[r, col] = True
    assert inside.all()
    j = rows32.reshape(-1)
    keep = v & (j >= 0)
    # the fully failing row, the empty row
    f = c["fail_row"]
    assert (rows32[f] >= 0).all() and not v[f * k:(f + 1) * k].any()
    assert (rows32[c["empty_row"]] == -1).all()
    if c["fail_block"]:
        r0, r1 = c["fail_block"]
        assert (r0 * k, r1 * k) == (1024, 2048) and not v[1024:2048].any()
        assert len(set(prob[r0:r1].tolist())) == min(nprob, 64)
    live = min(c["rows_n"], cap)
    if live == cap:
        # every problem has a kept edge into its goal, and the counters expect it
        for p in range(nprob):
            g = c["goal_rows"][p]
            assert ids32[g] == (p << 16 | I.LOC_SKY) and rows32[g, 0] == (p << 16 | 1) and keep[g * k]
            if exp["mark"] is not None:
                assert exp["pgoal"][p] > pre["pgoal"][p] and exp["pkept"][p] > pre["pkept"][p]
        assert nprob < 64 or (prob == 63).sum() >= 3
    # the marks: every live row's node, the fully failing row's too
    if exp["mark"] is not None:
        assert (exp["mark"][ids32[:live].astype(np.int64)] == 1).all()
        if f < live:
            assert exp["mark"][ids32[f]] == 1 and pre["mark"][ids32[f]] == 0
        assert (exp["mark"][nprob << 16:] == pre["mark"][nprob << 16:]).all()
        assert (exp["mark"] == 2).sum() > 0  # prefilled bytes elsewhere survive
    if name == "gates" and cap == 389:  # can_pass_gate decides some edges
        other = I.rows_flags(name, nprob, cap, k, 1 - can_pass).astype(bool)
        assert (other != v).sum() >= 10
    assert (exp["pkept"][nprob:] == pre["pkept"][nprob:]).all() and (exp["pgoal"][nprob:] == pre["pgoal"][nprob:]).all()
    print(f"\n{name} {case} can_pass={can_pass}: live rows {live}, kept {int(keep[:live * k].sum())}, "
          f"pgoal {(exp['pgoal'] - pre['pgoal'])[:min(nprob, 4)].tolist()}")


def test_the_cross_edge_counts_by_its_low_bits():
    """The edge from a row of problem 2 into global id 1: pgoal[2] counts it ((j & 0xFFFF) == 1),
    pgoal[0] does not (the row's problem decides), count[1] counts it (j == target == 1) and
    counts none of the edges into the goals of problems 1 and 2."""
    name = "n180"
    c, pre, v, exp = _rows_expected(name, "p3", 0)
    r, col = c["cross"]
    k = c["k"]
    j = c["rows32"].reshape(-1).astype(np.int64)
    keep = v.astype(bool) & (j >= 0)
    prob = np.repeat(c["ids32"] >> 16, k)
    by_low_bits = [int((keep & (prob == p) & ((j & 0xFFFF) == 1)).sum()) for p in range(3)]
    by_global_id = [int((keep & (prob == p) & (j == (p << 16 | 1))).sum()) for p in range(3)]
    assert (exp["pgoal"] - pre["pgoal"])[:3].tolist() == by_low_bits
    assert by_low_bits[2] == by_global_id[2] + 1 and by_low_bits[:2] == by_global_id[:2]
    assert exp["count"][1] - pre["count"][1] == int((keep & (j == 1)).sum()) == by_global_id[0] + 1
    without = c["rows32"].copy()
    without[r, col] = -1
    e2 = R.rows_ref(without, c["ids32"], c["rows_n"], v, 1, 16, 3, pre)
    assert (exp["pgoal"] - e2["pgoal"])[:3].tolist() == [0, 0, 1]
    assert (exp["pkept"] - e2["pkept"])[:3].tolist() == [0, 0, 1]


def _copy(d):
    return {k: (None if a is None else np.array(a)) for k, a in d.items()}


def test_compare_rejects_the_mistakes_it_is_for():
    name, layout = "n40", "k8"
    c = I.masked_case(name, layout)
    v = I.masked_flags(name, layout, 0)
    pre = I.masked_prefill(c, (7, 1 << 40))
    exp = R.masked_ref(c["nbr"], v, c["target"], pre)
    assert R.compare(_copy(exp), exp) == []
    j = c["nbr"].reshape(-1)
    keep = v.astype(bool) & (j >= 0)

    def rejected(got, exp, *names):
        bad = R.compare(got, exp)
        assert sorted(b.split(":")[0] for b in bad) == sorted(names), bad

    got = _copy(exp)  # one workgroup's share missing from count[0]
    got["count"][0] -= keep[2048:3072].sum()
    rejected(got, exp, "count")
    got = _copy(exp)  # counts that overwrite instead of add
    got["count"] -= pre["count"]
    rejected(got, exp, "count")
    got = _copy(exp)  # one failed entry left unmasked
    e = int(np.flatnonzero((v == 0) & (j >= 0))[17])
    got["nbr"].reshape(-1)[e] = j[e]
    rejected(got, exp, "nbr")
    got = _copy(exp)  # out16 the table's low bits whatever the flag: no 0xFFFF for a failed edge
    got["out16"] = (j & 0xFFFF).astype(np.uint16)
    rejected(got, exp, "out16")

    # the rows entry
    rc, rpre, rv, rexp = _rows_expected(name, "p3", 0)
    assert R.compare(_copy(rexp), rexp) == []
    k = rc["k"]
    got = _copy(rexp)  # the mark of the fully failing row missing
    got["mark"][rc["ids32"][rc["fail_row"]]] = 0
    rejected(got, rexp, "mark")
    got = _copy(rexp)  # out16 carrying the entry where it fits 16 bits, not its low 16 bits
    rj = rc["rows32"].reshape(-1)
    rkeep = rv.astype(bool) & (rj >= 0)
    got["out16"] = np.where(rkeep & (rj < 0x10000), rj, 0xFFFF).astype(np.uint16)
    rejected(got, rexp, "out16")
    got = _copy(rexp)  # pgoal counted by global id
    prob = np.repeat(rc["ids32"] >> 16, k)
    got["pgoal"] = rpre["pgoal"] + np.bincount(prob[rkeep & (rj == 1)], minlength=I.COUNTERS).astype(np.uint64)
    rejected(got, rexp, "pgoal")
    got = _copy(rexp)  # pkept[nprob] touched
    got["pkept"][rc["nprob"]] += 1
    rejected(got, rexp, "pkept")
    got = _copy(rexp)  # per-problem counts that overwrite
    got["pkept"][:3] -= rpre["pkept"][:3]
    rejected(got, rexp, "pkept")
    # a write into a row >= rows_n: its flag, its entry, its u16 entry
    rc, rpre, rv, rexp = _rows_expected(name, "p3_rows_cap_m1", 0)
    last = (rc["cap"] - 1) * k
    assert rexp["valid"][last] == 0xA5 and rexp["out16"][last] == 0xBEEF
    full = R.rows_ref(rc["rows32"], rc["ids32"], rc["cap"], rv, 1, 16, 3, rpre)
    for what in ("valid", "rows32", "out16", "mark"):
        got = _copy(rexp)
        got[what] = np.array(full[what])
        if what == "rows32" and (full["rows32"] == rexp["rows32"]).all():
            continue  # (the last row lost no entry)
        rejected(got, rexp, what)
    # an output that is NULL must come back as None, and the other way round
    rc, rpre, rv, rexp = _rows_expected(name, "p3_no_count", 0)
    assert rexp["count"] is None and rexp["out16"] is not None and rexp["mark"] is not None
    got = _copy(rexp)
    got["count"] = np.zeros(2, np.int64)
    rejected(got, rexp, "count")
