"""The planner batch's stage-test inputs do what they claim (no GPU: the reference alone).

tests/plan_batch_inputs.py builds the cases, tests/plan_batch_ref.py restates the device
stages; here every branch and exit of pb_query_row must be taken by some query, both
outcomes of the state and motion checks must occur, and no input may sit so close to a
threshold that the device's last bit could decide (conditions on the inputs, not tolerances).
Run with -s for the counts.
"""
import collections

import numpy as np
import pytest

import plan_batch_inputs as I
import plan_batch_ref as R


@pytest.fixture(scope="module")
def refs():
    return {name: I.reference(name) for name in I.case_names()}


def _outcomes(ref_list):
    c = collections.Counter()
    for ref in ref_list:
        for i, o in ref["outcome"].items():
            c[o] += 1
            if o in R.BRANCHES:
                c[f"radius_{ref['info'][i][0]}"] += 1
    return c


def test_every_branch_and_exit_is_taken(refs):
    total = collections.Counter()
    for name, rl in refs.items():
        c = _outcomes(rl)
        total.update(c)
        print(f"{name}: nodes {[r['n'] for r in rl]} queries {[len(r['queries']) for r in rl]} {dict(c)}")
    print("all cases:", dict(total))
    for what in R.BRANCHES + ("gate", "overflow", "radius_2", "radius_3"):
        assert total[what] > 0, f"no query takes {what}"


def test_cases_reach_what_they_are_for(refs):
    for k in (4, 8, 16):
        for cp in (0, 1):
            c = _outcomes(refs[f"product_k{k}_p{cp}"])
            assert c["lane"] > 0 and c["lane"] >= 0.9 * sum(c[b] for b in R.BRANCHES)
    for name in ("scaled_k4", "scaled_k16"):
        up8, up20, up45, down, tight = refs[name]
        assert _outcomes([up8])["bisect_lane"] > 0 and _outcomes([up20])["rank_all"] > 0
        # the overflow exit: every query of the problem gives up, the rows come back all-none
        assert set(up45["outcome"].values()) == {"overflow"}
        assert all(np.all(row == -1) for row in up45["rows"].values())
        c = _outcomes([down])  # (k = 4 is mostly served by the first radius even here)
        assert name != "scaled_k16" or (c["radius_2"] > 0 and c["radius_3"] > 0)
        c = _outcomes([tight])  # exact and dropped rows in one problem
        assert c["gate"] > 0 and sum(c[b] for b in R.BRANCHES) > 0
    want = {40: "lane", 100: "bisect_lds", 300: "rank_all", 600: "overflow"}
    for n, o in want.items():
        for ref in refs[f"degenerate_{n}"]:
            assert ref["n"] == n + 2 and set(ref["outcome"].values()) == {o}, (n, _outcomes([ref]))
    coarse, flat = refs["grid"]
    assert coarse["h_eff"] > I.case("grid")["segs"][0]["h"] and flat["dims"][2] == 1
    cap = refs["capacity"]
    segs = I.case("capacity")["segs"]
    assert len(cap[0]["queries"]) > segs[0]["cap"] > 0 and len(cap[1]["queries"]) == segs[1]["cap"]
    assert segs[2]["cap"] == 0 and segs[3]["cap"] > len(cap[3]["queries"])
    assert len({x.tobytes() for x in cap[0]["nodes"]}) == cap[0]["n"]  # distinct coordinates
    for S in (1, 16, 17, 64):
        b = I.case(f"batch_{S}")
        assert len(b["segs"]) == S and len({q["seed"] for q in b["segs"]}) == S
    c = I.compact_chunk()
    for n in (c, c + 1, 4 * c, 4 * c + 1):
        assert I.case(f"samples_{n}")["ns"] == n
        assert refs[f"nodes_{n}"][0]["n"] == n
        need = R.expected_words(refs[f"nodes_{n}"][0], 8)["need"]
        assert n < 4 * c or len(np.unique(need // c)) >= 4  # the numbering crosses k_pb_number's chunks


def test_both_outcomes_of_the_checks_occur(refs):
    for name, rl in refs.items():
        valid = np.concatenate([r["valid"] for r in rl])
        if not name.startswith("degenerate"):
            assert valid.any() and not valid.all(), f"{name}: one state outcome only"
        kept = sum(r["motions"][0] for r in rl if "motions" in r)
        dropped = sum(r["motions"][1] for r in rl if "motions" in r)
        print(f"{name}: samples valid {int(valid.sum())} / {len(valid)}, row entries kept {kept}, dropped {dropped}")
        if not name.startswith("degenerate"):
            assert kept > 0 and dropped > 0, f"{name}: one motion outcome only"


def test_no_input_near_a_threshold(refs):
    for name, rl in refs.items():
        for p, ref in enumerate(rl):
            if ref["cap"] == 0:
                continue
            assert ref["thr_margin"] > 1e-9, f"{name} problem {p}: a node within 1e-9 of the query threshold"
            for i, info in ref["info"].items():
                assert info[2] > 1e-12, f"{name} problem {p} node {i}: a candidate within 1e-12 of a deciding threshold"
                assert info[3] > 1e-9, f"{name} problem {p} node {i}: the ellipsoid gate within 1e-9 of gbound"


def test_exact_cases_are_exact(refs):
    exact = [f"product_k{k}_p{cp}" for k in (4, 8, 16) for cp in (0, 1)] + ["grid", "capacity", "degenerate_40",
                                                                            "degenerate_100", "degenerate_300"]
    exact += [n for n in I.case_names() if n.startswith(("samples", "nodes"))]
    for name in exact:
        for p, ref in enumerate(refs[name]):
            bad = [o for o in ref["outcome"].values() if o in R.EXITS]
            assert not bad, f"{name} problem {p}: {len(bad)} dropped rows ({set(bad)})"


def test_reverse_tables():
    for n in (1, 2, 255, 257, 16385, 40000):
        tab = I.reverse_table(n)
        assert tab.shape == (n, 16) and tab.min() >= -1 and tab.max() < n
        srt = np.sort(tab, axis=1)
        assert not np.any((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)), "an entry twice in a row"
        deg = np.bincount(tab[tab >= 0], minlength=n)
        assert deg[0] == 0
        if n >= 16385:
            assert 2000 < deg[n - 1] < 3100
