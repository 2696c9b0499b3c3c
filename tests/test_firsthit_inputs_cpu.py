"""CPU: the inputs of test_gpu_firsthit.py (firsthit_inputs.py) checked with the restatement
alone (firsthit_ref.py): every class of edge the crafted sets claim to hold is present in each
world where it can exist, both outcomes occur per can_pass_gate, and the scalar and the numpy
form of the restatement give the same answers on every crafted set."""
import numpy as np
import pytest

import firsthit_inputs as fi
import firsthit_ref as fr
import small_path_inputs as spi


def _answers(name, can_pass):
    _, rg, ro = spi.setup()
    s1, s2 = fi.edges(name, fi.BLOCK + 1)
    m = fr.matrices(fi.ref_world(name), rg, ro, s1, s2, can_pass)
    t, obb = fr.reduce_min(m["t"])
    et, eo = fi.expected(name, fi.BLOCK + 1, can_pass)
    assert np.array_equal(t, et) and np.array_equal(obb, eo)  # (the prefiltered form == the full matrix)
    return s1, s2, m, t, obb


def test_tile_constant_and_worlds():
    assert fi.T >= 64 and len(fi.obbs("T")) == fi.T and len(fi.obbs("T+1")) == fi.T + 1
    assert len(fi.obbs("300")) > fi.T and len(fi.obbs("1100")) > 4 * fi.T  # several tiles
    assert fi.obbs("filling")["filling"].all()
    for name in fi.HAS_GATES:
        ob = fi.obbs(name)
        assert ob["filling"].any() and not ob["filling"].all()
        assert not ob[fi.T - 1:fi.T + 1]["filling"].any()  # (the records at the tile edge, where there are any)


@pytest.mark.parametrize("name", fi.WORLDS)
def test_scalar_and_numpy_forms_agree(name):
    _, rg, ro = spi.setup()
    w = fi.ref_world(name)
    s1, s2 = fi.edges(name, fi.BLOCK + 1)
    for cp in fi.CAN_PASS:
        t, obb = fi.expected(name, fi.BLOCK + 1, cp)
        for k in range(len(s1)):
            assert fr.first_hit(w, rg, ro, list(s1[k]), list(s2[k]), cp) == (t[k], obb[k]), (name, cp, k)


@pytest.mark.parametrize("name", fi.WORLDS)
def test_edge_sets_hold_what_they_claim(name):
    ob = fi.obbs(name)
    fill = ob["filling"].astype(bool)
    res = {cp: _answers(name, cp) for cp in fi.CAN_PASS}
    rows = np.arange(fi.BLOCK + 1)
    for cp in fi.CAN_PASS:
        s1, s2, m, t, obb = res[cp]
        blocked = obb >= 0
        zero_len = (s1 == s2).all(axis=1)
        nothing = name == "filling" and cp  # every OBB is skipped: no edge is blocked
        print(f"{name} can_pass {cp}: blocked {int(blocked.sum())}/{len(obb)}, t == 0 {int((t == 0).sum())}, "
              f"0 < t < 1 {int(((t > 0) & (t < 1)).sum())}, t == 1 {int((t == 1).sum())}")
        assert ((t >= 0) & (t <= 1))[blocked].all() and np.isinf(t[~blocked]).all()
        # misses that pass the prefilter, and misses that fail it
        assert (~blocked & m["part"].any(axis=1)).any() or nothing
        assert (~blocked & ~m["part"].any(axis=1)).sum() >= 4
        assert (~blocked & zero_len).any()  # a zero-length edge outside every box
        if nothing:
            assert not blocked.any()
            continue
        assert blocked.sum() >= 4 and (~blocked).sum() >= 16  # both outcomes (a 1-OBB world has few targets)
        win = np.maximum(obb, 0)
        # starts inside a box (an edge with length), zero-length edges inside one
        assert (blocked & (t == 0) & m["start"][rows, win] & ~zero_len).any()
        assert (blocked & zero_len).any()
        # hits with 0 < t < 1
        assert (blocked & (t > 0) & (t < 1) & m["slab"][rows, win]).sum() >= 2
        # end-only hits: the winner neither contains the start nor passes the slab test
        if not fill.all():
            end_only = blocked & (t == 1.0) & ~m["start"][rows, win] & ~m["slab"][rows, win] & m["end"][rows, win]
            assert end_only.any()
        # the last record of the first tile, the first record of the next
        if len(ob) >= fi.T:
            assert (obb == fi.T - 1).any()
        if len(ob) > fi.T:
            assert (obb == fi.T).any()
        # ties on t between two indices: the lower one is the answer
        if name in fi.HAS_GATES:
            ties = blocked & ((m["t"] == t[:, None]).sum(axis=1) >= 2)
            assert ties.any()
    # edges through the filling boxes: blocked by one with can_pass 0; with 1 they pass, or hit a bar
    if fill.any():
        _, _, m0, t0, obb0 = res[False]
        _, _, _, t1, obb1 = res[True]
        hits_filling = np.isfinite(m0["t"][:, fill]).any(axis=1)
        wins_filling = (obb0 >= 0) & fill[np.maximum(obb0, 0)]
        assert (wins_filling & (obb1 == -1)).any()
        if not fill.all():
            assert (hits_filling & (obb1 >= 0) & ~fill[np.maximum(obb1, 0)]).any()
        assert not fill[obb1[obb1 >= 0]].any()
