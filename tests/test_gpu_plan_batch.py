"""The batched planner's device stages (csrc/plan_batch.hip) and the reverse-edge CSR
(csrc/planner.hip) against plain references, below the level of a finished path.

epp_dbg_plan_batch runs one batch through plan_batch_layout / plan_batch_launch as the
product does, without solver or fallback, and hands back the emitted block; the reference
(tests/plan_batch_ref.py) restates the stages in numpy plus the oracle.  Every comparison is
an equality: the nodes, every header word, every listed row keyed by its node, the
referenced coordinates, the completion slots.  tests/plan_batch_inputs.py builds the cases
(tests/test_plan_batch_inputs_cpu.py shows which branch of pb_query_row each reaches).
"""
import numpy as np
import pytest

from eppamd import capi

import plan_batch_inputs as I
import plan_batch_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    w = I.device_world()
    yield w
    w.close()


def _run(world, name, seqs=(7,), fill=0):
    b = I.case(name)
    return capi.dbg_plan_batch(world, b["can_pass"], b["lo"], b["hi"], b["ns"], b["k"], b["segs"], seqs=seqs, fill=fill)


@pytest.mark.parametrize("name", I.case_names())
def test_emitted_block_equals_reference(world, name):
    em = _run(world, name, seqs=(0x1234567,))
    R.compare(em, I.reference(name), I.case(name)["k"])


# one case per shape of the batch: uploaded problems, ties, capped rows, dropped rows
REPEAT = ["product_k8_p0", "scaled_k16", "degenerate_100", "capacity", "batch_17"]


@pytest.mark.parametrize("name", REPEAT)
def test_second_run_on_one_workspace(world, name):
    """The same batch twice on one workspace, another seq: the second run's block (the pinned
    block's emitted part overwritten with 0xFF bytes in between) is the first's."""
    k = I.case(name)["k"]
    once = _run(world, name, seqs=(3,))
    twice = _run(world, name, seqs=(3, 0xFFFFFFF0), fill=2)
    assert twice["seq"] == 0xFFFFFFF0
    R.compare(once, I.reference(name), k)
    R.compare(twice, I.reference(name), k)
    R.emitted_equal(once, twice, I.reference(name), k)


@pytest.mark.parametrize("name", REPEAT)
def test_workspace_prefilled_with_ff(world, name):
    """The device workspace and the pinned block hold 0xFF bytes before the run: the stages
    clear what they read."""
    k = I.case(name)["k"]
    em = _run(world, name, seqs=(11,), fill=1)
    R.compare(em, I.reference(name), k)
    R.emitted_equal(_run(world, name, seqs=(11,)), em, I.reference(name), k)


def test_unsupported_world():
    """A world without OBBs has no tile tables: restricted rows are refused, cap == 0 runs."""
    w = capi.World(np.zeros(0, capi.OBB_DTYPE), 0.1, 0.1)
    try:
        b = I.case("batch_1")
        with pytest.raises(capi.EppError) as e:
            capi.dbg_plan_batch(w, False, b["lo"], b["hi"], b["ns"], b["k"], b["segs"])
        assert e.value.code == capi.EPP_ERR_UNSUPPORTED
        segs = [dict(q, cap=0) for q in b["segs"]]
        em = capi.dbg_plan_batch(w, False, b["lo"], b["hi"], b["ns"], b["k"], segs, seqs=(5,))
        assert int(em["hdr"][3 + 3]) == b["ns"] + 2 and int(em["hdr"][1]) == 0  # every sample valid, no rows
        assert np.all(em["done"] == 5)
    finally:
        w.close()


# ---------------------------------------------------------------------------- reverse CSR
# 16384 = the single scan workgroup's chunk (1024 threads x 16 counts)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 16383, 16384, 16385, 40000, 70000])
def test_reverse_csr(n):
    tab = I.reverse_table(n)
    roff, radj, radj16 = capi.dbg_reverse_csr(tab)
    deg = np.bincount(tab[tab >= 0], minlength=n)
    want_off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    assert np.array_equal(roff, want_off)  # the exclusive prefix of the in-degrees
    # every node's run: its sources ascending = the edges sorted by (target, source)
    src = np.repeat(np.arange(n, dtype=np.int32), tab.shape[1])
    dst = tab.reshape(-1)
    have = dst >= 0
    order = np.lexsort((src[have], dst[have]))
    assert np.array_equal(radj, src[have][order])
    if n <= 65535:
        assert radj16 is not None and np.array_equal(radj16.astype(np.int32), radj)
    else:
        assert radj16 is None
    if n >= 16383:
        assert deg[0] == 0 and deg[n - 1] > 2000  # an empty run and the hub's
