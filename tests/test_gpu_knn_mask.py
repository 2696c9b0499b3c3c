"""What k_motions_v5<W, 0, true> (csrc/motions_tile.hip) writes besides the validity flags when
it is given a MotionMask -- the masked table, its u16 copy, the kept / into-target counts, and
for the batched planner the marks and the per-problem counts over packed rows -- compared whole
and exactly with knn_mask_ref's restatement of the tail on the oracle's flags.  This file is the
statement of that contract: everything the planner's searches read comes out of this tail.

The two entries run through epp_dbg_knn_motions_masked / epp_dbg_knn_motions_rows
(csrc/host_dbg_planner.cpp), which allocate and clear nothing: every output is prefilled by the
test and downloaded whole, so a write outside the live rows, a counter that is overwritten
rather than added to, or a touched slot past nprob shows as a difference.

Worlds (knn_mask_inputs.WORLDS): c1 (W 1, S 64), n40 (W 2), n180 (W 4, S 32), n700 (W 2, S 16),
n520 (W 16, S 32), n600 (W 32), the gate cluster (W 4, fillings; can_pass_gate 0 and 1 on all).
The masked entry: 3109 = 3 * 1024 + 37 entries (k = 1) and 3112 (k = 8), counters prefilled
(0, 0) and (7, 2^40).  The rows entry: knn_mask_inputs.ROWS_CASES -- nprob 1, 3 and 64, rows_n
0, 1, cap - 1, cap and cap + 5, cap k = 1020, 1024 and 1040 (k = 4, 8, 16), and count, out16 or
mark left out.  test_knn_mask_inputs_cpu.py shows on the CPU that the cases hold what they are
named for and that the comparison rejects the mistakes this file is for.

Every assertion is an equality.
"""
import numpy as np
import pytest

from eppamd import capi

import knn_mask_inputs as I
import knn_mask_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_kernels(monkeypatch):
    monkeypatch.delenv("EPP_MOTIONS_KERNEL", raising=False)
    monkeypatch.delenv("EPP_MOTIONS_BLOCK", raising=False)


@pytest.fixture(scope="module")
def worlds():
    """name -> capi.World, created on first use, closed with the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = I.device_world(name)
        return made[name]

    yield get
    for w in made.values():
        w.close()


@pytest.fixture(scope="module")
def problem_nodes():
    """name -> the device array of 64 x 65536 nodes (100 MB, allocated and zeroed once) holding
    that world's problem_nodes; only the nodes that have a position are uploaded."""
    state = {"buf": None, "name": None}

    def get(name):
        if state["buf"] is None:
            state["buf"] = capi.DeviceBuffer(24 * (I.MAX_PROB << I.NS_LOG))
            state["buf"].zero()
        if state["name"] != name:
            I.upload_problem_nodes(name, state["buf"])
            state["name"] = name
        return state["buf"]

    yield get
    if state["buf"] is not None:
        state["buf"].free()


def _masked(name, layout, can_pass, counters):
    c = I.masked_case(name, layout)
    pre = I.masked_prefill(c, counters)
    return c, pre, R.masked_ref(c["nbr"], I.masked_flags(name, layout, can_pass), c["target"], pre)


def _run_masked(w, c, pre, can_pass, **kw):
    return capi.dbg_knn_motions_masked(w, c["nodes"], kw.pop("nbr", c["nbr"]), can_pass, c["target"], pre["valid"],
                                       pre["out16"], pre["count"], **kw)


def _rows(name, case, can_pass):
    c = I.rows_case(name, case)
    pre = I.rows_prefill(c)
    v = I.rows_flags(name, c["nprob"], c["cap"], c["k"], can_pass)
    return c, pre, R.rows_ref(c["rows32"], c["ids32"], c["rows_n"], v, c["target"], c["ns_log"], c["nprob"], pre)


def _run_rows(w, nodes, c, pre, can_pass, **kw):
    nprob = kw.pop("nprob", c["nprob"])
    return capi.dbg_knn_motions_rows(w, nodes, c["rows32"], c["ids32"], c["rows_n"], can_pass, c["target"], pre["valid"],
                                     pre["out16"], pre["count"], pre["mark"], pre["pkept"], pre["pgoal"], c["ns_log"],
                                     nprob, **kw)


def _untouched_masked(c, pre):
    return dict(nbr=c["nbr"], valid=pre["valid"], out16=pre["out16"], count=pre["count"])


def _untouched_rows(c, pre):
    return dict(pre, rows32=c["rows32"], ids32=c["ids32"], rows_n=np.array([c["rows_n"]], np.int64))


# ---- a. the masked entry ----------------------------------------------------------------------
@pytest.mark.parametrize("name,layout,can_pass",
                         [(name, layout, cp) for name in I.WORLDS for layout in I.LAYOUTS for cp in (0, 1)])
def test_masked_entry(name, layout, can_pass, worlds):
    """Flags, masked table, out16 and both counts; the counters prefilled 0 and (7, 2^40)."""
    for counters in I.COUNTER_PREFILLS:
        c, pre, exp = _masked(name, layout, can_pass, counters)
        got = _run_masked(worlds(name), c, pre, can_pass)
        assert got.pop("rc") == capi.EPP_OK
        assert R.compare(got, exp) == [], (name, layout, can_pass, counters)


# ---- b. the rows entry ------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,can_pass",
                         [(name, case, cp) for name in I.WORLDS for case in I.ROWS_CASES for cp in (0, 1)])
def test_rows_entry(name, case, can_pass, worlds, problem_nodes):
    """Every output whole: the live rows' flags, entries, u16 entries, marks and counts, and
    everything else as it was prefilled."""
    w = worlds(name)
    assert capi.dbg_knn_motions_rows_supported(w)
    c, pre, exp = _rows(name, case, can_pass)
    got = _run_rows(w, problem_nodes(name), c, pre, can_pass)
    assert got.pop("rc") == capi.EPP_OK
    assert R.compare(got, exp) == [], (name, case, can_pass)


# ---- c. refusals ------------------------------------------------------------------------------
def test_masked_entry_refuses_what_the_small_path_would_take(worlds, monkeypatch):
    """m <= 1024 on c1 (<= 256 OBBs), and any batch with EPP_MOTIONS_KERNEL set:
    EPP_ERR_UNSUPPORTED, nothing written; then the valid call on the same buffers."""
    w = worlds(I.C1)
    c, pre, exp = _masked(I.C1, "k8", 0, (7, 1 << 40))
    full = dict(pre, nodes=c["nodes"], nbr=c["nbr"])
    dev = {name: capi.DeviceBuffer.from_array(a) for name, a in full.items()}

    def whole():
        return {name: dev[name].download(a.dtype, a.size).reshape(a.shape) for name, a in full.items()}

    # the first 128 rows of the table, 1024 entries, in the whole table's buffers
    small = _run_masked(w, c, pre, 0, nbr=c["nbr"][:128], dev=dev, upload=False)
    assert small.pop("rc") == capi.EPP_ERR_UNSUPPORTED
    assert R.compare(whole(), full) == []
    monkeypatch.setenv("EPP_MOTIONS_KERNEL", "v4")
    got = _run_masked(w, c, pre, 0, dev=dev, upload=False)
    assert got.pop("rc") == capi.EPP_ERR_UNSUPPORTED
    assert R.compare(got, _untouched_masked(c, pre)) == []
    monkeypatch.delenv("EPP_MOTIONS_KERNEL")
    got = _run_masked(w, c, pre, 0, dev=dev, upload=False)
    assert got.pop("rc") == capi.EPP_OK
    assert R.compare(got, exp) == []


def test_rows_entry_runs_where_the_masked_entry_refuses(worlds, problem_nodes, monkeypatch):
    """The planner's own rows: neither the small path (1024 entries on c1) nor
    EPP_MOTIONS_KERNEL applies."""
    w = worlds(I.C1)
    for case, env in (("k8_at_1024", None), ("k4_below_1024", None), ("k8_at_1024", "small"), ("p3", "generic")):
        if env:
            monkeypatch.setenv("EPP_MOTIONS_KERNEL", env)
        c, pre, exp = _rows(I.C1, case, 0)
        got = _run_rows(w, problem_nodes(I.C1), c, pre, 0)
        assert got.pop("rc") == capi.EPP_OK
        assert R.compare(got, exp) == [], (case, env)


def test_both_entries_refuse_a_world_without_obbs(worlds, problem_nodes):
    empty = I.empty_world()
    assert not capi.dbg_knn_motions_rows_supported(empty)
    c, pre, exp = _masked("n40", "k8", 0, (7, 1 << 40))
    dev = {}
    got = _run_masked(empty, c, pre, 0, dev=dev)
    assert got.pop("rc") == capi.EPP_ERR_UNSUPPORTED
    assert R.compare(got, _untouched_masked(c, pre)) == []
    got = _run_masked(worlds("n40"), c, pre, 0, dev=dev, upload=False)
    assert got.pop("rc") == capi.EPP_OK
    assert R.compare(got, exp) == []
    c, pre, exp = _rows("n40", "p3", 0)
    dev = {}
    got = _run_rows(empty, problem_nodes("n40"), c, pre, 0, dev=dev)
    assert got.pop("rc") == capi.EPP_ERR_UNSUPPORTED
    assert R.compare(got, _untouched_rows(c, pre)) == []
    got = _run_rows(worlds("n40"), problem_nodes("n40"), c, pre, 0, dev=dev, upload=False)
    assert got.pop("rc") == capi.EPP_OK
    assert R.compare(got, exp) == []
    empty.close()


def test_invalid_arguments_write_nothing(worlds, problem_nodes):
    """The rows entry: nprob 0 or 65 with marks, mark without out16.  The masked entry, which
    has no such arguments: no count.  EPP_ERR_INVALID_ARGUMENT, every output as prefilled; the
    next valid call on the same buffers gives the restatement's result."""
    w, nodes = worlds("n180"), problem_nodes("n180")
    c, pre, exp = _rows("n180", "p3", 1)
    dev = {}
    for nprob in (0, 65):
        got = _run_rows(w, nodes, c, pre, 1, nprob=nprob, dev=dev)
        assert got.pop("rc") == capi.EPP_ERR_INVALID_ARGUMENT, nprob
        assert R.compare(got, _untouched_rows(c, pre)) == [], nprob
    got = _run_rows(w, nodes, c, dict(pre, out16=None), 1, dev=dev)
    assert got.pop("rc") == capi.EPP_ERR_INVALID_ARGUMENT
    assert R.compare(got, _untouched_rows(c, dict(pre, out16=None))) == []
    assert R.compare(dict(out16=dev["out16"].download(np.uint16, pre["out16"].size)), dict(out16=pre["out16"])) == []
    got = _run_rows(w, nodes, c, pre, 1, dev=dev, upload=False)
    assert got.pop("rc") == capi.EPP_OK
    assert R.compare(got, exp) == []
    c, pre, exp = _masked("n180", "k8", 1, (7, 1 << 40))
    dev = {}
    got = _run_masked(w, c, pre, 1, dev=dev)  # (creates the buffers, count among them)
    assert got.pop("rc") == capi.EPP_OK and R.compare(got, exp) == []
    got = _run_masked(w, c, dict(pre, count=None), 1, dev=dev)
    assert got.pop("rc") == capi.EPP_ERR_INVALID_ARGUMENT
    assert R.compare(got, _untouched_masked(c, dict(pre, count=None))) == []
    dev["count"].upload(pre["count"])
    got = _run_masked(w, c, pre, 1, dev=dev, upload=False)
    assert got.pop("rc") == capi.EPP_OK
    assert R.compare(got, exp) == []


# ---- d. the separate kernel -------------------------------------------------------------------
@pytest.mark.parametrize("can_pass", (0, 1))
def test_fused_tail_agrees_with_mask_edges_count(can_pass, worlds):
    """k_mask_edges_count (planner.hip) on the same table and the fused launch's own flags: the
    same masked table and the same two counts."""
    name, layout = "gates", "k8"
    c, pre, _ = _masked(name, layout, can_pass, (0, 0))
    got = _run_masked(worlds(name), c, pre, can_pass)
    assert got.pop("rc") == capi.EPP_OK
    table, kept, into = capi.mask_edges_count(c["nbr"], got["valid"].reshape(c["nbr"].shape), c["target"])
    assert R.compare(dict(nbr=table), dict(nbr=got["nbr"])) == []
    assert [kept, into] == got["count"].tolist() and kept > 0 and into > 0
