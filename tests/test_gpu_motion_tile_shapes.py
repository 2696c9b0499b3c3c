"""GPU parity of k_motions_v5 (csrc/motions_tile.hip), the default edge-validity kernel and
the only one behind the k-NN-table entries, against the CPU oracle, bit for bit, at every row
width W it is compiled for.

build_blob (csrc/world_index.cpp) picks the smallest W (words of OBB bits per tile row), then
the fewest tiles T per axis, for which no tile holds more than 32 W OBBs, then S local slabs
per tile by the LDS budget; launch_motions_tile picks the instantiation from W.

The shapes the suite reached before this file.  Measured on the CPU, from the index build
(epp_dbg_build_blob) of every world the suite sends through this kernel, and not on a GPU:

    world (tests)          OBBs            T   W   S    fits 150 KB LDS
    c1                     9 / 10 filling  1   1   64   yes
    c2                     64 / 72         2   1   64   yes
    c3                     512 / 520       6   1   64   yes
    3000-obstacle world    3040            5   8   4    no (467 KB): the cell-list kernel runs

So every GPU test of k_motions_v5 ran W = 1, S = 64, T in {1, 2, 6}: 20 of its 24
instantiations (6 W x analytic / discrete32 x endpoint arrays / k-NN table) had never executed
under a test, nor had any S < 64.

The shapes this file adds (tile_shape_inputs.py; test_tile_shape_inputs_cpu.py asserts them on
the CPU, from the same index build, and that every world fits the LDS; here the k-NN-table
entry, which has no other kernel to fall back to, is the witness that the tile kernel ran):

    world    OBBs                 T   W    S    LDS bytes
    n40      40                   1   2    64    27,616
    n180     180                  3   4    32    79,184
    n500     500                  2   8    64   143,136
    n350     350                  1   16   64    92,336
    n600     600                  1   32   64   152,128
    n700     700                  5   2    16   145,408
    n520     520                  2   16   32   145,216
    gates    144 (24 fillings)    2   4    64    68,928

In n500, n520 and gates the tile boundaries run through the cluster, so the FX / FY rows hold
zeros and ones past their first word; in n180 the cluster lies inside one tile.  Both tables
come from the index build on the CPU; what a GPU run adds is that the kernel gives the
oracle's answers on these shapes.

A cluster stacks dozens of boxes on one spot, where "invalid" survives the loss of almost any
one candidate.  The edges that notice a dropped candidate are the ones across the corners
where one box sticks out of the rest (tile_shape_inputs.corner_pairs), a fifth of the set.

What only matters for W > 1: bit j & 31 of word j >> 5 in the LE / GE prefix rows, the FX / FY
"first tile along the axis" rows, the FILL row (the gate cluster has openings at tile slots
past 32), the u16 id table behind them, the per-lane popcount, scan and bit-pick over W words,
and slab_row_stride(W).  A wrong word index there drops a candidate OBB, and the answer is
"valid" for an edge that collides.

Worlds, edges, tables and expectations: tile_shape_inputs.py.
"""
import numpy as np
import pytest

from eppamd import capi

import tile_shape_inputs as I

pytestmark = pytest.mark.gpu

CASES = [(name, mode, cp) for name in I.WORLDS for mode in (0, 1) for cp in (0, 1)]
_case = pytest.mark.parametrize("name,mode,can_pass", CASES)


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    bad = np.flatnonzero(got != exp)
    assert got.shape == exp.shape and len(bad) == 0, (
        what, f"{len(bad)} of {len(exp)} differ; first at {bad[:10].tolist()}: got {got[bad[:10]].tolist()}, "
              f"expected {exp[bad[:10]].tolist()}")


def _world(name):
    _, rg, ro = I.setup(name)
    return capi.World(I.world(name)[0], rg, ro)


def _default_kernels(monkeypatch):
    monkeypatch.delenv("EPP_MOTIONS_KERNEL", raising=False)
    monkeypatch.delenv("EPP_MOTIONS_BLOCK", raising=False)
    monkeypatch.delenv("EPP_STATES_KERNEL", raising=False)


@_case
def test_motions_against_the_oracle(name, mode, can_pass, monkeypatch):
    """World.check_motions through the default kernel choice: k_motions_v5<W, mode, false>."""
    _default_kernels(monkeypatch)
    w = _world(name)
    s1, s2 = I.motion_edges(name)
    _same(w.check_motions(s1, s2, can_pass, mode), I.exp_motions(name, mode, can_pass), (name, mode, can_pass))
    w.close()


@_case
def test_knn_table_motions(name, mode, can_pass, monkeypatch):
    """epp_check_knn_motions, k_motions_v5<W, mode, true>: EPP_OK (it returns
    EPP_ERR_UNSUPPORTED exactly when launch_motions_tile declines the world, so this is the
    witness that the tile kernel runs on it), the oracle's flags on the edges the table
    denotes, which are epp_knn_edges' output, and epp_check_motions' flags on those."""
    _default_kernels(monkeypatch)
    w = _world(name)
    nodes, nbr = I.knn_table(name)
    n, k = nbr.shape
    d_n, d_k, d_v = capi.DeviceBuffer.from_array(nodes), capi.DeviceBuffer.from_array(nbr), capi.DeviceBuffer(n * k)
    d_v.zero()
    rc = capi.lib().epp_check_knn_motions(w.handle, d_n.ptr, d_k.ptr, n, k, can_pass, mode, d_v.ptr, None)
    assert rc == capi.EPP_OK, (name, rc)
    capi.sync()
    got = d_v.download(np.uint8, n * k)
    exp = I.exp_knn_motions(name, mode, can_pass)
    _same(got, exp, (name, mode, can_pass, "table vs oracle"))
    s1, s2 = capi.knn_edges(nodes, nbr)
    h1, h2 = I.knn_table_edges(name)
    assert np.array_equal(s1, h1) and np.array_equal(s2, h2)
    _same(got, w.check_motions(s1, s2, can_pass, mode), (name, mode, can_pass, "table vs endpoint arrays"))
    w.close()


@_case
def test_motions_across_kernels(name, mode, can_pass, monkeypatch):
    """The same edges through the cell-list kernels (EPP_MOTIONS_KERNEL=v4) and the generic
    k_motions (=generic): the oracle's flags again, so a difference above says which side is
    wrong."""
    w = _world(name)
    s1, s2 = I.motion_edges(name)
    exp = I.exp_motions(name, mode, can_pass)
    for impl in ("v4", "generic"):
        monkeypatch.setenv("EPP_MOTIONS_KERNEL", impl)
        _same(w.check_motions(s1, s2, can_pass, mode), exp, (name, mode, can_pass, impl))
    w.close()


@pytest.mark.parametrize("name", I.WORLDS)
def test_states_against_the_oracle(name, monkeypatch):
    """check_states and check_states_mindist on the same worlds, whose candidate lists are
    hundreds of OBBs long: the staged part runs from k_states_v5's budget to past it
    (k_states_v4)."""
    _default_kernels(monkeypatch)
    w = _world(name)
    pts = I.state_points(name)
    for cp in (0, 1):
        _same(w.check_states(pts, cp), I.exp_states(name, cp), (name, "states", cp))
    _same(w.check_states_mindist(pts, I.MIN_DISTANCE), I.exp_mindist(name), (name, "mindist"))
    w.close()
