"""GPU: the exact k-NN at the edges of its argument, every route against the numpy reference.

The four k-NN kernels have one answer (knn_kernels.h): candidates ranked by (distance, index),
in range iff the squared distance is < max_dist^2.  The cases of knn_edge_inputs.py stand where
that is under load (test_knn_edge_inputs_cpu.py proves that they reach those branches): squared
radii attained exactly, both sides of the switch between the all-pairs kernel and the grid,
tables smaller than K, one-cell worlds, a capped and clamped axis, empty and crowded grids,
radii below and beyond the tile pass's reach, clouds far from the origin, a caller box far
wider than the nodes.

Every case runs on every route for K = 4, 8, 16 and 32, and the table must be the reference's
(knn_ref, computed once per case for K = 32 and sliced).  On a mismatch the number of differing
rows is printed, and the first ten with their got and expected rows and squared distances.
"""
import numpy as np
import pytest

from eppamd import capi

import knn_edge_inputs as I

pytestmark = pytest.mark.gpu

# route -> (capi.knn method, EPP_KNN_TILE or None for the default)
ROUTES = {
    "brute": ("brute", None),
    "grid_tile1": ("grid", "1"),
    "grid_tile0": ("grid", "0"),
    "grid_ws": ("grid_ws", None),
    "ws": ("ws", None),
}
BOX_ROUTES = {"grid_ws_box": "grid_ws", "ws_box": "ws"}
BOXED = tuple((n, "own") for n in I.NAMES if I.cases()[n]["box"] is not None) + tuple((n, "tight") for n in I.TIGHT_BOX)


def _env(monkeypatch, tile):
    monkeypatch.delenv("EPP_KNN_IMPL", raising=False)
    if tile is None:
        monkeypatch.delenv("EPP_KNN_TILE", raising=False)
    else:
        monkeypatch.setenv("EPP_KNN_TILE", tile)


class _Diffs:
    """Collects got != expected per table; check() fails with every table that differed: how many
    rows, and the first ten with both rows and their squared distances."""

    def __init__(self, name):
        self.name, self.nodes, self.msgs = name, I.cases()[name]["nodes"], []

    def _row(self, i, row):
        d2 = I.sq_dists(self.nodes, i)
        return " ".join(f"{j}:{d2[j]:.17g}" if j >= 0 else "-1" for j in row)

    def same(self, got, k, what):
        exp = I.reference(self.name)[:, :k]
        assert got.shape == exp.shape, (what, got.shape, exp.shape)
        bad = np.flatnonzero((got != exp).any(1))
        if len(bad):
            c = I.cases()[self.name]
            lines = [f"{self.name} {what} k {k} max_dist^2 {c['max_dist'] ** 2:.17g}: {len(bad)} of {len(exp)} rows differ"]
            for i in bad[:10]:
                lines.append(f"    row {i} got      {self._row(i, got[i])}")
                lines.append(f"    row {i} expected {self._row(i, exp[i])}")
            self.msgs.append("\n".join(lines))

    def check(self):
        if self.msgs:
            msg = "\n".join(self.msgs)
            print(msg)
            pytest.fail(msg)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", I.NAMES)
def test_table_is_the_reference(name, route, monkeypatch):
    method, tile = ROUTES[route]
    _env(monkeypatch, tile)
    c = I.cases()[name]
    d = _Diffs(name)
    for k in I.KS:
        d.same(capi.knn(c["nodes"], k, c["max_dist"], method=method), k, route)
    d.check()


@pytest.mark.parametrize("route", BOX_ROUTES)
@pytest.mark.parametrize("name,which", BOXED)
def test_table_under_a_caller_box(name, which, route, monkeypatch):
    """The two caller-box entry points: the case's own box, or the nodes' tight bounding box."""
    _env(monkeypatch, None)
    c = I.cases()[name]
    box = c["box"] if which == "own" else I.tight_box(name)
    d = _Diffs(name)
    for k in I.KS:
        d.same(capi.knn(c["nodes"], k, c["max_dist"], method=BOX_ROUTES[route], box=box), k, f"{route} {which} box")
    d.check()


@pytest.mark.parametrize("name", ["switch_2048", "switch_2049"])
def test_switch_auto(name, monkeypatch):
    """epp_knn picks the all-pairs kernel up to 2048 nodes and the grid from 2049: the reference
    on both sides."""
    _env(monkeypatch, None)
    c = I.cases()[name]
    d = _Diffs(name)
    for k in I.KS:
        d.same(capi.knn(c["nodes"], k, c["max_dist"], method="auto"), k, "auto")
    d.check()
