"""CPU: the planner's host graph searches (csrc/graph_search.h) and per-problem geometry
(csrc/plan_geometry.h), compiled into a small stand-alone program (tests/graph_search_host.cpp)
that checks the searches against a plain restatement of its own -- std::priority_queue of
(f, node), plain dist / prev / closed vectors, no stamps -- and prints one line per check; the
geometry is restated here in numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(cxx):
        cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("graphsearch") / "graph_search_host")
    # -ffp-contract=off as the library
    cc = subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "graph_search_host.cpp"),
                         "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, f"compiling tests/graph_search_host.cpp with {cxx} failed:\n{cc.stderr}"
    return exe


def _lines(host, *args):
    run = subprocess.run([host] + [str(a) for a in args], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert lines
    bad = [ln for ln in lines if not ln.endswith(" ok")]
    assert not bad, bad
    return lines


def _field(line, name):
    w = line.split()
    return int(w[w.index(name) + 1])


SEEDS = list(range(1, 13))


@pytest.mark.parametrize("k", [4, 8, 16])
@pytest.mark.parametrize("n", [2, 3, 64, 2000])
def test_astar_equals_plain_restatement(host, n, k):
    """Seeded k-NN graphs of uniform points, 30 % of the edges masked, node 0 -> node 1: code,
    path (node indices, positions bit for bit) and closed nodes of the forward and the
    symmetrised whole-table search, wide and narrow, equal the restatement's; n = 2 also with
    and without its one edge."""
    lines = _lines(host, "astar", n, k, *SEEDS)
    assert len(lines) == len(SEEDS) + 2
    fwd = [_field(ln, "forward") for ln in lines[:len(SEEDS)]]
    assert set(fwd) <= {0, 1}
    if k == 4 and n >= 64:  # (sparse enough: some seeds leave the goal unreachable, some do not)
        assert 0 in fwd and 1 in fwd, fwd
    assert [_field(ln, "forward") for ln in lines[len(SEEDS):]] == [0, 1]


def test_ties_pop_the_lower_index_first(host):
    """A 9 x 9 x 1 unit lattice, opposite corners, the 4 axis neighbours: many nodes share f;
    same path and same closed nodes as std::priority_queue<pair<double, int>, ..., greater<>>."""
    (line,) = _lines(host, "ties")
    assert _field(line, "forward") == 1 and _field(line, "path") == 17


def test_stamps_wrap_and_reuse(host):
    """Searches on one SearchState across the stamp's wrap-around (cur preset to 0xFFFFFFFE),
    and n = 64 after n = 2000, equal the restatement (which starts fresh every time)."""
    assert len(_lines(host, "stamps")) == 2


# n = 2000, k = 4, bound 1.25 |s g| + 0.05: the seeds of each outcome, found by running the
# program over seeds 1..400 -- forward reaches the goal within the bound (1); forward
# exhausted, then symmetrised reaches it (0 then 1); forward exhausted, symmetrised pops above
# the bound (0 then -1); forward pops above the bound (-1)
ROWS_K4 = {169: (1, -2), 242: (1, -2), 275: (1, -2), 297: (1, -2), 384: (0, 1), 28: (0, -1), 43: (0, -1),
           1: (-1, -2), 2: (-1, -2), 3: (-1, -2)}


def test_rows_equal_whole_table(host):
    """The rows as the device builds them (the nodes inside the ellipsoid, compact node order,
    row_of = -1 outside): a forward search on them that returns 1 gives the whole table's
    forward path and pops; one that returns 0 means the whole table's fails too, and a
    symmetrised search on the rows that then returns 1 gives the whole table's symmetrised
    path and pops.  Every outcome occurs."""
    lines = _lines(host, "rows", 2000, 4, 1.25, *ROWS_K4)
    got = {_field(ln, "seed"): (_field(ln, "forward"), _field(ln, "symmetrised")) for ln in lines}
    assert got == ROWS_K4
    seen = set(got.values())
    assert {(1, -2), (0, 1), (-1, -2)} <= seen
    # the same outcomes on row sets of hundreds of nodes (bound 2 |s g| + 0.05; seeds found as
    # above): "0 then 1" with 45..269 nodes closed by the symmetrised search, "1" with 72..727
    for seeds, want in (((59, 64, 137, 129, 170, 43), (0, 1)), ((3, 6, 14, 20, 47, 48), (1, -2))):
        lines = _lines(host, "rows", 2000, 4, 2.0, *seeds)
        assert all((_field(ln, "forward"), _field(ln, "symmetrised")) == want for ln in lines), lines
        assert all(_field(ln, "nodes") >= 400 and _field(ln, "closed") >= 45 for ln in lines), lines
    # denser graphs and the small size: whatever the outcome, the lines end in ok; most reach the goal
    for n, k in ((2000, 8), (2000, 16), (64, 4), (64, 16), (3, 4)):
        lines = _lines(host, "rows", n, k, 1.25, *range(1, 11))
        if (n, k) == (2000, 16):
            assert sum(_field(ln, "forward") == 1 for ln in lines) >= 5
    # bound = |s g| + 0.05: seed 43's rows exhaust both searches (0 then 0)
    (line,) = _lines(host, "rows", 2000, 4, 1.0, 43)
    assert (_field(line, "forward"), _field(line, "symmetrised")) == (0, 0)


@pytest.mark.parametrize("n,k", [(64, 4), (2000, 8), (2000, 16)])
def test_reverse_csr_on_rows(host, n, k):
    """RowsReverse::build equals, for every v, the ascending u with v in row(u) -- also for a
    made-up row that lists a node twice (a k-NN row holds k distinct nodes, so the device
    emits none) and into a scratch with stale contents."""
    lines = _lines(host, "csr", n, k, 1, 2, 3)
    assert len(lines) == 4 and all(_field(ln, "edges") > 0 for ln in lines)


LO, HI = np.array([-6.0, -6.0, 0.0]), np.array([6.0, 6.0, 2.0])


def _geometry(host, s, g, nmax, ellipse, restrict_ok, lo=LO, hi=HI):
    run = subprocess.run([host, "geometry"] + [repr(float(x)) for x in (*s, *g, *lo, *hi)] +
                         [str(nmax), repr(float(ellipse)), str(int(restrict_ok))], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    v = run.stdout.split()
    f = [float(x) for x in v]
    return dict(bound=f[0], gbound=f[1], h=f[2], cap=int(v[3]), klo=np.array(f[4:7]), khi=np.array(f[7:10]),
                glo=np.array(f[10:13]), ghi=np.array(f[13:16]))


def _want(s, g, nmax, ellipse, restrict_ok, lo=LO, hi=HI):
    """The numpy restatement: cells of ~1.5 nodes, bound = ellipse |s g| + 0.25, the grid bound
    7.5 cells wider, capacity 1.25 x volume fraction x nmax + 1024 and 0 when not below nmax / 2."""
    s, g = np.asarray(s, float), np.asarray(g, float)
    vbox = float(np.prod(hi - lo))
    h = (1.5 * vbox / nmax) ** (1.0 / 3.0)
    d = float(np.linalg.norm(g - s))
    bound = ellipse * d + 0.25
    vell = np.pi * bound * (bound * bound - d * d) / 6.0
    want = 1.25 * min(1.0, vell / vbox) * nmax + 1024.0
    cap = int(want) if restrict_ok and want < 0.5 * nmax else 0
    return dict(bound=bound, gbound=bound + 7.5 * h, h=h, cap=cap, klo=np.minimum(lo, np.minimum(s, g)),
                khi=np.maximum(hi, np.maximum(s, g)))


GEOMETRY = [  # start, goal, nmax, ellipse
    ((1.0, 2.0, 1.0), (1.0, 2.0, 1.0), 65538, 1.25),      # d_sg = 0
    ((-1.0, 0.5, 0.6), (1.5, -0.75, 1.4), 65538, 1.25),   # a short segment: cap > 0
    ((-5.5, -5.0, 0.2), (5.5, 5.25, 1.8), 65538, 1.25),   # a long one: want >= nmax / 2, cap = 0
    ((-6.5, 0.0, 1.0), (2.0, 6.25, 2.5), 4098, 1.0),      # ends outside the sampling box widen the k-NN box
]


@pytest.mark.parametrize("case", range(len(GEOMETRY)))
def test_plan_geometry(host, case):
    s, g, nmax, ellipse = GEOMETRY[case]
    got = _geometry(host, s, g, nmax, ellipse, True)
    want = _want(s, g, nmax, ellipse, True)
    for key in ("bound", "gbound", "h"):
        assert got[key] == pytest.approx(want[key], rel=1e-13, abs=0), key
    assert got["cap"] == want["cap"]
    assert (got["cap"] > 0) == (case != 2)  # (only the long segment's ellipsoid holds half the nodes)
    assert np.array_equal(got["klo"], want["klo"]) and np.array_equal(got["khi"], want["khi"])
    assert _geometry(host, s, g, nmax, ellipse, False)["cap"] == 0
    # the box: inside the k-NN box, and around every point of the gbound ellipsoid that lies in the k-NN box
    assert np.all(got["glo"] >= got["klo"]) and np.all(got["ghi"] <= got["khi"])
    s, g = np.asarray(s), np.asarray(g)
    rng = np.random.default_rng(1234 + case)
    a = 0.5 * got["gbound"]
    pts = np.empty((0, 3))
    while len(pts) < 10000:  # (rejection sampling in the cube around the ellipsoid's bounding sphere)
        x = 0.5 * (s + g) + rng.uniform(-a, a, (40000, 3))
        keep = np.linalg.norm(x - s, axis=1) + np.linalg.norm(x - g, axis=1) <= got["gbound"]
        keep &= np.all(x >= got["klo"], axis=1) & np.all(x <= got["khi"], axis=1)
        pts = np.concatenate([pts, x[keep]])
    pts = pts[:10000]
    assert np.all(pts >= got["glo"]) and np.all(pts <= got["ghi"])
