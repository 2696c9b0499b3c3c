"""CPU: the restatement of the thrust / body-rate calls (thrust_rates_ref.py) against closed
forms, the comparisons of the GPU test against four mistakes, the shared headers
(csrc/thrust_rates.h, csrc/traj_sample.h) compiled into a stand-alone host program against the
restatement, and the presence of the new surface."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import clearance_ref as CR
import oracle as O
import thrust_rates_inputs as ti
import thrust_rates_ref as tr

from conftest import PKG, ROOT

G = 9.81


# ---- closed forms ------------------------------------------------------------------------------
def test_closed_forms():
    z = np.zeros((1, 3))
    f, w, c, _ = tr.samples(z, z, G)  # hover
    assert f[0] == G and w[0] == 0.0 and c[0] == 1.0
    f, w, c, _ = tr.samples([[G, 0.0, 0.0]], z, G)  # pure sideways acceleration a_x = g: 45 degrees
    assert CR.ulps(c, 1.0 / np.sqrt(2.0))[0] <= 1.0 and CR.ulps(f, G * np.sqrt(2.0))[0] <= 1.0
    # F perpendicular to j: |F x j| = |F| |j|, so the rate is |j| / |F|
    rs = np.random.RandomState(5)
    F = rs.uniform(-10, 10, (200, 3))
    j = np.cross(F, rs.uniform(-10, 10, (200, 3)))
    a = F - [0.0, 0.0, G]
    f, w, c, _ = tr.samples(a, j, G)
    exp = np.linalg.norm(j, axis=1) / np.linalg.norm(F, axis=1)
    assert np.abs(w / exp - 1.0).max() < 1e-12
    # F parallel to j: the thrust direction does not turn
    f, w, c, _ = tr.samples([[0.0, 0.0, 1.0]], [[0.0, 0.0, 5.0]], G)
    assert w[0] == 0.0 and c[0] == 1.0
    # free fall
    with np.errstate(all="ignore"):
        f, w, c, f2 = tr.samples([[0.0, 0.0, -G]], z, G)
    assert f2[0] == 0.0 and f[0] == 0.0 and np.isnan(w[0]) and np.isnan(c[0])
    # upside down
    f, w, c, _ = tr.samples([[0.0, 0.0, -3 * ti.G]], z, ti.G)  # (9.8125: every step exact)
    assert c[0] == -1.0 and f[0] == 2 * ti.G


def test_derivative_values():
    c = np.arange(1.0, 11.0)
    assert tr.deriv(c, 0.5, 9) == 362880.0 * c[9]  # order 9: a constant
    assert tr.deriv(c, 0.0, 3) == 6.0 * c[3] and tr.deriv(c, 0.0, 0) == c[0]
    # small integers: exact whichever way they are summed
    t = 2.0
    for k in range(10):
        exp = sum(tr.falling(j, k) * c[j] * t ** (j - k) for j in range(k, 10))
        assert tr.deriv(c, t, k) == exp, k
    assert tr.deriv(c, 0.25, 0) == CR.horner(c, 0.25)  # order 0: the fused Horner of the positions
    assert np.isnan(tr.deriv(c, np.nan, 2))


def test_reductions():
    t = np.arange(6) * 0.5
    nan, inf = np.nan, np.inf
    out, rows = tr.reduce([3.0, 1.0, nan, 1.0, 5.0, 5.0], [nan, 2.0, inf, 1.0, inf, 0.0], [nan] * 6, t)
    assert rows.tolist() == [1, 4, 2, -1]  # the earliest row among equals; NaN never; +inf does
    assert out.tolist() == [1.0, 0.5, 5.0, 2.0, inf, 1.0, inf, -1.0]
    out, rows = tr.reduce(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0))
    assert np.array_equal(out, tr.IDENTITY) and rows.tolist() == [-1] * 4
    out, rows = tr.reduce([inf, inf], [-inf, -inf], [inf, 0.5], [0.0, 1.0])
    assert rows.tolist() == [-1, 0, -1, 1]  # a value equal to the identity never updates


# ---- the GPU test's comparisons reject four mistakes -------------------------------------------
@functools.lru_cache(maxsize=None)
def _tracks():
    _, Ts, Cs, _, _ = ti.hand_tracks()
    fT, fC, _ = O.minsnap_batch(list(ti.fit_waypoints()[:8]), ti.V_MAX, ti.A_MAX, threads=8)
    return list(Ts) + list(fT), list(Cs) + list(fC)


@pytest.mark.parametrize("variant", tr.VARIANTS[1:])
def test_mutations_are_rejected(variant):
    Ts, Cs = _tracks()
    exp_out, exp_rows, exp = tr.tracks(Ts, Cs, ti.DT * 4, ti.G)
    assert tr.compare_tracks(exp_out, exp_rows, exp_out, exp_rows) == []
    got_out, got_rows, got = tr.tracks(Ts, Cs, ti.DT * 4, ti.G, variant)
    bad = tr.compare_tracks(got_out, got_rows, exp_out, exp_rows)
    print(variant, len(bad), bad[:6])
    assert bad
    if variant != "non-strict comparison":  # the per-sample comparison sees the arithmetic ones too
        k = len(Ts) - 1
        assert tr.compare_samples((got[k].thrust, got[k].rate, got[k].cos_tilt),
                                  (exp[k].thrust, exp[k].rate, exp[k].cos_tilt))
    else:
        assert {k for k, what in bad} >= {0} and all(what == "rows" or what[-2] in "1357" for _, what in bad)


def test_comparison_allows_the_roots_ulp_and_no_more():
    f = np.array([1.0, 2.0, np.inf, np.nan, 0.0])
    exp = (f, f, f)
    up1 = np.array([np.nextafter(1.0, 2.0), np.nextafter(2.0, 3.0), np.inf, np.nan, 0.0])
    up2 = np.array([np.nextafter(up1[0], 2.0), np.nextafter(up1[1], 3.0), np.inf, np.nan, 0.0])
    assert tr.compare_samples((up1, up2, up2), exp) == []
    assert tr.compare_samples((up2, f, f), exp) == [("thrust", 0), ("thrust", 1)]
    got = np.array([np.nextafter(np.nextafter(1.0, 2.0), 2.0), 2.0, np.nan, np.inf, 0.0])
    assert tr.compare_samples((got, f, f), exp) == [("thrust", 0), ("thrust", 2), ("thrust", 3)]


# ---- the shared headers on the host ------------------------------------------------------------
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _cxx():
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(cxx):
        cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    return cxx


def _compile(tmp, extra, name, src=None):
    exe = str(tmp / name)
    cc = subprocess.run([_cxx(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I",
                         os.path.join(PKG, "csrc"), src or os.path.join(ROOT, "tests", "thrust_rates_host.cpp"), "-o",
                         exe], capture_output=True, text=True)
    return exe, cc


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    """[(what, program)]: the plain build and one with AddressSanitizer and UBSan (a program with
    its own main: nothing is preloaded).  Whether the compiler has the sanitizers' runtimes is
    asked with an empty program; where it has, the host program must build with them too, so
    an error in the project's headers under those flags fails here and is not passed over."""
    tmp = tmp_path_factory.mktemp("thrustrates")
    exe, cc = _compile(tmp, [], "thrust_rates_host")
    assert cc.returncode == 0, f"compiling tests/thrust_rates_host.cpp failed:\n{cc.stderr}"
    exes = [("plain", exe)]
    empty = tmp / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe, cc = _compile(tmp, SAN, "empty_san", str(empty))
    if cc.returncode != 0 or subprocess.run([probe]).returncode != 0:
        print(f"sanitized variant NOT run: {_cxx()} cannot build or run an empty program with {SAN[1]}")
        return exes
    san, cc = _compile(tmp, SAN, "thrust_rates_host_san")
    assert cc.returncode == 0, f"compiling tests/thrust_rates_host.cpp with {SAN[1]} failed:\n{cc.stderr}"
    return exes + [("address,undefined", san)]


def _run(exe, mode, lines):
    text = "\n".join(" ".join(float(v).hex() for v in line) for line in lines) + "\n"
    run = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = [[float.fromhex(v) for v in l.split()] for l in run.stdout.splitlines()]
    assert len(out) == len(lines)
    return np.array(out)


def test_host_program_equals_restatement(host_programs):
    rs = np.random.RandomState(11)
    a = rs.uniform(-20, 20, (300, 3))
    j = rs.uniform(-50, 50, (300, 3))
    a[0], j[0] = 0.0, 0.0                      # hover
    a[1], j[1] = [0.0, 0.0, -ti.G], 0.0        # free fall
    a[2], j[2] = [2.0 ** -560, 0.0, -ti.G], [0.0, 6 * 2.0 ** 400, 0.0]  # x / 0
    a[3] = [np.nan, 1.0, 2.0]
    g = np.full((300, 1), ti.G)
    exp = tr.samples(a, j, ti.G)[:3]
    c = rs.uniform(-3, 3, (60, 10))
    c[:5, 6:] = 0.0
    t = rs.uniform(0, 4, (60, 1))
    t[0] = 0.0
    want = np.array([[tr.deriv(ci, ti_[0], k) for k in range(10)] + [tr.deriv(ci, ti_[0], 2), tr.deriv(ci, ti_[0], 3)]
                     for ci, ti_ in zip(c, t)])
    print("host programs run:", [what for what, _ in host_programs])
    for what, exe in host_programs:
        got = _run(exe, "samples", np.hstack([a, j, g]))
        assert tr.compare_samples(got.T, exp) == [], exe
        got = _run(exe, "deriv", np.hstack([t, c]))
        assert got.tobytes() == want.tobytes(), (exe, np.argwhere(got != want)[:4].tolist())


# ---- surface -----------------------------------------------------------------------------------
def test_surface():
    from eppamd import capi
    L = capi.lib()
    for name in ("epp_sample_derivative_batch", "epp_thrust_rates", "epp_traj_thrust_rates_batch"):
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.sample_derivative) and callable(capi.thrust_rates) and callable(capi.trajectory_thrust_rates)
    import online_traj_planner as otp
    assert hasattr(otp.PathPlanner, "candidate_thrust_rates")
    assert os.path.exists(os.path.join(PKG, "csrc", "thrust_rates.h"))


def test_argument_checks():
    """They precede every device call, so they run without a GPU."""
    from eppamd import capi
    L = capi.lib()
    p = np.zeros(64).ctypes.data  # a stand-in for device pointers: every case is rejected before anything is read
    nan, inf = float("nan"), float("inf")
    bad = capi.EPP_ERR_INVALID_ARGUMENT
    for name, a in {
        "order -1": (p, p, p, 1, 0.1, -1, p, p), "order 10": (p, p, p, 1, 0.1, 10, p, p),
        "n_tracks < 0": (p, p, p, -1, 0.1, 2, p, p), "dt 0": (p, p, p, 1, 0.0, 2, p, p),
        "dt < 0": (p, p, p, 1, -0.1, 2, p, p), "dt NaN": (p, p, p, 1, nan, 2, p, p),
        "dt inf": (p, p, p, 1, inf, 2, p, p), "NULL seg_times": (None, p, p, 1, 0.1, 2, p, p),
        "NULL coeffs": (p, None, p, 1, 0.1, 2, p, p), "NULL wp_offsets": (p, p, None, 1, 0.1, 2, p, p),
        "NULL values": (p, p, p, 1, 0.1, 2, p, None),
    }.items():
        assert L.epp_sample_derivative_batch(*a, None) == bad, name
        assert b"epp_sample_derivative_batch" in L.epp_last_error(), name
    for name, a in {
        "n < 0": (p, p, -1, G, p, p, p), "g NaN": (p, p, 1, nan, p, p, p), "g inf": (p, p, 1, inf, p, p, p),
        "NULL acc": (None, p, 1, G, p, p, p), "NULL jerk": (p, None, 1, G, p, p, p),
        "NULL thrust": (p, p, 1, G, None, p, p),
    }.items():
        assert L.epp_thrust_rates(*a, None) == bad, name
        assert b"epp_thrust_rates" in L.epp_last_error(), name
    for name, a in {
        "n_tracks < 0": (p, p, p, -1, 0.1, G, p, p), "dt 0": (p, p, p, 1, 0.0, G, p, p),
        "dt NaN": (p, p, p, 1, nan, G, p, p), "dt inf": (p, p, p, 1, inf, G, p, p),
        "g NaN": (p, p, p, 1, 0.1, nan, p, p), "g -inf": (p, p, p, 1, 0.1, -inf, p, p),
        "NULL seg_times": (None, p, p, 1, 0.1, G, p, p), "NULL coeffs": (p, None, p, 1, 0.1, G, p, p),
        "NULL wp_offsets": (p, p, None, 1, 0.1, G, p, p), "NULL out": (p, p, p, 1, 0.1, G, None, p),
    }.items():
        assert L.epp_traj_thrust_rates_batch(*a, None) == bad, name
        assert b"epp_traj_thrust_rates_batch" in L.epp_last_error(), name
    # empty batches are fine, with or without buffers, and launch nothing
    assert L.epp_sample_derivative_batch(None, None, None, 0, 0.1, 3, None, None, None) == capi.EPP_OK
    assert L.epp_thrust_rates(None, None, 0, G, None, None, None, None) == capi.EPP_OK
    assert L.epp_traj_thrust_rates_batch(None, None, None, 0, 0.1, G, None, None, None) == capi.EPP_OK
