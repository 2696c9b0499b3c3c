"""CPU: the restatement of the time scaling to thrust, body-rate and tilt limits
(thrust_scale_ref.py) against closed forms, the comparisons of the GPU test against five
mistakes, the shared header (csrc/thrust_scale.h) compiled into a stand-alone host program
against the restatement, the presence of the new surface and the argument checks."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import thrust_scale_inputs as si
import thrust_scale_ref as sr

from conftest import PKG, ROOT


# ---- closed forms ------------------------------------------------------------------------------
def test_grid_points_and_derivatives():
    c = np.zeros((1, 3, 10))
    c[0, 0] = np.arange(1.0, 11.0)
    g = sr.Grid([2.0], c)
    assert len(g.time) == 65 and g.time[0] == 0.0 and g.time[1] == 2.0 / 64 and g.time[64] == 2.0
    # small integers at t = 2: exact whichever way they are summed
    for k in (2, 3):
        exp = sum(sr.falling(j, k) * c[0, 0, j] * 2.0 ** (j - k) for j in range(k, 10))
        assert sr.deriv(c[0, 0], 2.0, k) == exp
    assert g.acc[64, 0] == sr.deriv(c[0, 0], 2.0, 2) and g.jerk[0, 0] == 6.0 * c[0, 0, 3]
    g = sr.Grid([0.5, 0.25, 1.0], np.zeros((3, 3, 10)))
    assert len(g.time) == 195 and g.time[65] == 0.5 and g.time[129] == 0.75 and g.time[130] == 0.75
    assert g.time[-1] == 1.75


def test_scaled_quantities_closed_forms():
    T, C = si.one({(0, 2): si.A / 2.0})
    f, w, c = sr.Grid(T, C).at(1.5, si.G)
    assert (f == 16.25).all() and (w == 0.0).all() and (c == si.G / 16.25).all()
    T, C = si.one({(0, 3): 32.90625 / 6.0})
    f, w, c = sr.Grid(T, C).at(1.5, si.G)
    assert w[0] == 1.0 and (w[1:] < 1.0).all() and f[0] == si.G
    T, C = si.one({(2, 2): -si.G / 2.0})  # free fall: NaN rate and cos_tilt violate nothing
    q = sr.Grid(T, C).at(1.0, si.G)
    assert (q[0] == 0.0).all() and np.isnan(q[1]).all() and np.isnan(q[2]).all()
    assert sr.violation(q, si.L_FALL) == sr.F_MIN


def test_search_closed_forms():
    # feasible from s0 on: the answer is the first of the search's dyadic scales at or above s0
    for s0 in (1.0, 1.5, 1.0 + 2.0 ** -12, 3.3, 700.0, 1024.0):
        scale, status, first, seen = sr.search(lambda s: 0 if s >= s0 else 5)
        assert status == 0 and scale >= s0 and (scale == 1.0 or scale - s0 < scale * 2.0 ** -12)
        assert first == (0 if s0 == 1.0 else 5) and len(seen) <= 1 + sr.MAX_DOUBLINGS + sr.BISECT_ROUNDS
        if scale > 1.0:
            assert len(seen) == 1 + int(np.ceil(np.log2(max(s0, 2.0)))) + sr.BISECT_ROUNDS
    scale, status, first, seen = sr.search(lambda s: 2)
    assert (scale, status, first) == (1.0, 1, 2) and seen == [1.0] + [2.0 ** k for k in range(1, 11)]
    # every scale visited is dyadic with at most 13 significant bits
    _, _, _, seen = sr.search(lambda s: 0 if s >= 777.7 else 1)
    assert all(float(s * 8) == int(s * 8) and int(s * 8) % (1 << max(0, int(s * 8).bit_length() - 13)) == 0
               for s in seen)


def test_apply_is_one_round_of_the_time_scaling():
    rs = np.random.RandomState(3)
    T, C = rs.uniform(0.5, 2.0, 4), rs.uniform(-2, 2, (4, 3, 10))
    Tn, Cn = sr.apply(T, C, 1.5)
    inv, f = 1.0 / 1.5, 1.0
    for n in range(10):
        assert (Cn[:, :, n] == C[:, :, n] * f).all()
        f = f * inv
    assert (Tn == T * 1.5).all() and (sr.apply(T, C, 1.0)[1] == C).all()


def test_limits_conditions():
    ok = sr.Limits(9.81, 0.0, np.inf, np.inf, -1.0)
    assert sr.limits_ok(ok) and sr.limits_ok(si.L_FIT) and all(sr.limits_ok(g.limits) for g in si.hand_groups())
    for bad in (ok._replace(g=0.0), ok._replace(g=np.inf), ok._replace(g=np.nan), ok._replace(f_min=-1.0),
                ok._replace(f_min=9.81), ok._replace(f_max=9.81), ok._replace(rate_max=0.0),
                ok._replace(cos_tilt_min=1.0), ok._replace(cos_tilt_min=np.nan), ok._replace(f_max=np.nan)):
        assert not sr.limits_ok(bad), bad


# ---- the GPU test's comparisons reject five mistakes -------------------------------------------
@functools.lru_cache(maxsize=None)
def _fitted():
    fT, fC, _ = O.minsnap_batch(list(si.fit_waypoints()[:12]), si.V_MAX, si.A_MAX, threads=8)
    return list(fT), list(fC)


@pytest.mark.parametrize("variant", sr.VARIANTS[1:])
def test_mutations_are_rejected(variant):
    bad_hand, bad_grid = [], []
    for g in si.hand_groups():
        exp = sr.scale_tracks(g.Ts, g.Cs, g.limits)
        assert sr.compare_results(exp, exp) == []
        bad_hand += [(g.name, b) for b in sr.compare_results(sr.scale_tracks(g.Ts, g.Cs, g.limits, variant), exp)]
        if variant in ("a / s3", "reciprocal", "tau = T dropped"):  # (the grid call has no search)
            e = np.array([sr.grid_extremes(T, C, 1.5, g.limits.g)[0] for T, C in zip(g.Ts, g.Cs)])
            v = np.array([sr.grid_extremes(T, C, 1.5, g.limits.g, variant)[0] for T, C in zip(g.Ts, g.Cs)])
            every = [[True] * 4] * len(e)
            assert sr.compare_grid(e, e, every) == []
            bad_grid += [(g.name, b) for b in sr.compare_grid(v, e, every)]
    fT, fC = _fitted()
    exp = sr.scale_tracks(fT, fC, si.L_FIT)
    bad_fit = sr.compare_results(sr.scale_tracks(fT, fC, si.L_FIT, variant), exp)
    print(variant, len(bad_hand), len(bad_grid), len(bad_fit), bad_hand[:4])
    assert bad_hand  # every mistake shows on the hand-built tracks' exact answers
    if variant == "tau = T dropped":
        assert bad_grid
    if variant in ("a / s3", "hi from an infeasible mid", "11 rounds"):
        assert bad_fit


# ---- the shared header on the host -------------------------------------------------------------
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
                         os.path.join(PKG, "csrc"), src or os.path.join(ROOT, "tests", "thrust_scale_host.cpp"), "-o",
                         exe], capture_output=True, text=True)
    return exe, cc


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    """[(what, program)]: the plain build and one with AddressSanitizer and UBSan (a program with
    its own main: nothing is preloaded).  Whether the compiler has the sanitizers' runtimes is
    asked with an empty program; where it has, the host program must build with them too."""
    tmp = tmp_path_factory.mktemp("thrustscale")
    exe, cc = _compile(tmp, [], "thrust_scale_host")
    assert cc.returncode == 0, f"compiling tests/thrust_scale_host.cpp failed:\n{cc.stderr}"
    exes = [("plain", exe)]
    empty = tmp / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe, cc = _compile(tmp, SAN, "empty_san", str(empty))
    if cc.returncode != 0 or subprocess.run([probe]).returncode != 0:
        print(f"sanitized variant NOT run: {_cxx()} cannot build or run an empty program with {SAN[1]}")
        return exes
    san, cc = _compile(tmp, SAN, "thrust_scale_host_san")
    assert cc.returncode == 0, f"compiling tests/thrust_scale_host.cpp with {SAN[1]} failed:\n{cc.stderr}"
    return exes + [("address,undefined", san)]


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _run(exe, mode, records):
    run = subprocess.run([exe, mode], input="\n".join(records) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    lines = run.stdout.splitlines()
    assert len(lines) == len(records)
    return [l.split() for l in lines]


def _host_scale(exe, Ts, Cs, L):
    recs = [f"{float(len(np.ravel(T))).hex()} {_hex(L)} {_hex(np.ravel(T))} {_hex(np.ravel(C))}" for T, C in zip(Ts, Cs)]
    out = []
    for T, words in zip(Ts, _run(exe, "scale", recs)):
        M = len(np.ravel(T))
        vals = [float.fromhex(w) for w in words[3:]]
        out.append((float.fromhex(words[0]), int(words[1]), int(words[2]), np.array(vals[:M]),
                    np.array(vals[M:]).reshape(M, 3, 10)))
    return out


def test_host_program_equals_restatement(host_programs):
    fT, fC = _fitted()
    print("host programs run:", [what for what, _ in host_programs])
    for what, exe in host_programs:
        for g in si.hand_groups():
            exp = sr.scale_tracks(g.Ts, g.Cs, g.limits)
            assert sr.compare_results(_host_scale(exe, g.Ts, g.Cs, g.limits), exp) == [], (what, g.name)
        exp = sr.scale_tracks(fT, fC, si.L_FIT)
        assert sum(r.scale > 1.0 for r in exp) >= 8
        assert sr.compare_results(_host_scale(exe, fT, fC, si.L_FIT), exp) == [], what
        # the grid extremes: bit for bit too (the host's square root is the restatement's)
        g = si.hand_groups()[0]
        Ts, Cs = list(g.Ts) + fT, list(g.Cs) + fC
        for s in (1.0, 1.5):
            recs = [f"{float(len(np.ravel(T))).hex()} {_hex([si.GRAVITY, s])} {_hex(np.ravel(T))} {_hex(np.ravel(C))}"
                    for T, C in zip(Ts, Cs)]
            got = np.array([[float.fromhex(w) for w in words] for words in _run(exe, "grid", recs)])
            want = np.array([sr.grid_extremes(T, C, s, si.GRAVITY)[0] for T, C in zip(Ts, Cs)])
            assert got.tobytes() == want.tobytes(), (what, s, np.argwhere(got != want)[:4].tolist())


# ---- surface -----------------------------------------------------------------------------------
NEW = ("epp_traj_thrust_grid_batch", "epp_traj_scale_to_thrust_limits", "epp_generate_trajectory_flyable_host")


def test_surface():
    from eppamd import capi
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTED
    assert callable(capi.thrust_grid) and callable(capi.scale_to_thrust_limits)
    assert callable(capi.generate_trajectory_flyable)
    import online_traj_planner as otp
    import polynomial_trajectory as pt
    assert hasattr(otp.PathPlanner, "candidate_flyable_scales")
    assert "thrustLimits" in pt.generate_trajectory.__doc__
    for h in ("thrust_scale.h", "poly_deriv.h"):
        assert os.path.exists(os.path.join(PKG, "csrc", h))
    header = open(os.path.join(ROOT, "include", "epp.h")).read()
    assert all(name + "(" in header for name in NEW)
