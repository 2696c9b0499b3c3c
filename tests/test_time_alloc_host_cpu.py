"""CPU: the shared header csrc/time_alloc.h compiled into a stand-alone host program
(tests/host/time_alloc_main.cpp, its own main), plain and with AddressSanitizer and UBSan,
against the truth values of tests/golden/time_alloc_costs.json and the restatement."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import time_alloc_ref as tr

from conftest import GOLDEN, PKG, ROOT

SRC = os.path.join(ROOT, "tests", "host", "time_alloc_main.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _cxx():
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(cxx):
        cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    return cxx


def _compile(tmp, extra, name, src=SRC):
    exe = str(tmp / name)
    cc = subprocess.run([_cxx(), "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-I",
                         os.path.join(PKG, "csrc"), src, "-o", exe], capture_output=True, text=True)
    return exe, cc


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    """[(what, program)]: the plain build and, where the compiler has the sanitizers' runtimes
    (asked with an empty program), one with them; nothing is preloaded."""
    tmp = tmp_path_factory.mktemp("timealloc")
    exe, cc = _compile(tmp, [], "time_alloc_main")
    assert cc.returncode == 0, f"compiling {SRC} failed:\n{cc.stderr}"
    exes = [("plain", exe)]
    empty = tmp / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe, cc = _compile(tmp, SAN, "empty_san", str(empty))
    if cc.returncode != 0 or subprocess.run([probe]).returncode != 0:
        print(f"sanitized variant NOT run: {_cxx()} cannot build or run an empty program with {SAN[1]}")
        return exes
    san, cc = _compile(tmp, SAN, "time_alloc_main_san")
    assert cc.returncode == 0, f"compiling {SRC} with {SAN[1]} failed:\n{cc.stderr}"
    return exes + [("address,undefined", san)]


def _hex(values):
    return " ".join(float(v).hex() for v in np.ravel(values))


def _run(exe, mode, records):
    run = subprocess.run([exe, mode], input="\n".join(records) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    lines = run.stdout.splitlines()
    assert len(lines) == len(records)
    return [l.split() for l in lines]


def _golden():
    with open(os.path.join(GOLDEN, "time_alloc_costs.json")) as f:
        recs = json.load(f)
    out = []
    for r in recs:
        T = np.array([float.fromhex(x) for x in r["T"]])
        C = np.array([float.fromhex(x) for x in r["C"]]).reshape(len(T), 3, 10)
        out.append((r["name"], T, C, float.fromhex(r["cost"]), float.fromhex(r["scale"])))
    return out


def test_golden_file_is_the_restatement():
    for name, T, C, J, A in _golden():
        assert tr.cost(T, C) == J and tr.cost_abs(T, C) == A, name


def test_host_cost_equals_truth(host_programs):
    gold = _golden()
    print("host programs run:", [what for what, _ in host_programs])
    answers = []
    for what, exe in host_programs:
        recs = [f"{float(len(T)).hex()} {_hex(T)} {_hex(C)}" for _, T, C, _, _ in gold]
        out = _run(exe, "cost", recs)
        for (name, T, C, J, A), words in zip(gold, out):
            got = float.fromhex(words[0])
            print(what, name, got, J, abs(got - J) / (tr.EPS * A))
            # both sum 36 products per polynomial
            assert int(words[1]) == 0 and abs(got - J) <= 64 * tr.EPS * A, (what, name)
        answers.append([w[0] for w in out])
        # invalid tracks: a time <= 0, a NaN time, a NaN coefficient, no segment
        _, T, C, _, _ = gold[1]
        bad = []
        for i, v in ((0, 0.0), (1, -1.0), (2, float("nan")), (0, float("inf"))):
            Tb = T.copy()
            Tb[i] = v
            bad.append(f"{float(len(T)).hex()} {_hex(Tb)} {_hex(C)}")
        Cb = C.copy()
        Cb[2, 1, 7] = float("nan")
        bad.append(f"{float(len(T)).hex()} {_hex(T)} {_hex(Cb)}")
        bad.append(float(0).hex())
        for words in _run(exe, "cost", bad):
            assert np.isnan(float.fromhex(words[0])) and int(words[1]) == -1
    assert all(a == answers[0] for a in answers)  # the sanitized build computes the same bits


def test_host_times_and_direction_equal_restatement(host_programs):
    rs = np.random.RandomState(11)
    for what, exe in host_programs:
        for M in (2, 3, 7):
            T = rs.uniform(0.1, 2.0, M)
            T[0] = 0.11
            V = tr.variants(T, 0.1, 0.1)
            recs = [f"{float(M).hex()} {float(n).hex()} {_hex([0.1, 0.1])} {_hex(T)}" for n in range(M)]
            got = np.array([[float.fromhex(w) for w in words] for words in _run(exe, "times", recs)])
            assert got.tobytes() == V[1:].tobytes(), (what, M)
            g = rs.uniform(-50, 50, M)
            got = np.array([float.fromhex(w) for w in _run(exe, "dir", [f"{float(M).hex()} {_hex(g)}"])[0]])
            assert got.tobytes() == tr.direction(g).tobytes(), (what, M)
