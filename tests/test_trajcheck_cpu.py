"""CPU: the argument checks of epp_traj_check_batch (they precede every device call, so they
run without a GPU) and the host side of the shared sampling recurrence (csrc/traj_sample.h's
RangeIter, compiled into a small stand-alone program) against the oracle's row count."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
from eppamd import capi, synth

from conftest import PKG, ROOT

EPP_ERR_INVALID_ARGUMENT = -1


def _call(world, T, Cf, off, n, dt, rows, md=0.1, times=None):
    return capi.lib().epp_traj_check_batch(world, T, Cf, off, n, dt, md, rows, times, None)


def test_symbol_and_argument_checks():
    L = capi.lib()
    assert hasattr(L, "epp_traj_check_batch") and "epp_traj_check_batch" in capi.EXPORTED
    # stand-ins for device pointers: every case below is rejected before anything is read
    buf = np.zeros(64)
    p = buf.ctypes.data
    world = C.c_void_p(p)  # (a non-NULL handle; never dereferenced by a rejected call)
    cases = {
        "NULL world": (None, p, p, p, 1, 0.05, p),
        "n_tracks < 0": (world, p, p, p, -1, 0.05, p),
        "dt == 0": (world, p, p, p, 1, 0.0, p),
        "dt < 0": (world, p, p, p, 1, -0.05, p),
        "dt NaN": (world, p, p, p, 1, float("nan"), p),
        "dt inf": (world, p, p, p, 1, float("inf"), p),
        "NULL seg_times": (world, None, p, p, 1, 0.05, p),
        "NULL coeffs": (world, p, None, p, 1, 0.05, p),
        "NULL wp_offsets": (world, p, p, None, 1, 0.05, p),
        "NULL first_invalid": (world, p, p, p, 1, 0.05, None),
    }
    for name, (w, T, Cf, off, n, dt, rows) in cases.items():
        rc = _call(w, T, Cf, off, n, dt, rows)
        assert rc == EPP_ERR_INVALID_ARGUMENT, name
        assert b"epp_traj_check_batch" in L.epp_last_error(), name
    # an empty batch is fine, with or without buffers, and launches nothing
    assert _call(world, None, None, None, 0, 0.05, None) == capi.EPP_OK
    assert _call(world, p, p, p, 0, 0.05, p, times=p) == capi.EPP_OK


@pytest.fixture(scope="module")
def rows_host(tmp_path_factory):
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(cxx):
        cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("trajrows") / "traj_rows_host")
    # -ffp-contract=off as the library: the recurrence is plain additions either way
    cc = subprocess.run([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"),
                         os.path.join(ROOT, "tests", "traj_rows_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, f"compiling tests/traj_rows_host.cpp with {cxx} failed:\n{cc.stderr}"
    return exe


def _tracks(dt):
    """Ragged tracks (1..30 segments, the GPU tests' batch) and exact multiples of dt."""
    tracks = [synth.random_track_waypoints(900 + k, 1 + (k * 7) % 30) for k in range(24)]
    Ts = [O.segment_times(wp, 1.0, 2.0) for wp in tracks]
    return Ts + [np.array([0.5, 0.25, 1.0]), np.array([dt * 512]), np.array([dt * 511.5]), np.array([dt / 2])]


def _run(rows_host, mode, dt, Ts):
    args = []
    for T in Ts:  # one run for all tracks
        args += (["/"] if args else []) + [repr(float(t)) for t in T]
    run = subprocess.run([rows_host] + mode + [repr(float(dt))] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return run.stdout.splitlines()


@pytest.mark.parametrize("dt", [0.05, 0.01, 0.1])
def test_host_recurrence_row_count_equals_oracle(rows_host, dt):
    Ts = _tracks(dt)
    Cs = [np.zeros((len(t), 3, 10)) for t in Ts]  # (the rows' times do not depend on the coefficients)
    lines = _run(rows_host, [], dt, Ts)
    assert len(lines) == len(Ts)
    for T, Cf, line in zip(Ts, Cs, lines):
        out = line.split()
        ref = O.sample_traj(T, Cf, dt)
        assert int(out[0]) == len(ref), (T, out)
        if len(ref):
            assert float(out[1]) == ref[-1, 9], (T, out)


CAPS = (1, 7, 8, 9, 512, 513)


@pytest.mark.parametrize("dt", [0.05, 0.01, 0.1])
def test_producer_equals_single_steps_at_every_cap(rows_host, dt):
    """The shared stepping loop (range_produce: eight samples at once where it may, else one)
    gives the samples of plain next / advance steps -- segment, time in the segment and time,
    compared as printed hex floats, so bit for bit -- whatever room each call is given (below,
    at and above the eight of the shortcut, at and above a kernel's chunk), and range_count
    their number."""
    Ts = _tracks(dt)
    lines = _run(rows_host, ["samples"], dt, Ts)
    per = 1 + len(CAPS)
    assert len(lines) == per * len(Ts)
    for k, T in enumerate(Ts):
        head, _, step = lines[per * k].partition(" |")
        way, n, counted = head.split()
        assert way == "step" and int(n) == len(step.split()) // 3 and int(counted) == int(n), (T, head)
        assert int(n) > 0
        for cap, line in zip(CAPS, lines[per * k + 1:per * (k + 1)]):
            head, _, got = line.partition(" |")
            assert head == f"cap{cap} {n}", (T, head, n)
            if got != step:
                a, b = step.split(), got.split()
                j = next(i for i in range(len(a)) if a[i] != b[i])
                raise AssertionError((T, cap, "sample", j // 3, a[j - j % 3:j - j % 3 + 3], b[j - j % 3:j - j % 3 + 3]))
