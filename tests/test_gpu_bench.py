"""bench.py's plain run on the GPU: `--steps` sets the timed steps, the JSON line carries
ms_per_step, nothing but the headline runs without `--full`, and `--dump-outputs` writes
the flags of the last timed step (checked against the CPU oracle on the same states).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from eppamd import config, synth

from conftest import ROOT

pytestmark = pytest.mark.gpu

N_STATES = 1 << 20


def test_plain_run_dumps_last_step_flags(cfg, geom, tmp_path):
    steps = 19  # the last timed step checks resident batch (19 - 1) % 16 = 2
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", "2", "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "state validity checks/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(N_STATES / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # a plain run measures the headline only
    assert d["full_plan"] is None and d["cpu_baseline"] is None and d["parity"] is None and d["side"] == {}
    assert sorted(os.listdir(dump)) == ["valid.npy"]
    flags = np.load(dump / "valid.npy")
    assert flags.dtype == np.float32 and flags.shape == (N_STATES,)
    rg, ro = config.inflate_radii(cfg)
    gates, obstacles = synth.track_world(42)
    lo, hi = synth.C2_BOUNDS
    batch = (steps - 1) % 16
    pts = synth.sample_states(7, lo, hi, N_STATES, start=batch * N_STATES)
    ref = O.check_states(O.world_build(geom, gates, obstacles, rg, ro), rg, ro, pts, False, threads=16)
    assert np.array_equal(flags, ref.astype(np.float32))
    assert d["config"]["valid_fraction"] == pytest.approx(float(ref.mean()), abs=1e-12)
