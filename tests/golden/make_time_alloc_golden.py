"""Writes tests/golden/time_alloc_costs.json: a few tracks (segment times and the truth
solve's coefficients as hexadecimal doubles) with their truth snap cost and its rounding scale
from tests/time_alloc_ref.py.  Run from the repository root: python tests/golden/make_time_alloc_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import numpy as np  # noqa: E402

import time_alloc_inputs as ti  # noqa: E402
import time_alloc_ref as tr  # noqa: E402


def records():
    out = []
    t = ti.tracks()
    for name in ("m1", "m3", "va", "clamp", "m12"):
        k = t[name]
        C = tr.solve(k.wp, k.T, k.v0, k.a0)[0]
        out.append({"name": name, "T": [float(x).hex() for x in k.T], "C": [float(x).hex() for x in C.ravel()],
                    "cost": float(tr.cost(k.T, C)).hex(), "scale": float(tr.cost_abs(k.T, C)).hex()})
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "time_alloc_costs.json"), "w") as f:
        json.dump(records(), f, indent=0)
        f.write("\n")
