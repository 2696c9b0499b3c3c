#!/usr/bin/env python3
"""Kernel time of the constrained batch fit with no pins beside the plain batch fit, on the
bench's C5 side-leg batch (4096 tracks x 12 segments, seeds 10_000 + k, v_max = 1.0, a_max = 2.0):

    epp_minsnap_batch               k_minsnap
    epp_minsnap_batch_constrained   k_minsnap_constrained, mask 0 inside, ends [0, 0, 0, 0]

The two compute the same fit (checked here: the same bytes).  A timed window is --launches
back-to-back calls on one stream between a hipEvent pair; the two calls alternate, --windows
windows a side after --warmup untimed windows of each.  Reports per launch the median, the
smallest and the largest window of each side, in microseconds.

    python scripts/minsnap_constrained_time.py [--out profiles/minsnap_constrained_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-path-planner_amd"))

from eppamd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.lib()
    nt, M, v_max, a_max = a.tracks, 12, 1.0, 2.0
    wp = np.ascontiguousarray(np.concatenate([synth.random_track_waypoints(10_000 + k, M) for k in range(nt)]))
    off = np.arange(nt + 1, dtype=np.int32) * (M + 1)
    stream = C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        capi.check(L.epp_event_create(C.byref(e)))
    d_wp, d_off = capi.DeviceBuffer.from_array(wp, stream), capi.DeviceBuffer.from_array(off, stream)
    d_mask = capi.DeviceBuffer.from_array(np.zeros(nt * (M + 1), np.uint8), stream)
    d_val = capi.DeviceBuffer.from_array(np.zeros(nt * (M + 1) * 12), stream)
    out = {n: (capi.DeviceBuffer(8 * M * nt), capi.DeviceBuffer(240 * M * nt), capi.DeviceBuffer(4 * nt))
           for n in ("plain", "constrained")}

    def plain():
        T, Cf, st = out["plain"]
        capi.check(L.epp_minsnap_batch(d_wp.ptr, d_off.ptr, nt, v_max, a_max, None, None, T.ptr, Cf.ptr, st.ptr, stream))

    def constrained():
        T, Cf, st = out["constrained"]
        capi.check(L.epp_minsnap_batch_constrained(d_wp.ptr, d_off.ptr, nt, v_max, a_max, None, d_mask.ptr, d_val.ptr,
                                                   T.ptr, Cf.ptr, st.ptr, stream))

    def window(fn):
        capi.check(L.epp_event_record(ev[0], stream))
        for _ in range(a.launches):
            fn()
        capi.check(L.epp_event_record(ev[1], stream))
        capi.check(L.epp_stream_sync(stream))
        x = C.c_float(0)
        capi.check(L.epp_event_elapsed_ms(ev[0], ev[1], C.byref(x)))
        return 1e3 * x.value / a.launches

    us = {"plain": [], "constrained": []}
    for r in range(a.warmup + a.windows):
        for name, fn in (("plain", plain), ("constrained", constrained)):
            t = window(fn)
            if r >= a.warmup:
                us[name].append(t)
    same = all(out["plain"][i].download(np.uint8, n, stream).tobytes() ==
               out["constrained"][i].download(np.uint8, n, stream).tobytes()
               for i, n in enumerate((8 * M * nt, 240 * M * nt, 4 * nt)))
    res = {"tracks": nt, "segments": M, "launches_per_window": a.launches, "windows": a.windows, "same_bytes": same}
    for name, v in us.items():
        v = np.array(v)
        res[name] = {"median_us": float(np.median(v)), "min_us": float(v.min()), "max_us": float(v.max())}
    res["constrained_over_plain"] = res["constrained"]["median_us"] / res["plain"]["median_us"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for e in ev:
        L.epp_event_destroy(e)
    capi.check(L.epp_stream_destroy(stream))


if __name__ == "__main__":
    main()
