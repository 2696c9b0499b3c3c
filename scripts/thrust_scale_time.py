#!/usr/bin/env python3
"""Device time of epp_traj_scale_to_thrust_limits (k_traj_thrust_scale: the whole search and the
apply in one launch) beside one epp_traj_thrust_grid_batch call, beside the host-driven
composition of the same search (one grid call and one readback per step, at most 1 + 10 + 12
steps; wall time), and beside epp_traj_scale_to_limits (k_traj_scale) on the same batch: the
bench's C5 batch, 4096 fitted tracks of 12 segments (seeds 10_000 + k, v_max = 1.0, a_max = 2.0).

The limits: f_max is the median over the tracks of the greatest thrust on the grid at scale 1,
the other limits off, so about half the tracks need scaling.  The scaling calls work in place:
every repetition restores the segment times and coefficients first, outside the timed span.

hipEvent pairs on one stream around each call, --warmup untimed launches, then --reps timed
ones; the composition is wall time (time.perf_counter) around its loop, readbacks included.

    python scripts/thrust_scale_time.py [--reps 20] [--out profiles/traj_thrust_scale_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-path-planner_amd"))

from eppamd import capi, synth  # noqa: E402

MAX_DOUBLINGS, BISECT_ROUNDS = 10, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--g", type=float, default=9.81)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.lib()
    nt, g = a.tracks, a.g
    stream = C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        capi.check(L.epp_event_create(C.byref(e)))

    off = np.arange(nt + 1, dtype=np.int32) * 13
    d_off = capi.DeviceBuffer.from_array(off, stream)
    d_T, d_C = capi.DeviceBuffer(8 * 12 * nt), capi.DeviceBuffer(240 * 12 * nt)
    d_st, d_vi, d_sc = capi.DeviceBuffer(4 * nt), capi.DeviceBuffer(4 * nt), capi.DeviceBuffer(8 * nt)
    d_s, d_out = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(64 * nt)
    tracks = [synth.random_track_waypoints(10_000 + k, 12) for k in range(nt)]
    d_wp = capi.DeviceBuffer.from_array(np.ascontiguousarray(np.concatenate(tracks)), stream)
    capi.check(L.epp_minsnap_batch(d_wp.ptr, d_off.ptr, nt, 1.0, 2.0, None, None, d_T.ptr, d_C.ptr, d_st.ptr, stream))
    capi.check(L.epp_stream_sync(stream))
    assert (d_st.download(np.int32, nt, stream) == 0).all()
    T0, C0 = d_T.download(np.float64, 12 * nt, stream), d_C.download(np.float64, 360 * nt, stream)

    def restore():
        d_T.upload(T0, stream)
        d_C.upload(C0, stream)

    def timed(fn, before=None):
        ms = []
        for r in range(a.warmup + a.reps):
            if before:
                before()
            capi.check(L.epp_event_record(ev[0], stream))
            fn()
            capi.check(L.epp_event_record(ev[1], stream))
            capi.check(L.epp_stream_sync(stream))
            x = C.c_float(0)
            capi.check(L.epp_event_elapsed_ms(ev[0], ev[1], C.byref(x)))
            if r >= a.warmup:
                ms.append(x.value)
        ms = np.array(ms)
        return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}

    def grid(scales=None):
        capi.check(L.epp_traj_thrust_grid_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, d_s.ptr if scales else None, g,
                                                d_out.ptr, stream))

    grid()
    capi.check(L.epp_stream_sync(stream))
    f_max = float(np.median(d_out.download(np.float64, 8 * nt, stream).reshape(nt, 8)[:, 2]))
    lim = (g, 0.0, f_max, float("inf"), -1.0)

    def fused():
        capi.check(L.epp_traj_scale_to_thrust_limits(d_T.ptr, d_C.ptr, d_off.ptr, nt, *lim, d_sc.ptr, d_st.ptr,
                                                     d_vi.ptr, stream))

    def sibling():
        capi.check(L.epp_traj_scale_to_limits(d_T.ptr, d_C.ptr, d_off.ptr, nt, 0.8, 1.6, d_sc.ptr, d_st.ptr, stream))

    def composition():
        """The search of csrc/thrust_scale.h for every track in step, the feasibility of each
        step from one grid call and its readback.  Returns (scale, steps)."""
        phase = np.zeros(nt, np.int8)  # 0: at 1; 1: doubling; 2: bisecting; 3: done
        s = np.ones(nt)
        hi, lo = np.full(nt, 2.0), np.ones(nt)
        d, rounds = np.ones(nt, np.int32), np.zeros(nt, np.int32)
        scale = np.ones(nt)
        steps = 0
        while (phase < 3).any():
            d_s.upload(s, stream)
            grid(True)
            capi.check(L.epp_stream_sync(stream))
            bad = d_out.download(np.float64, 8 * nt, stream).reshape(nt, 8)[:, 2] > f_max
            steps += 1
            p0, p1, p2 = phase == 0, phase == 1, phase == 2
            phase[p0 & ~bad] = 3
            phase[p0 & bad] = 1
            give_up = p1 & bad & (d == MAX_DOUBLINGS)
            phase[give_up] = 3
            more = p1 & bad & ~give_up
            hi[more] *= 2.0
            d[more] += 1
            start = p1 & ~bad
            lo[start] = hi[start] * 0.5
            phase[start] = 2
            hi[p2 & ~bad] = s[p2 & ~bad]
            lo[p2 & bad] = s[p2 & bad]
            rounds[p2] += 1
            done = p2 & (rounds == BISECT_ROUNDS)
            scale[done] = hi[done]
            phase[done] = 3
            s = np.where(phase == 1, hi, np.where(phase == 2, 0.5 * (lo + hi), 1.0))
        return scale, steps

    r = {"tracks": nt, "segments": 12, "g": g, "f_max": f_max, "reps": a.reps, "warmup": a.warmup}
    print("timing", file=sys.stderr, flush=True)
    r["scale_to_thrust_limits"] = timed(fused, restore)
    scale = d_sc.download(np.float64, nt, stream)
    status = d_st.download(np.int32, nt, stream)
    r["scaled_fraction"] = float((scale > 1.0).mean())
    r["scale_max"] = float(scale.max())
    assert (status == 0).all()
    restore()
    r["thrust_grid"] = timed(grid)
    wall = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        comp_scale, steps = composition()
        if rep >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    wall = np.array(wall)
    r["composition_wall"] = {"median_ms": float(np.median(wall)), "min_ms": float(wall.min()),
                             "max_ms": float(wall.max()), "steps": steps}
    assert comp_scale.tobytes() == scale.tobytes()  # the same answers
    r["scale_to_limits"] = timed(sibling, restore)
    r["sibling_scaled_fraction"] = float((d_sc.download(np.float64, nt, stream) > 1.0).mean())
    r["composition_over_fused"] = r["composition_wall"]["median_ms"] / r["scale_to_thrust_limits"]["median_ms"]
    r["fused_over_grid"] = r["scale_to_thrust_limits"]["median_ms"] / r["thrust_grid"]["median_ms"]
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    for e in ev:
        L.epp_event_destroy(e)
    capi.check(L.epp_stream_destroy(stream))


if __name__ == "__main__":
    main()
