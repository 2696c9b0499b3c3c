#!/usr/bin/env python3
"""Kernel time of the segment-time allocation beside the fit it repeats, on the bench's C5
side-leg batch (4096 tracks x 12 segments, seeds 10_000 + k, fitted at v_max = 1.0, a_max = 2.0):

    epp_minsnap_batch_times      the fit at the caller's times: one solve per track
    epp_traj_snap_cost           the cost of the fitted batch
    epp_minsnap_time_gradient    13 solves per track, one workgroup each, and the quotients
    epp_minsnap_optimize_times   the whole descent per track (default parameters)

hipEvent pairs on one stream around each call, a few warm-up calls, the median of --reps
repeats.  The descent works in place, so every repeat restores the start times first (outside
the event pair).  Reports the time per solve of the gradient and of the descent against the
fit's (the descent's solves are counted on the host from its iteration counts: a lower bound,
rejected trial steps are not reported by the call).

    python scripts/timealloc_time.py [--reps 20] [--out profiles/timealloc_time.json]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.lib()
    nt, M, v_max, a_max = a.tracks, 12, 1.0, 2.0
    tracks = [synth.random_track_waypoints(10_000 + k, M) for k in range(nt)]
    wp = np.ascontiguousarray(np.concatenate(tracks))
    off = np.arange(nt + 1, dtype=np.int32) * (M + 1)
    stream = C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        capi.check(L.epp_event_create(C.byref(e)))
    d_wp, d_off = capi.DeviceBuffer.from_array(wp, stream), capi.DeviceBuffer.from_array(off, stream)
    d_T0, d_T, d_C = capi.DeviceBuffer(8 * M * nt), capi.DeviceBuffer(8 * M * nt), capi.DeviceBuffer(240 * M * nt)
    d_st, d_it = capi.DeviceBuffer(4 * nt), capi.DeviceBuffer(4 * nt)
    d_J, d_J1, d_g = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * M * nt)
    capi.check(L.epp_minsnap_batch(d_wp.ptr, d_off.ptr, nt, v_max, a_max, None, None, d_T0.ptr, d_C.ptr, d_st.ptr,
                                   stream))
    prm = capi.TimeoptParams()

    T0 = d_T0.download(np.float64, M * nt, stream)

    def restore():
        d_T.upload(T0, stream)

    def fit():
        capi.check(L.epp_minsnap_batch_times(d_wp.ptr, d_off.ptr, nt, None, None, d_T.ptr, d_C.ptr, d_st.ptr, stream))

    def cost():
        capi.check(L.epp_traj_snap_cost(d_T.ptr, d_C.ptr, d_off.ptr, nt, d_J.ptr, d_st.ptr, stream))

    def grad():
        capi.check(L.epp_minsnap_time_gradient(d_wp.ptr, d_off.ptr, nt, None, None, d_T.ptr, prm.h, prm.t_min, d_J.ptr,
                                               d_g.ptr, d_st.ptr, stream))

    def opt():
        capi.check(L.epp_minsnap_optimize_times(d_wp.ptr, d_off.ptr, nt, None, None, d_T.ptr, d_C.ptr, prm, d_J.ptr,
                                                d_J1.ptr, d_it.ptr, d_st.ptr, stream))

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

    res = {"tracks": nt, "segments": M, "v_max": v_max, "a_max": a_max, "reps": a.reps, "warmup": a.warmup,
           "params": [prm.h, prm.t_min, prm.step0, prm.max_halvings, prm.ftol, prm.max_iter]}
    restore()
    res["minsnap_batch_times"] = timed(fit)
    res["traj_snap_cost"] = timed(cost)
    res["time_gradient"] = timed(grad)
    res["optimize_times"] = timed(opt, before=restore)
    capi.check(L.epp_stream_sync(stream))
    it = d_it.download(np.int32, nt, stream)
    st = d_st.download(np.int32, nt, stream)
    J0, J1 = d_J.download(np.float64, nt, stream), d_J1.download(np.float64, nt, stream)
    res["iters_median"] = float(np.median(it))
    res["iters_max"] = int(it.max())
    res["status_counts"] = {str(k): int((st == k).sum()) for k in np.unique(st)}
    res["cost_ratio_median"] = float(np.median(J1 / J0))
    per_fit = res["minsnap_batch_times"]["median_ms"] / nt
    res["gradient_per_solve_over_fit"] = res["time_gradient"]["median_ms"] / (nt * (M + 1)) / per_fit
    # at least: the first fit, (M + 1) solves per gradient (one more gradient than accepted steps
    # unless the last step stopped the loop), one trial per accepted step, the last fit
    solves = float(np.sum(2 + (it + 1) * M + it))
    res["descent_solves_at_least"] = solves
    res["descent_per_solve_over_fit_at_most"] = res["optimize_times"]["median_ms"] / solves / per_fit
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
