#!/usr/bin/env python3
"""Device time of epp_traj_thrust_rates_batch (k_traj_thrust_rates) beside the composition it
replaces and beside epp_traj_clearance_batch (k_traj_clearance, a small world) on the same
tracks: the bench's C5 batch, 4096 fitted tracks of 12 segments (seeds 10_000 + k, v_max = 1.0,
a_max = 2.0) sampled at dt = 0.01; the clearance against the 72-OBB world (synth.track_world(42),
configs/config_filling.json).

The composition: epp_sample_count + epp_sample_batch (the time column; 80 B per row to HBM) +
epp_sample_derivative_batch at orders 2 and 3 (24 B per row each) + epp_thrust_rates on those
values (48 B read, 24 B written per row); its per-track reductions, host steps, are not timed.

hipEvent pairs on one stream around each call, --warmup untimed launches, then --reps timed
ones.  For kernel times run it under a kernel trace (rocprofv3 --kernel-trace --stats).

    python scripts/thrust_rates_time.py [--reps 20] [--out profiles/traj_thrust_rates_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-path-planner_amd"))

from eppamd import capi, config, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--g", type=float, default=9.81)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.lib()
    nt, dt, g = a.tracks, a.dt, a.g
    cfg = config.load(os.path.join(ROOT, "configs", "config_filling.json"))
    rg, ro = config.inflate_radii(cfg)
    world = capi.World(capi.build_obbs(config.geometry(cfg), *synth.track_world(42)), rg, ro)
    world.build_index()
    stream = C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        capi.check(L.epp_event_create(C.byref(e)))

    def timed(fn):
        ms = []
        for r in range(a.warmup + a.reps):
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

    off = np.arange(nt + 1, dtype=np.int32) * 13
    d_off = capi.DeviceBuffer.from_array(off, stream)
    d_T, d_C = capi.DeviceBuffer(8 * 12 * nt), capi.DeviceBuffer(240 * 12 * nt)
    d_st, d_cnt, d_roff = capi.DeviceBuffer(4 * nt), capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt)
    d_out, d_idx = capi.DeviceBuffer(64 * nt), capi.DeviceBuffer(32 * nt)
    d_clr, d_crow, d_ctime, d_near = (capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt),
                                      capi.DeviceBuffer(4 * nt))
    tracks = [synth.random_track_waypoints(10_000 + k, 12) for k in range(nt)]
    d_wp = capi.DeviceBuffer.from_array(np.ascontiguousarray(np.concatenate(tracks)), stream)
    capi.check(L.epp_minsnap_batch(d_wp.ptr, d_off.ptr, nt, 1.0, 2.0, None, None, d_T.ptr, d_C.ptr, d_st.ptr, stream))
    capi.check(L.epp_stream_sync(stream))
    assert (d_st.download(np.int32, nt, stream) == 0).all()

    def count():
        capi.check(L.epp_sample_count(d_T.ptr, d_off.ptr, nt, dt, d_cnt.ptr, stream))

    count()
    capi.check(L.epp_stream_sync(stream))
    cnt = d_cnt.download(np.int64, nt, stream)
    roff = np.zeros(nt + 1, np.int64)
    roff[1:] = np.cumsum(cnt)
    n_rows = int(roff[-1])
    d_roff.upload(roff[:-1].copy(), stream)
    d_rows = capi.DeviceBuffer(80 * n_rows)
    d_acc, d_jerk = capi.DeviceBuffer(24 * n_rows), capi.DeviceBuffer(24 * n_rows)
    d_f, d_w, d_c = capi.DeviceBuffer(8 * n_rows), capi.DeviceBuffer(8 * n_rows), capi.DeviceBuffer(8 * n_rows)

    def rows():
        capi.check(L.epp_sample_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, None, d_roff.ptr, d_rows.ptr, stream))

    def deriv(order, buf):
        return lambda: capi.check(L.epp_sample_derivative_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, order, d_roff.ptr,
                                                                buf.ptr, stream))

    def per_sample():
        capi.check(L.epp_thrust_rates(d_acc.ptr, d_jerk.ptr, n_rows, g, d_f.ptr, d_w.ptr, d_c.ptr, stream))

    def fused():
        capi.check(L.epp_traj_thrust_rates_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, g, d_out.ptr, d_idx.ptr, stream))

    def clearance():
        capi.check(L.epp_traj_clearance_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, d_clr.ptr, d_crow.ptr,
                                              d_ctime.ptr, d_near.ptr, stream))

    r = {"tracks": nt, "segments": 12, "dt": dt, "g": g, "obbs": world.n, "rows": n_rows, "reps": a.reps,
         "warmup": a.warmup}
    print(f"{n_rows} rows; timing", file=sys.stderr, flush=True)
    r["traj_thrust_rates"] = timed(fused)
    r["traj_clearance"] = timed(clearance)
    r["sample_count"] = timed(count)
    r["sample_batch"] = timed(rows)
    r["sample_derivative_2"] = timed(deriv(2, d_acc))
    r["sample_derivative_3"] = timed(deriv(3, d_jerk))
    r["thrust_rates"] = timed(per_sample)
    parts = ("sample_count", "sample_batch", "sample_derivative_2", "sample_derivative_3", "thrust_rates")
    r["composed"] = {k: float(sum(r[q][k] for q in parts)) for k in ("median_ms", "min_ms", "max_ms")}
    r["fused_over_clearance"] = r["traj_thrust_rates"]["median_ms"] / r["traj_clearance"]["median_ms"]
    r["composed_over_fused"] = r["composed"]["median_ms"] / r["traj_thrust_rates"]["median_ms"]
    # the same answers: the fused extremes are the composition's on every 64th track
    out = d_out.download(np.float64, 8 * nt, stream).reshape(nt, 8)
    idx = d_idx.download(np.int64, 4 * nt, stream).reshape(nt, 4)
    f = d_f.download(np.float64, n_rows, stream)
    w = d_w.download(np.float64, n_rows, stream)
    c = d_c.download(np.float64, n_rows, stream)
    for k in range(0, nt, 64):
        s = slice(roff[k], roff[k + 1])
        want = [int(np.argmin(f[s])), int(np.argmax(f[s])), int(np.argmax(w[s])), int(np.argmin(c[s]))]
        assert idx[k].tolist() == want, (k, idx[k], want)
        assert out[k, 0::2].tolist() == [f[s][want[0]], f[s][want[1]], w[s][want[2]], c[s][want[3]]]
    r["f_min"] = [float(out[:, 0].min()), float(out[:, 0].max())]
    r["rate_max"] = [float(out[:, 4].min()), float(out[:, 4].max())]
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
