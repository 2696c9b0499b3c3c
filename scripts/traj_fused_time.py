#!/usr/bin/env python3
"""Device time of a fused check of fitted tracks beside the composition it replaces, on 4096
fitted tracks of 12 segments (seeds 10_000 + k, v_max = 1.0, a_max = 2.0) sampled at dt = 0.01
against the 72-OBB world (synth.track_world(42), configs/config_filling.json).  --kind:

    point   epp_traj_check_batch (first failing row, min_distance 0.05) against
            epp_sample_count + epp_sample_batch (80 B per row to HBM) +
            epp_check_states_mindist on the contiguous n x 3 repack of columns 0 / 3 / 6
    chord   epp_traj_sweep_batch (first failing chord between consecutive rows through
            World::checkRayValid, can_pass_gate 0) against epp_sample_count + epp_sample_batch +
            epp_check_motions (mode 0) on the two contiguous n x 3 edge arrays of consecutive
            positions
    clearance  epp_traj_clearance_batch (closest approach of the rows to a collision OBB)
            against epp_sample_count + epp_sample_batch + epp_states_clearance on the n x 3
            repack; nothing exits early here, so "valid" (10 m above everything) and "mixed"
            do the same work.  --obbs 300 runs the 300-OBB world (synth.track_world(7, 8, 252)):
            more than one LDS tile of records

The fused call is one launch and writes no row; the repack of the composed one, a host step
today, is made once outside the timing.  Two cases: "valid" (every track lifted 10 m, above
every obstacle: no early exit, everything evaluated and checked) and "mixed" (the tracks as
fitted: valid and colliding ones).

hipEvent pairs on one stream around each call, --warmup untimed launches, then --reps timed
ones; median, min and max of each, the three composed calls timed one by one and summed (each
of the two sampling calls reads the track offsets back inside its pair, as it always does).

    python scripts/traj_fused_time.py --kind point [--reps 20] [--out profiles/traj_check_time.json]
    python scripts/traj_fused_time.py --kind chord [--reps 20] [--out profiles/traj_sweep_time.json]
    python scripts/traj_fused_time.py --kind clearance [--obbs 300] [--out profiles/traj_clearance_time.json]
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
    ap.add_argument("--kind", choices=("point", "chord", "clearance"), required=True)
    ap.add_argument("--obbs", type=int, choices=(72, 300), default=72)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tracks", type=int, default=4096)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--min-distance", type=float, default=0.05, help="point")
    ap.add_argument("--can-pass-gate", type=int, default=0, help="chord")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = capi.lib()
    clear = a.kind == "clearance"
    point = a.kind == "point" or clear  # (the items are the rows)
    nt, dt, md, cp = a.tracks, a.dt, a.min_distance, a.can_pass_gate
    cfg = config.load(os.path.join(ROOT, "configs", "config_filling.json"))
    rg, ro = config.inflate_radii(cfg)
    poses = synth.track_world(42) if a.obbs == 72 else synth.track_world(7, n_gates=8, n_obstacles=252)
    world = capi.World(capi.build_obbs(config.geometry(cfg), *poses), rg, ro)
    assert world.n == a.obbs
    world.build_index()
    stream = C.c_void_p()
    capi.check(L.epp_stream_create(C.byref(stream)))
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        capi.check(L.epp_event_create(C.byref(e)))
    off = np.arange(nt + 1, dtype=np.int32) * 13
    d_off = capi.DeviceBuffer.from_array(off, stream)
    d_T, d_C = capi.DeviceBuffer(8 * 12 * nt), capi.DeviceBuffer(240 * 12 * nt)
    d_st, d_cnt, d_roff = capi.DeviceBuffer(4 * nt), capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt)
    d_first, d_time = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(8 * nt)
    d_clr, d_near = capi.DeviceBuffer(8 * nt), capi.DeviceBuffer(4 * nt)  # (clearance)

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

    res = {"tracks": nt, "segments": 12, "dt": dt,
           **({} if clear else {"min_distance": md} if point else {"can_pass_gate": cp}),
           "obbs": world.n, "reps": a.reps, "warmup": a.warmup}
    for case, lift in (("valid", 10.0), ("mixed", 0.0)):
        tracks = [synth.random_track_waypoints(10_000 + k, 12) + [0.0, 0.0, lift] for k in range(nt)]
        d_wp = capi.DeviceBuffer.from_array(np.ascontiguousarray(np.concatenate(tracks)), stream)
        capi.check(L.epp_minsnap_batch(d_wp.ptr, d_off.ptr, nt, 1.0, 2.0, None, None, d_T.ptr, d_C.ptr, d_st.ptr,
                                       stream))
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

        def rows():
            capi.check(L.epp_sample_batch(d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, None, d_roff.ptr, d_rows.ptr, stream))

        rows()
        capi.check(L.epp_stream_sync(stream))
        xyz = d_rows.download(np.float64, n_rows * 10, stream).reshape(-1, 10)[:, [0, 3, 6]]
        # the repack (untimed), and where each track's items (rows | chords) start
        if point:
            n_items, ioff, per_track = n_rows, roff, cnt
            d_in = [capi.DeviceBuffer.from_array(np.ascontiguousarray(xyz), stream)]
        else:  # chord j of track k runs from row j to row j + 1 of that track
            start = np.ones(n_rows, bool)
            start[roff[1:][cnt > 0] - 1] = False  # a track's last row starts no chord
            si = np.flatnonzero(start)
            n_items, per_track = len(si), np.maximum(cnt - 1, 0)
            ioff = np.zeros(nt + 1, np.int64)
            ioff[1:] = np.cumsum(per_track)
            d_in = [capi.DeviceBuffer.from_array(np.ascontiguousarray(xyz[si + k]), stream) for k in (0, 1)]
        d_valid = capi.DeviceBuffer(n_items)
        d_dist, d_nr = capi.DeviceBuffer(8 * n_items if clear else 16), capi.DeviceBuffer(4 * n_items if clear else 16)

        def composed_check():
            if clear:
                capi.check(L.epp_states_clearance(world.handle, d_in[0].ptr, n_items, d_dist.ptr, d_nr.ptr, stream))
            elif point:
                capi.check(L.epp_check_states_mindist(world.handle, d_in[0].ptr, n_items, md, d_valid.ptr, stream))
            else:
                capi.check(L.epp_check_motions(world.handle, d_in[0].ptr, d_in[1].ptr, n_items, cp, 0, d_valid.ptr,
                                               stream))

        def fused():
            if clear:
                capi.check(L.epp_traj_clearance_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, d_clr.ptr,
                                                      d_first.ptr, d_time.ptr, d_near.ptr, stream))
            elif point:
                capi.check(L.epp_traj_check_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, md, d_first.ptr,
                                                  d_time.ptr, stream))
            else:
                capi.check(L.epp_traj_sweep_batch(world.handle, d_T.ptr, d_C.ptr, d_off.ptr, nt, dt, cp, d_first.ptr,
                                                  d_time.ptr, stream))

        check_key = "states_clearance" if clear else "check_states_mindist" if point else "check_motions"
        r = {"rows": n_rows} if point else {"rows": n_rows, "chords": n_items}
        print(f"{case}: {n_rows} rows, {n_items} items uploaded; timing", file=sys.stderr, flush=True)
        r["fused"] = timed(fused)
        r["sample_count"] = timed(count)
        r["sample_batch"] = timed(rows)
        r[check_key] = timed(composed_check)
        parts = ("sample_count", "sample_batch", check_key)
        r["composed"] = {k: float(sum(r[p][k] for p in parts)) for k in ("median_ms", "min_ms", "max_ms")}
        r["composed_over_fused"] = r["composed"]["median_ms"] / r["fused"]["median_ms"]
        # the same answers, or the times compare different work
        if clear:
            dist = d_dist.download(np.float64, n_items, stream)
            exp_clr = np.array([dist[roff[k]:roff[k + 1]].min() if cnt[k] else np.inf for k in range(nt)])
            got_clr = d_clr.download(np.float64, nt, stream)
            assert np.array_equal(got_clr, exp_clr), "fused and composed answers differ"
            r["clearance_min"], r["clearance_max"] = float(got_clr.min()), float(got_clr.max())
            r["tracks_touching"] = int((got_clr == 0).sum())
            res[case] = r
            for b in (d_rows, d_valid, d_wp, d_dist, d_nr, *d_in):
                b.free()
            continue
        first = d_first.download(np.int64, nt, stream)
        flags = d_valid.download(np.uint8, n_items, stream)
        exp = np.full(nt, -1, np.int64)
        bad = np.flatnonzero(flags == 0)
        tr = np.searchsorted(ioff, bad, side="right") - 1
        uniq, idx = np.unique(tr, return_index=True)
        exp[uniq] = bad[idx] - ioff[uniq]
        assert np.array_equal(first, exp), "fused and composed answers differ"
        r["tracks_valid"] = int((first < 0).sum())
        r["rows_before_first_collision" if point else "chords_before_first_collision"] = int(
            np.where(first < 0, per_track, first + 1).sum())
        res[case] = r
        for b in (d_rows, d_valid, d_wp, *d_in):
            b.free()
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
