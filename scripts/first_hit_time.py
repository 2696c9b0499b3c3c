"""Timing of epp_motions_first_hit (k_motions_first_hit, brute force over every OBB) next to
epp_check_motions mode 0 (k_motions_v5, tile-filtered) from the same build, on bench.py's C2
world (64 OBBs) and C3 world (512 OBBs) with the C3 leg's 1,048,576 edges:
python scripts/first_hit_time.py [ROUNDS] [REPLAYS].  Each call is captured into a graph of
its own; a round is HIP events around REPLAYS replays; prints one JSON line with every round's
per-launch time and the medians (diagnostics only: DESIGN.md section 4 quotes them)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-path-planner_amd")]
from eppamd import capi, config, synth  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPLAYS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
N = 1 << 20
L = capi.lib()
cfg = config.load(os.path.join(ROOT, "configs", "config.json"))
geom = config.geometry(cfg)
rg, ro = config.inflate_radii(cfg)
lo, hi = synth.C2_BOUNDS
s1, s2 = synth.edges(43, 8, lo, hi, N)
d1, d2 = capi.DeviceBuffer.from_array(s1), capi.DeviceBuffer.from_array(s2)
d_valid, d_t, d_obb = capi.DeviceBuffer(N), capi.DeviceBuffer(8 * N), capi.DeviceBuffer(4 * N)
st = C.c_void_p()
capi.check(L.epp_stream_create(C.byref(st)))
st = st.value


def replay_us(call):
    g = C.c_void_p()
    capi.check(L.epp_graph_begin(st))
    call()
    capi.check(L.epp_graph_end(st, C.byref(g)))
    for _ in range(5):  # warm-up
        capi.check(L.epp_graph_launch(g.value, st))
    capi.check(L.epp_stream_sync(st))
    out = []
    for _ in range(ROUNDS):
        e0, e1 = C.c_void_p(), C.c_void_p()
        capi.check(L.epp_event_create(C.byref(e0)))
        capi.check(L.epp_event_create(C.byref(e1)))
        capi.check(L.epp_event_record(e0, st))
        for _ in range(REPLAYS):
            capi.check(L.epp_graph_launch(g.value, st))
        capi.check(L.epp_event_record(e1, st))
        capi.check(L.epp_stream_sync(st))
        ms = C.c_float()
        capi.check(L.epp_event_elapsed_ms(e0, e1, C.byref(ms)))
        L.epp_event_destroy(e0)
        L.epp_event_destroy(e1)
        out.append(round(ms.value / REPLAYS * 1e3, 2))
    capi.check(L.epp_graph_destroy(g.value))
    return out


res = {"edges": N, "rounds": ROUNDS, "replays": REPLAYS}
for name, poses in (("c2_64", synth.track_world(42)), ("c3_512", synth.track_world(42, n_obstacles=472))):
    w = capi.World(capi.build_obbs(geom, *poses), rg, ro)
    w.build_index()
    motions = replay_us(lambda: w.check_motions_dev(d1.ptr, d2.ptr, N, 0, 0, d_valid.ptr, stream=st))
    first = replay_us(lambda: capi.check(L.epp_motions_first_hit(w.handle, d1.ptr, d2.ptr, N, 0, d_t.ptr, d_obb.ptr, st)))
    capi.check(L.epp_stream_sync(st))
    flags, obb = d_valid.download(np.uint8, N), d_obb.download(np.int32, N)
    assert np.array_equal(obb >= 0, flags == 0)
    res[name] = {"obbs": w.n, "blocked": int((obb >= 0).sum()), "k_motions_v5_us": motions,
                 "k_motions_first_hit_us": first, "k_motions_v5_median_us": float(np.median(motions)),
                 "k_motions_first_hit_median_us": float(np.median(first))}
print(json.dumps(res), flush=True)
