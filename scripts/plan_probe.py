"""Full-plan (C4) breakdown (diagnostics): one track through OnlineTrajGenerator.
pre_compute_traj as bench.py runs it, timed per call, with the planner's own split (device
pipeline vs host search, summed over the segments) and the planner call alone; under the
planner thread counts given as arguments (EPP_PLAN_THREADS, each in its own process)."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# EPP_PKG: another build of the package (scripts/ab_pkg.sh) for a same-box A/B
sys.path[:0] = [ROOT, os.environ.get("EPP_PKG") or os.path.join(ROOT, "efficient-path-planner_amd")]

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    import numpy as np
    import online_traj_planner as otp
    from eppamd import config, synth
    cfg = config.load(os.path.join(ROOT, "configs", "config.json"))
    cfg["world_properties"]["lower_bound"] = [-6, -6, 0]
    cfg["world_properties"]["upper_bound"] = [6, 6, 2]
    cfg["path_planner_properties"]["samples_fmt"] = 65536
    geom = config.geometry(cfg)
    fd, path = tempfile.mkstemp(suffix=".json")
    with os.fdopen(fd, "w") as f:
        json.dump(cfg, f)
    gates, obstacles = synth.track_world(100)
    cps = synth.gate_checkpoints(gates, geom.gate_height, 0.55)
    otg = otp.OnlineTrajGenerator(cps[0], cps[-1], gates, obstacles, path)
    for _ in range(int(os.environ.get("EPP_PROBE_WARM", "1"))):  # untimed calls first
        otg.pre_compute_traj(0.0)
    ts, st = [], []
    for _ in range(int(os.environ.get('EPP_PROBE_CALLS', '30'))):
        t = time.perf_counter()
        otg.pre_compute_traj(0.0)
        ts.append((time.perf_counter() - t) * 1e3)
        st.append(otg.planner_stats())
    os.unlink(path)
    print(f"{os.path.basename(os.environ.get('EPP_PKG', '') or 'cur')} threads {os.environ.get('EPP_PLAN_THREADS', '4')} writer {os.environ.get('EPP_PATH_WRITER', '1')}: pre_compute_traj p50 {np.median(ts):.4f} ms "
          f"(mean {np.mean(ts):.2f}, min {min(ts):.2f}); planner: ms {np.median([s['ms'] for s in st]):.4f}, device sum "
          f"{np.median([s['ms_device'] for s in st]):.2f}, search sum {np.median([s['ms_search'] for s in st]):.2f}, "
          f"rows down per track {np.median([s['rows_downloaded'] for s in st]):.0f} "
          f"(EPP_PLAN_ELLIPSE {os.environ.get('EPP_PLAN_ELLIPSE', 'default')})",
          flush=True)
    order = np.argsort(ts)[::-1][:6]
    print("   slowest:", ", ".join(f"#{i} {ts[i]:.2f} ms (planner {st[i]['ms']:.2f}, device {st[i]['ms_device']:.2f}, "
                                   f"search {st[i]['ms_search']:.2f}, attempts {st[i]['attempts']}, "
                                   f"fallbacks {st[i]['fallbacks']})"
                                   for i in order), flush=True)
    print("   fallbacks per call:", [s["fallbacks"] for s in st], "mean", np.mean([s["fallbacks"] for s in st]))
    print("   restricted searches per call p50: pops", np.median([s.get("astar_pops", 0) for s in st]), "nodes",
          np.median([s.get("restricted_nodes", 0) for s in st]), "slowest problem (ms)",
          np.median([s.get("ms_restricted_max", 0) for s in st]), "its copy (ms)",
          np.median([s.get("ms_copy_of_max", 0) for s in st]))
    print("   fallback reasons [capacity, inexact row, goal edge outside the rows, pop above bound, -, symmetrised: pop above bound,"
          " symmetrised: exhausted]:", np.sum([s.get("fallback_why", [0] * 7) for s in st], 0).tolist(),
          "; symmetrised searches decided on the rows:", sum(s.get("restricted_symmetrised", 0) for s in st))
    warm = int(os.environ.get("EPP_PROBE_WARM", "1"))
    print("   planner call numbers of the calls with symmetrised searches decided on the rows:",
          [9 * (warm + i) for i, s in enumerate(st) if s.get("restricted_symmetrised", 0)], flush=True)
    print(f"   planner phases p50 (ms): batch {np.median([s['ms_batch'] for s in st]):.3f} (enqueued by "
          f"{np.median([s.get('ms_enqueue', float('nan')) for s in st]):.3f}) solve "
          f"{np.median([s['ms_solve'] for s in st]):.3f} shortcut {np.median([s['ms_shortcut'] for s in st]):.3f}; "
          f"outside the planner {np.median([t - s['ms'] for t, s in zip(ts, st)]):.3f}", flush=True)
    if os.environ.get("EPP_PROBE_PERCALL"):
        for i, (t, s) in enumerate(zip(ts, st)):
            print(f"   #{i}: {t:.3f} ms, batch {s['ms_batch']:.3f} solve {s['ms_solve']:.3f} shortcut "
                  f"{s['ms_shortcut']:.3f} outside {t - s['ms']:.3f}; rows {s['rows_downloaded']} pops "
                  f"{s.get('astar_pops', 0)} slowest search {s.get('ms_restricted_max', 0):.3f}", flush=True)
    print("   all (ms):", " ".join(f"{t:.2f}/{s['ms']:.2f}" for t, s in zip(ts, st)), flush=True)
else:
    for t in (sys.argv[1:] or ["4"]):
        t, _, pw = t.partition(":")  # "4" or "4:0" (EPP_PATH_WRITER=0)
        env = dict(os.environ, EPP_PLAN_THREADS=t)
        if pw:
            env["EPP_PATH_WRITER"] = pw
        r = subprocess.run([sys.executable, __file__, "--child"], env=env, timeout=120)
        if r.returncode:
            sys.exit(r.returncode)
