"""Same-box comparison of two builds of the planner (diagnostics): for the bench's C4 tracks
(world seeds 100..107, bench.py's configuration), under EPP_PLAN_ELLIPSE default / 1.0 / 0,
prints a hash of the planned paths' bytes (every gate-to-gate segment through plan_paths, two
calls, then the goals outside the sampling box that the symmetrised search decides, through
plan_once) and every integer field of PlannerStats.  Run it once per build (EPP_PKG=ab/pkg_X,
scripts/ab_pkg.sh) and diff the outputs: they must be identical."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.environ.get("EPP_PKG") or os.path.join(ROOT, "efficient-path-planner_amd")]

INT_FIELDS = ("attempts", "states_sampled", "states_valid", "edges_checked", "edges_valid", "rows_downloaded",
              "restricted_rows", "fallbacks", "fallback_why", "astar_pops", "restricted_nodes",
              "restricted_symmetrised", "symmetrised_after_census")
OUTSIDE = [((0, 5.0, 1.0), (0, 6.4, 1.0)), ((5.0, 0, 1.0), (6.4, 0.5, 1.0)), ((0, -5, 1.0), (0.5, -6.5, 1.0)),
           ((2, 2, 1.2), (2.5, 2.5, 2.5)), ((-5, -5, 1.0), (-6.4, -6.4, 1.0))]

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
    tag = "ellipse " + (os.environ.get("EPP_PLAN_ELLIPSE") or "default")

    def report(what, h, st):
        print(tag, what, h.hexdigest()[:16], json.dumps({k: st[k] for k in INT_FIELDS if k in st}), flush=True)

    for world in range(100, 108):
        gates, obstacles = synth.track_world(world)
        cps = synth.gate_checkpoints(gates, geom.gate_height, 0.55)
        pp = otp.PathPlanner(gates, obstacles, path)
        problems = [(cps[s], cps[s + 1]) for s in range(0, len(cps) - 1, 2)]
        for call in range(2):
            h = hashlib.sha256()
            for ok, p in pp.plan_paths(problems, 2.0):
                h.update(b"1" if ok else b"0")
                h.update(np.ascontiguousarray(p, dtype=np.float64).tobytes() if ok else b"")
            report(f"world {world} call {call}", h, pp.last_stats())
    gates, obstacles = synth.track_world(100)
    pp = otp.PathPlanner(gates, obstacles, path)
    h = hashlib.sha256()
    for s, g in OUTSIDE:
        for seed in (0, 1):
            got = pp.plan_once(np.array(s, float), np.array(g, float), 65536, seed)
            h.update(b"-" if got is None else np.ascontiguousarray(got, dtype=np.float64).tobytes())
    report("world 100 goals outside the box", h, pp.last_stats())
    os.unlink(path)
else:
    for ellipse in ("", "1.0", "0"):
        env = dict(os.environ)
        env.pop("EPP_PLAN_ELLIPSE", None)
        if ellipse:
            env["EPP_PLAN_ELLIPSE"] = ellipse
        r = subprocess.run([sys.executable, __file__, "--child"], env=env, timeout=300)
        if r.returncode:
            sys.exit(r.returncode)
