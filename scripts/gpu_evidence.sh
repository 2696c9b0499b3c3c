#!/bin/bash
# Round-5 evidence session: every GPU test, smoke, the bench (driver shape and default),
# rocprofv3 kernel traces (headline alone, whole bench, the batched planner alone) and the
# PMC FETCH_SIZE / WRITE_SIZE passes of the headline (separate runs) -> $EPP_EVIDENCE_DIR
# (default: evidence_out/ in the repository root).
# Every GPU step has its own time limit; a fault/abort/timeout stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${EPP_EVIDENCE_DIR:-evidence_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
stop() { case "$1" in 0) return 0 ;; *) echo "step $2 ended with $1: stopping"; exit "$1" ;; esac; }
if [ -z "${SKIP_TESTS:-}" ]; then
  echo "== pytest -m gpu"
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider > "$OUT/pytest_gpu.log" 2>&1; rc=$?
  tail -4 "$OUT/pytest_gpu.log"; stop $rc pytest
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1; rc=$?
  tail -1 "$OUT/smoke.log"; stop $rc smoke
fi
echo "== bench (driver shape: 20 steps; every leg)"
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > "$OUT/bench20.json" 2> "$OUT/bench20.err"; rc=$?
stop $rc bench20
echo "== bench (default steps; every leg)"
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; rc=$?
stop $rc bench
if [ -z "${SKIP_PROF:-}" ]; then
  echo "== rocprofv3: headline, whole bench, planner"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 bench.py > "$OUT/prof_bench.json" 2> "$OUT/prof.err"; rc=$?
  stop $rc rocprof
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_full" -o run -- python3 bench.py --full --no-cpu > "$OUT/prof_full_bench.json" 2> "$OUT/prof_full.err"; rc=$?
  stop $rc rocprof_full
  EPP_PROBE_CALLS=30 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_plan" -o run -- python3 scripts/plan_probe.py --child > "$OUT/prof_plan.log" 2>&1; rc=$?
  stop $rc rocprof_plan
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout -s KILL 120 rocprofv3 --pmc $c --output-format csv -d "$OUT/pmc_$c" -o run -- python3 bench.py --steps 200 --warmup 20 > "$OUT/pmc_$c.json" 2> "$OUT/pmc_$c.err"; rc=$?
    stop $rc pmc_$c
  done
fi
echo done
