#!/bin/bash
# Motion-kernel A/B on one box (diagnostics): the collision + planner parity tests, then
# scripts/motions_ab.py on the product library and on a second build given as $1 (a
# libepp.so built elsewhere, e.g. with scripts/ab_build.sh), three rounds in alternation;
# without $1 only the product is timed.  Then a short bench with its side legs.  Logs go
# to $EPP_EVIDENCE_DIR (default: evidence_out/).
set -u
OUT="${EPP_EVIDENCE_DIR:-evidence_out}"
OTHER="${1:-}"
mkdir -p "$OUT"
timeout -k 10 500 python -u -m pytest -x -q --timeout 200 --timeout-method thread -p no:cacheprovider tests/test_gpu_collision.py tests/test_gpu_planner.py > "$OUT/mt.log" 2>&1 || { tail -20 "$OUT/mt.log"; exit 1; }
tail -2 "$OUT/mt.log"
for r in 1 2 3; do
  timeout -k 10 120 python scripts/motions_ab.py || exit 1
  if [ -n "$OTHER" ]; then timeout -k 10 120 python scripts/motions_ab.py "$OTHER" || exit 1; fi
done
timeout -k 10 300 python bench.py --full --no-cpu --steps 20 --warmup 5 > "$OUT/b20.json"
