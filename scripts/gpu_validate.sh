#!/bin/bash
# One GPU-box session: the GPU parity tests, smoke(), the full bench (one JSON line -> $OUT/bench_default.json).
# usage: OUT=<log dir> bash scripts/gpu_validate.sh   (on an MI355X box, ~15 min)
OUT=${OUT:-logs}   # log directory
mkdir -p $OUT
export TMPDIR=/tmp
echo "== pytest -m gpu"; timeout 700 python -m pytest tests -m gpu -x -q --timeout=180 > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -4 $OUT/pytest_gpu.log
echo "== smoke"; timeout 200 python __graft_entry__.py smoke > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/smoke.log
echo "== bench --full"; timeout 600 python bench.py --full > $OUT/bench_default.log 2>&1; echo "bench rc=$?"; tail -1 $OUT/bench_default.log > $OUT/bench_default.json; python - <<PY
import json
r = json.loads(open("$OUT/bench_default.json").read())
print("value", r["value"], "ms", r["ms_per_step"], "frac", r["roofline"]["frac"], "f32", r.get("f32_scan_engine", {}).get("frac"))
print("graph_path", json.dumps(r.get("graph_path"))[:900])
print("cpu", r.get("cpu_baseline", {}).get("value"))
PY
