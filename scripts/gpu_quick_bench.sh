#!/bin/bash
# GPU-box helper: the full bench without the CPU baseline and the side legs, key numbers on stdout.  Arguments go to bench.py; results under $OUT.
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python bench.py --full --no-cpu-baseline --no-side "$@" > $OUT/bench_quick.json 2> $OUT/bench_quick.err || { tail -20 $OUT/bench_quick.err; exit 3; }
python3 - $OUT/bench_quick.json <<'PY'
import json, sys
j = json.load(open(sys.argv[1]))
print("value %.4e pos/s  ms/step %.3f  in_flight4 %s  pcie %s  resident %s" % (j["value"], j["ms_per_step"], j.get("resident_in_flight4", {}).get("ms_per_step"), j.get("pcie_inclusive", {}).get("ms_per_step"), j.get("resident", {}).get("ms_per_step")))
print("in-stream kernel_ms:", j["kernel_ms"])
print("resident kernel_ms:", j.get("resident", {}).get("kernel_ms"))
PY
