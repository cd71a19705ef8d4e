#!/bin/bash
# GPU-box helper: full -m gpu test suite, then the default bench with every leg (--full; BENCH_ARGS=--no-cpu-baseline leaves the CPU baseline
# out); results under $OUT.
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/gpu_tests.log 2>&1
rc=$?
tail -15 $OUT/gpu_tests.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 900 python bench.py --full $BENCH_ARGS > $OUT/bench_latest.json 2> $OUT/bench_latest.err || { tail -20 $OUT/bench_latest.err; exit 3; }
python - $OUT/bench_latest.json <<'PY'
import json, sys
j = json.load(open(sys.argv[1]))
print("value %.3e pos/s  ms/step %.2f  roofline %s frac %.4f" % (j["value"], j["ms_per_step"], j["roofline"]["kernel"], j["roofline"]["frac"]))
print(j["kernel_ms"])
print(j.get("cpu_baseline"))
print("pcie_inclusive:", j.get("pcie_inclusive")); print("resident:", j.get("resident"))
PY
