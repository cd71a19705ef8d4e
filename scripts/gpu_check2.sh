#!/bin/bash
# GPU-box helper: -m gpu tests, then a short bench with the set_reads timing breakdown and the default bench with every leg (--full); results
# under $OUT.
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -x -q --capture=sys > $OUT/gpu_tests.log 2>&1
rc=$?
tail -25 $OUT/gpu_tests.log
[ $rc -ne 0 ] && exit $rc
UVCGPU_TIMING=1 timeout -k 10 600 python bench.py --steps 4 --warmup 1 --tiles 2 --serial > $OUT/bench_timing.json 2> $OUT/bench_timing.err || { tail -30 $OUT/bench_timing.err; exit 3; }
tail -40 $OUT/bench_timing.err
timeout -k 10 900 python bench.py --full $BENCH_ARGS > $OUT/bench_latest.json 2> $OUT/bench_latest.err || { tail -20 $OUT/bench_latest.err; exit 3; }
python - $OUT/bench_latest.json <<'PY'
import json, sys
j = json.load(open(sys.argv[1]))
print("value %.3e pos/s  ms/step %.2f  roofline %s frac %.4f" % (j["value"], j["ms_per_step"], j["roofline"]["kernel"], j["roofline"]["frac"]))
print(j["kernel_ms"])
print(j.get("cpu_baseline"))
print("pcie_inclusive:", j.get("pcie_inclusive")); print("resident:", j.get("resident"))
PY
