#!/bin/bash
# GPU-box helper: smoke, a small and the default bench with every leg (--full); results under $OUT.
cd "${GRAFT_REPO_ROOT:-.}"
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -20 $OUT/smoke.log; exit 1; }
tail -2 $OUT/smoke.log
timeout -k 10 400 python bench.py --full --tile-kb 100 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_100kb.json 2> $OUT/bench_100kb.err || { tail -20 $OUT/bench_100kb.err; exit 2; }
cat $OUT/bench_100kb.json
timeout -k 10 900 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || { tail -20 $OUT/bench_default.err; exit 3; }
cat $OUT/bench_default.json
