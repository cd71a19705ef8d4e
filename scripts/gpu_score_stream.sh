#!/bin/bash
# GPU-box helper: the measurements of DESIGN.md 4h.  One line per run under $OUT (default bench_out).
#   scripts/gpu_score_stream.sh [PARENT_LIB]
# PARENT_LIB = libuvcgpu.so of the parent commit (another build of the same ABI): bench.py and the 200 kb -A tile then alternate between
# the two builds.  Every step under its own time limit; the first step that fails ends the script.
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}; mkdir -p $OUT
PARENT=$1
export TMPDIR=/tmp
LOG=$OUT/score_stream_bench_ab.txt
: > $LOG
bench() {   # label [library]
    if [ -n "$2" ]; then export UVCGPU_LIBRARY=$PWD/$2; else unset UVCGPU_LIBRARY; fi
    timeout -k 10 300 python3 bench.py --gpus 1 --steps 16 --warmup 4 > $OUT/score_stream_bench.json 2> $OUT/score_stream_bench.err || { tail -20 $OUT/score_stream_bench.err; return 1; }
    unset UVCGPU_LIBRARY
    python3 -c "import json,sys; j=json.loads(open('$OUT/score_stream_bench.json').read().strip().splitlines()[-1]); print('$1 ms_per_step %.4f value %.4e' % (j['ms_per_step'], j['value']))" | tee -a $LOG
}
if [ -n "$PARENT" ]; then
    for order in "parent this" "this parent" "parent this"; do
        for who in $order; do
            if [ $who = parent ]; then bench parent $PARENT || exit 1; else bench this || exit 1; fi
        done
    done
else
    for rep in 1 2 3; do bench this || exit 1; done
fi
timeout -k 10 420 python3 scripts/gpu_score_stream.py --kb 200 --chunks 8 --reps 7 ${PARENT:+--parent-lib $PARENT} > $OUT/score_stream_200kb.txt 2>&1 || { tail -20 $OUT/score_stream_200kb.txt; exit 1; }
tail -5 $OUT/score_stream_200kb.txt
timeout -k 10 560 python3 scripts/gpu_score_stream.py --kb 1000 --mem-mb 2048 --reps 3 --no-one-call > $OUT/score_stream_1mb.txt 2>&1 || { tail -20 $OUT/score_stream_1mb.txt; exit 1; }
tail -5 $OUT/score_stream_1mb.txt
