#!/bin/bash
# GPU-box helper: uvc1-mi355x -R panel.bed with and without --merge-regions on a panel made by scripts/make_panel.py.
#   scripts/gpu_merge_regions.sh PANEL_DIR [N ...]        (default N: 300 2000 20000)
# PARENT_EXE=path/to/another/uvc1-mi355x adds that build's plain -R run, alternated with this build's.  One line per run under $OUT:
# wall time of the whole command, then the program's own rate and per-stage thread-seconds (--timing -t 1).
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}; mkdir -p $OUT
D=$1; shift
NS=${@:-300 2000 20000}
EXE=uvc_amd/csrc/uvc1-mi355x
LOG=$OUT/merge_regions_$(basename $D).txt
TMP=$(mktemp -d)
: > $LOG
run() {   # label exe args...
    local label=$1 exe=$2; shift 2
    local t0=$(date +%s%N)
    timeout -k 10 300 $exe $D/p.bam -f $D/p.fa -o $TMP/o.vcf.gz -s S -R $D/panel.bed -t 1 --timing "$@" 2> $TMP/o.err || { tail -5 $TMP/o.err; return 1; }
    local t1=$(date +%s%N)
    echo "$label | wall $(( (t1 - t0) / 1000000 )) ms | $(grep -E 'record lines|thread-seconds' $TMP/o.err | tr -s ' ' | tr '\n' '|')" | tee -a $LOG
}
for rep in 1 2 3; do
    if [ -n "$PARENT_EXE" ]; then run "parent -R" $PARENT_EXE || exit 1; fi
    run "this -R" $EXE || exit 1
    for n in $NS; do run "this -R --merge-regions $n" $EXE --merge-regions $n || exit 1; done
done
rm -rf $TMP
