#!/bin/bash
# GPU-box helper: kernel trace of a short bench run, reduced to a per-step timeline (kernel busy time vs idle gaps) and the hand-off of the
# P2 phase of the accumulate: how long after the end of the last k_p2_fast pass in front of the join k_p2_items and k_frag16 start, and when
# the side streams' kernels end.
#   TRACE_ARGS="--serial --tiles 2" bash scripts/gpu_trace.sh     (one tile alone: the chains show in full)
cd "${GRAFT_REPO_ROOT:-.}"
mkdir -p gpurun_out/trace
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d gpurun_out/trace/run -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras --tiles 4 $TRACE_ARGS > gpurun_out/trace/bench.json 2> gpurun_out/trace/err.txt
[ $? -eq 0 ] || { echo "the traced bench run failed (see err.txt beside the trace)"; exit 3; }
python3 - <<'PY'
import csv, glob, re
f = glob.glob("gpurun_out/trace/run/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]) for r in rows]
mc = glob.glob("gpurun_out/trace/run/**/*memory_copy_trace.csv", recursive=True)
if mc:
    for r in csv.DictReader(open(mc[0])):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "memcpy_" + r.get("Direction", "")))
ev.sort()
def base(n): return re.sub(r"<.*", "", n.replace("void ", ""))   # "void k_p2_fast<true, false, true>" -> "k_p2_fast"
# last step = from the last P1 kernel of the main stream (k_prep_scan, or k_prep_fast in the window and split forms) to the end
starts = [i for i, e in enumerate(ev) if base(e[2]) in ("k_prep_fast", "k_prep_scan")]
i0 = starts[-1]
# include what the accumulate launches in front of it, and the memsets just before
while i0 > 0 and (ev[i0 - 1][2].startswith("__amd_rocclr") or base(ev[i0 - 1][2]) in ("k_win_index", "k_prep_sums", "k_prep_slow")): i0 -= 1
seg = ev[i0:]
t0 = seg[0][0]
busy = 0; prev_end = t0; gaps = []
for s, e, n in seg:
    if s > prev_end: gaps.append((s - prev_end, n))
    busy += max(0, e - max(s, prev_end)); prev_end = max(prev_end, e)
print("last step: span %.3f ms, busy %.3f ms, %d launches" % ((prev_end - t0) / 1e6, busy / 1e6, len(seg)))
# the hand-off behind the P2 phase: the LINK pass is k_p2_fast<true, ...> (or k_p2_fast_split<true, ...>)
link = [e for e in seg if base(e[2]) in ("k_p2_fast", "k_p2_fast_split") and "<true" in e[2]]
basep = [e for e in seg if base(e[2]) in ("k_p2_fast", "k_p2_fast_split") and "<false" in e[2]]
items = [e for e in seg if base(e[2]) == "k_p2_items"]
thres = [e for e in seg if base(e[2]) == "k_thres"]
# the last pass of k_p2_fast in front of the join: the LINK pass with UVCGPU_LINK=eager and before DESIGN 6-r8, the base pass since (the
# completion pass of LINK_M then runs behind k_p5b and is listed with the rest)
last, what = (link[-1], "LINK pass") if link else (None, "")
if basep and (not link or (items and link[-1][0] > items[0][0])): last, what = basep[-1], "base pass"
if last:
    l_end = last[1]
    print("%s ends at %.1f us" % (what, (l_end - t0) / 1e3))
    for want in ("k_p2_items", "k_frag_generic", "k_frag16", "k_frag16_split", "k_frag"):
        hit = [e for e in seg if base(e[2]) == want and e[0] >= last[0]]
        if hit: print("stall: %s starts %.1f us behind the end of the %s (runs %.1f us)" % (want, (hit[0][0] - l_end) / 1e3, what, (hit[0][1] - hit[0][0]) / 1e3))
    p2_side = ("k_p2_slow", "k_fragstat_fast", "k_win_index", "k_fragstat_sweep", "k_frag_sums", "k_p2_mism")
    t_fork = thres[-1][1] if thres else last[0]
    t_items = items[0][0] if items else l_end
    side = [e for e in seg if base(e[2]) in p2_side and e[0] >= t_fork and e[0] < max(l_end, t_items)]
    for s, e, n in side: print("P2-phase side kernel %-28s ends %8.1f us behind the end of the %s" % (n, (e - l_end) / 1e3, what))
for g, n in sorted(gaps, reverse=True)[:12]: print("gap %.1f us before %s" % (g / 1e3, n))
for s, e, n in seg: print("%9.1f %9.1f %s" % ((s - t0) / 1e3, (e - s) / 1e3, n))
PY
