"""Times uvcgpu_region_clip_junctions on the tile shapes the clip-site call was measured on (1 Mb x 300x, non-UMI; --umi --tile-kb 200
--depth 2000: the BASELINE config 4 shape), DESIGN.md 4r, for the library and for the naive build of the kernel file
(tests/native/libuvcgpu_clipjunc_naive.so) in one session.
    python scripts/gpu_clipjunctions_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--clip-frac 0.05] [--reps 25] [--min-votes 2]
The site rows are those Region.clip_sites returns over the whole tile at min_clip 10, min_mapq 0 and min_reads 3 and 1; the request is the
default one but for --min-votes (1: the single-read sites of min_reads 1 are searched as well, the heaviest list).
Figures per list and build: the four stages alone, from HIP events around their launches on the handle's stream
(uvcgpu_region_set_profiling + uvcgpu_region_kernel_times, entries k_clipjunc_pack / _queries / _search / _finish; median, minimum and
maximum of --reps calls after 3 warm-up calls) and the synchronous call as a caller sees it (row upload, the four stages, D2H of the
junction rows; wall clock; arrays prebuilt).  Beside them the (window, site, strand) triples of the list -- per searched site two strands
times the window starts whose query_len positions lie inside the reference -- and the triples per second of the search stage's median.
Each list is checked for what holds without a restatement: two calls and the two builds return the same bytes, the totals add up.
One JSON line per list and build."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uvc_amd import _ffi, region, synth    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tile-kb", type=int, default=1000); ap.add_argument("--depth", type=int, default=300); ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--umi", action="store_true"); ap.add_argument("--clip-frac", type=float, default=0.05); ap.add_argument("--min-votes", type=int, default=2)
ap.add_argument("--naive-library", default=os.path.join(ROOT, "tests", "native", "libuvcgpu_clipjunc_naive.so"))
a = ap.parse_args()

STAGES = ["k_clipjunc_pack", "k_clipjunc_queries", "k_clipjunc_search", "k_clipjunc_finish"]
libs = [("packed", region.gpu_lib()), ("naive", _ffi.Lib(a.naive_library, "uvcgpu_"))]
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi, clip_frac=a.clip_frac)
regions = []
for name, lib in libs:
    assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
    assert lib.dll.uvc_clipjunc_naive() == (name == "naive")
    R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
    lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
    lib.dll.uvcgpu_region_set_profiling(R.h, 1)
    regions.append(R)
n = regions[0].npos - 1
print(json.dumps({"what": "input", "positions": int(n + 1), "alignments": int(reads["n_reads"]), "clip_frac": a.clip_frac, "min_votes": a.min_votes}), flush=True)
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()
JROW, E = _ffi.ENUMS["UVC_CLIPJUNC_ROW"], _ffi.ENUMS
W = {name: first for name, first, _ in _ffi.CLIPJUNC_SECTIONS}


def kernel_ms(lib, R):
    k = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    return [(names[i], ms_buf[i]) for i in range(k) if i < len(names)]


def us(v):
    return {"median": round(float(np.median(v)) * 1e6, 1), "min": round(float(np.min(v)) * 1e6, 1), "max": round(float(np.max(v)) * 1e6, 1)} if len(v) else None


whole = [(regions[0].beg, regions[0].beg + regions[0].npos)]
for min_reads in (3, 1):
    rows = np.ascontiguousarray(regions[0].clip_sites(whole, 0, 10, min_reads)[1])
    ns = len(rows)
    want = None
    for (name, lib), R in zip(libs, regions):
        fn = lib.dll.uvcgpu_region_clip_junctions
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        req = _ffi.UvcClipJunctionsRequest(a.min_votes, 16, 1, 0, 10)
        out, totals = np.zeros((max(ns, 1), JROW), np.int64), np.zeros(8, np.int64)
        wall, stage = [], {s: [] for s in STAGES}
        for rep in range(a.reps + 3):
            R.accumulate()                                   # starts the handle's list of timed kernels (32 entries, 28 of them its own) anew
            assert lib.dll.uvcgpu_region_sync(R.h) == 0      # accumulate returns before its kernels end: the call below would wait for them
            t0 = time.perf_counter()
            assert fn(R.h, rows.ctypes.data, ns, C.byref(req), out.ctypes.data, totals.ctypes.data) == 0, lib.last_error()
            t1 = time.perf_counter()
            if want is None:
                want = (out.tobytes(), totals.tobytes())     # two calls and the two builds: the same bytes
            assert (out.tobytes(), totals.tobytes()) == want, (name, rep)
            if rep >= 3:
                wall.append(t1 - t0)
                last = dict(kernel_ms(lib, R)[-len(STAGES):])
                for s in STAGES:
                    stage[s].append(last[s] * 1e-3)
        j = out[:ns]
        searched = j[:, W["status"]] != E["UVC_CLIPJUNC_NOT_SEARCHED"]
        assert totals.tolist()[:5] == [ns, int(searched.sum()), int((j[:, W["status"]] == E["UVC_CLIPJUNC_PLACED"]).sum()), int((j[:, W["n_best"]] == 1).sum()), int((j[:, W["mate"]] >= 0).sum())]
        triples = int(2 * np.maximum(0, n - j[searched, W["query_len"]] + 1).sum())
        med = float(np.median(stage["k_clipjunc_search"]))
        print(json.dumps({"what": "uvcgpu_region_clip_junctions on the rows of clip_sites over the tile", "library": name, "min_reads": min_reads, "min_votes": a.min_votes, "reps": a.reps, "sites": ns,
                          "totals": totals[:5].tolist(), "classes": np.bincount(j[:, W["klass"]], minlength=5).tolist(), "pack_stage_us": us(stage["k_clipjunc_pack"]), "queries_stage_us": us(stage["k_clipjunc_queries"]),
                          "search_stage_us": us(stage["k_clipjunc_search"]), "finish_stage_us": us(stage["k_clipjunc_finish"]), "call_us": us(wall), "triples": triples,
                          "triples_per_s": round(triples / med, 1) if med > 0 else None}), flush=True)
for R in regions:
    R.close()
