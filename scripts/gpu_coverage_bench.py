"""Times uvcgpu_region_coverage on the bench's tile shape (1 Mb x 300x, non-UMI) against the alternative a caller had before it: fetching
the PREP32, FRAG, FAM and DUPLEX plane groups whole and summing them with numpy.
    python scripts/gpu_coverage_bench.py [--tile-kb 1000] [--depth 300] [--reps 25] [--kernel-only]
Range lists: one whole-tile range, 1000 windows of 1 kb, ~8000 ranges of 120 bp.  The call is synchronous (table upload, two kernels, D2H of the
rows, stream synchronise), so the wall clock around it after warm-up is the time a caller sees; the median of --reps calls is printed.  The
kernel alone comes from a profiler run of this script with --kernel-only (rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/gpu_coverage_bench.py
--kernel-only): k_coverage's rows of the stats table, ten calls per list.  One JSON line per figure."""
import argparse
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
ap.add_argument("--kernel-only", action="store_true")
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.accumulate()
beg, npos = R.beg, R.npos
lists = {
    "one whole-tile range": [(beg, beg + npos)],
    "1000 windows of 1 kb": [(beg + k * (npos // 1000), beg + (k + 1) * (npos // 1000)) for k in range(1000)],
    "8000 ranges of 120 bp": [(beg + k * (npos // 8000), beg + k * (npos // 8000) + min(120, npos // 8000)) for k in range(8000)],
}
thr = [1, 20, 100, 500]
E = _ffi.ENUMS
cells = 1 + 2 * 6 * (1 + 3) + 6                                              # plane cells per position behind the six measures
floor_us = cells * 4 * npos / 8000e9 * 1e6                                   # bench.py's HBM_PEAK_GBS
print(json.dumps({"what": "byte floor", "positions": int(npos), "bytes_per_position": cells * 4, "us": round(floor_us, 2)}))


def med(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6, float(np.min(t)) * 1e6


import ctypes as C    # noqa: E402
fn = lib.dll.uvcgpu_region_coverage
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
thr_arr = np.array(thr, np.int32)
for what, ranges in lists.items():
    n_pos = sum(b - q for q, b in ranges)
    arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])   # built once: the C call alone is timed
    out = np.zeros((len(ranges), E["UVC_NCOV"], E["UVC_COV_ROW"]), np.int64)

    def call():
        assert fn(R.h, arr, len(ranges), thr_arr.ctypes.data, len(thr), out.ctypes.data) == 0
    if a.kernel_only:
        for _ in range(10):
            call()
        continue
    m, lo = med(call, a.reps)
    assert np.array_equal(out[:, :, :3 + len(thr)], R.coverage(ranges, thr))
    print(json.dumps({"what": "uvcgpu_region_coverage, " + what, "ranges": len(ranges), "positions": n_pos, "median_us": round(m, 1), "min_us": round(lo, 1),
                      "floor_us_for_these_positions": round(cells * 4 * n_pos / 8000e9 * 1e6, 2)}))

if not a.kernel_only:
    base = slice(E["UVC_BASE_A"], E["UVC_BASE_NN"] + 1)

    def by_fetch():
        prep, frag, fam, dup = (R.fetch(g) for g in ("PREP32", "FRAG", "FAM", "DUPLEX"))
        m = [prep[E["UVC_P_a_dp"]].astype(np.int64), frag[:, E["UVC_FRAG_bDP"], base].sum((0, 1), dtype=np.int64)]
        m += [fam[:, E[k], base].sum((0, 1), dtype=np.int64) for k in ("UVC_FAM_cDP1", "UVC_FAM_cDP12", "UVC_FAM_cDP2")]
        m.append(dup[E["UVC_DUPLEX_dDP1"], base].sum(0, dtype=np.int64))
        return [(v.sum(), v.min(), v.max(), [(v >= t).sum() for t in thr]) for v in m]
    got = R.coverage(lists["one whole-tile range"], thr)[0]
    want = by_fetch()
    assert all(got[i, 0] == w[0] and got[i, 1] == w[1] and got[i, 2] == w[2] and got[i, 3:].tolist() == [int(x) for x in w[3]] for i, w in enumerate(want)), "the two ways disagree"
    m, lo = med(by_fetch, max(3, a.reps // 5))
    nbytes = sum(R.lib.call("field_bytes", R.h, _ffi.FIELD_GROUPS[g][0]) for g in ("PREP32", "FRAG", "FAM", "DUPLEX"))
    print(json.dumps({"what": "whole-group fetch of PREP32 + FRAG + FAM + DUPLEX and numpy sums, one whole-tile range", "bytes_copied": int(nbytes), "median_us": round(m, 1), "min_us": round(lo, 1)}))
R.close()
