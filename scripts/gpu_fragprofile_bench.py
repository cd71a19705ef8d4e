"""Times uvcgpu_region_fragment_profile on the bench's tile shapes (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE
config 4 shape), DESIGN.md 4o.
    python scripts/gpu_fragprofile_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--reps 25]
Range lists: one whole-tile range, 16 and 17 ranges, 1000 windows (more than a block's LDS window of 256 ranges), ~8000 ranges of 120 bp.
Two figures per list: the kernels alone, from HIP events around the five launches on the handle's stream (uvcgpu_region_set_profiling +
uvcgpu_region_kernel_times, entry k_fragprofile; median and minimum of --reps calls after 3 warm-up calls), and the synchronous call as a
caller sees it (ranges upload, kernels, D2H of the rows and the profile, stream synchronise; wall clock).  The result of every list is
checked against the numpy restatement of tests/fragprofile_restatement.py first.  One JSON line per figure."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fragprofile_restatement as fp       # noqa: E402
from uvc_amd import _ffi, region, synth    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tile-kb", type=int, default=1000); ap.add_argument("--depth", type=int, default=300); ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--umi", action="store_true")
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.accumulate()   # (accumulate starts the list of kernel times anew: the calls below come behind it)
frs = fp.fragments(reads, 0)
fams = fp.families(frs)
beg, npos = R.beg, R.npos
print(json.dumps({"what": "input", "positions": int(npos), "alignments": int(reads["n_reads"]), "fragments": int(len(frs["kind"])), "pairs": int((frs["kind"] == fp.KIND_PAIR).sum()),
                  "sized_families": int(len(fams["fam"]))}), flush=True)


def chain(pairs):
    return [(p, q, pairs[k - 1][1] if k else 0, 0) for k, (p, q) in enumerate(pairs)]


lists = {
    "one whole-tile range": chain([(beg, beg + npos)]),
    "16 ranges": chain([(beg + k * (npos // 16), beg + (k + 1) * (npos // 16)) for k in range(16)]),
    "17 ranges": chain([(beg + k * (npos // 17), beg + (k + 1) * (npos // 17)) for k in range(17)]),
    "1000 windows": chain([(beg + k * (npos // 1000), beg + (k + 1) * (npos // 1000)) for k in range(1000)]),
    "8000 ranges of 120 bp": chain([(beg + k * (npos // 8000), beg + k * (npos // 8000) + min(120, npos // 8000)) for k in range(8000)]),
}
fn = lib.dll.uvcgpu_region_fragment_profile
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()
req = _ffi.UvcFragmentProfileRequest(0, 100, 150, 151, 220)


def kernel_ms():
    n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    return [ms_buf[i] for i in range(n) if i < len(names) and names[i] == "k_fragprofile"]


lib.dll.uvcgpu_region_set_profiling(R.h, 1)
for what, ranges in lists.items():
    arr = (_ffi.UvcFamilyRange * len(ranges))(*[_ffi.UvcFamilyRange(*q) for q in ranges])   # built once: the C call alone is timed
    rows, prof = np.zeros((len(ranges), _ffi.ENUMS["UVC_FRAGPROF_TARGET_ROW"]), np.int64), np.zeros(_ffi.ENUMS["UVC_FRAGPROF_ROW"], np.int64)
    assert fn(R.h, arr, len(ranges), C.byref(req), rows.ctypes.data, prof.ctypes.data) == 0, lib.last_error()
    want_rows, want_prof = fp.rows_and_profile(frs, fams, ranges, beg, reads["refseq"])
    assert np.array_equal(rows, want_rows) and np.array_equal(prof, want_prof), what
    wall, kern = [], []
    for rep in range(a.reps + 3):
        R.accumulate()                                   # starts the handle's list of timed kernels (32 entries) anew
        assert lib.dll.uvcgpu_region_sync(R.h) == 0      # accumulate returns before its kernels end: the call below would wait for them
        t0 = time.perf_counter()
        assert fn(R.h, arr, len(ranges), C.byref(req), rows.ctypes.data, prof.ctypes.data) == 0
        t1 = time.perf_counter()
        k = kernel_ms()
        if rep >= 3:
            wall.append(t1 - t0); kern += k[-1:]
    print(json.dumps({"what": "uvcgpu_region_fragment_profile, " + what, "ranges": len(ranges), "reps": a.reps, "pairs_in_profile": int(prof[fp.PAIRS]),
                      "kernels_median_us": round(float(np.median(kern)) * 1e3, 1) if kern else None, "kernels_min_us": round(float(np.min(kern)) * 1e3, 1) if kern else None,
                      "call_median_us": round(float(np.median(wall)) * 1e6, 1), "call_min_us": round(float(np.min(wall)) * 1e6, 1), "call_max_us": round(float(np.max(wall)) * 1e6, 1)}), flush=True)
R.close()
