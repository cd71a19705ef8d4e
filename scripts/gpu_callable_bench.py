"""Times uvcgpu_region_callable on the bench's tile shapes (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE config 4
shape) against k_coverage on the same tile and list and against the alternative a caller had before it: fetching the PREP32, FRAG, FAM and
DUPLEX plane groups whole and finding the runs with numpy.
    python scripts/gpu_callable_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--reps 25] [--no-fetch]
Range lists: one whole-tile range, 1000 windows, 8000 ranges of 120 bp.  Requests: the default (cDP12=20), all six measures at their medians
over the tile, and cDP12 at its median with max_aDP at the median of aDP, which flips the mask as often as these depths allow.  Every list
is checked against the numpy restatement (tests/callable_restatement.py over the handle's own fetched planes) before it is timed.  The
worst case -- every position a run -- is a fourth list, every position of the tile as a range of its own, with the all-medians request.  The call
is synchronous (table upload, count + scan, 4 bytes D2H, emit, 16 bytes per run D2H); the buffer has room, so one call returns the runs.
Kernel time: uvcgpu_region_kernel_times, the sum of the entries k_callable_count (count + scan) and k_callable_emit; median and minimum of
--reps calls after 3 warm-up calls.  Byte floor: 4 bytes per tested cell and position plus 16 bytes per run over bench.py's HBM peak.  One
JSON line per figure."""
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
import callable_restatement as cr          # noqa: E402
from uvc_amd import _ffi, region, synth    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tile-kb", type=int, default=1000); ap.add_argument("--depth", type=int, default=300); ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--umi", action="store_true"); ap.add_argument("--no-fetch", action="store_true")
a = ap.parse_args()
HBM_PEAK_GBS = 8000.0   # bench.py's
E = _ffi.ENUMS
M = region.COVERAGE_MEASURES
CELLS = [1, 12, 12, 12, 12, 6]   # plane cells per position behind each measure: both strands x the six BASE symbols where the group has them

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.accumulate()
beg, npos = R.beg, R.npos
base = slice(E["UVC_BASE_A"], E["UVC_BASE_NN"] + 1)


def measures_by_fetch():
    prep, frag, fam, dup = (R.fetch(g) for g in ("PREP32", "FRAG", "FAM", "DUPLEX"))
    m = [prep[E["UVC_P_a_dp"]].astype(np.int64), frag[:, E["UVC_FRAG_bDP"], base].sum((0, 1), dtype=np.int64)]
    m += [fam[:, E[k], base].sum((0, 1), dtype=np.int64) for k in ("UVC_FAM_cDP1", "UVC_FAM_cDP12", "UVC_FAM_cDP2")]
    m.append(dup[E["UVC_DUPLEX_dDP1"], base].sum(0, dtype=np.int64))
    return np.stack(m)


m = measures_by_fetch()
med = {M[k]: int(np.median(m[k])) for k in range(len(M))}
print(json.dumps({"what": "input", "positions": int(npos), "alignments": int(reads["n_reads"]), "medians": med}))
lists = {
    "one whole-tile range": [(beg, beg + npos)],
    "1000 windows": [(beg + k * (npos // 1000), beg + (k + 1) * (npos // 1000)) for k in range(1000)],
    "8000 ranges of 120 bp": [(beg + k * (npos // 8000), beg + k * (npos // 8000) + min(120, npos // 8000)) for k in range(8000)],
}
requests = {
    "default (cDP12=20)": ({"cDP12": 20}, 0),
    "all six at their medians": ({k: v for k, v in med.items() if v > 0}, 0),
    "cDP12 at its median, max_aDP at the median of aDP": ({"cDP12": med["cDP12"]}, med["aDP"]),
}
fn = lib.dll.uvcgpu_region_callable
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
cov = lib.dll.uvcgpu_region_coverage
cov.restype, cov.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()


def kernel_ms():
    n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    return sum(ms_buf[i] for i in range(n) if i < len(names) and names[i].startswith("k_callable"))


def stats(v, scale):
    return round(float(np.median(v)) * scale, 1), round(float(np.min(v)) * scale, 1)


lib.dll.uvcgpu_region_set_profiling(R.h, 1)
for what, ranges in lists.items():
    n_pos = sum(q - p for p, q in ranges)
    arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])   # built once: the C call alone is timed
    thr = np.array([1, 20, 100, 500], np.int32)
    rows = np.zeros((len(ranges), E["UVC_NCOV"], E["UVC_COV_ROW"]), np.int64)
    wall = []
    for rep in range(a.reps + 3):
        t0 = time.perf_counter()
        assert cov(R.h, arr, len(ranges), thr.ctypes.data, 4, rows.ctypes.data) == 0
        wall.append(time.perf_counter() - t0)
    print(json.dumps({"what": "uvcgpu_region_coverage (yardstick), " + what, "ranges": len(ranges), "positions": n_pos, "call_median_us": stats(wall[3:], 1e6)[0], "call_min_us": stats(wall[3:], 1e6)[1]}))
    for rname, (min_depth, max_aDP) in requests.items():
        md, mx = cr.request(min_depth, max_aDP)
        want = cr.runs_of(m, beg, ranges, md, mx)
        got = R.callable(ranges, min_depth, max_aDP)
        assert np.array_equal(got, want), (what, rname)
        req = _ffi.UvcCallableRequest((C.c_int32 * 6)(*md), mx)
        buf = np.zeros(len(want) + 1, region.CALLABLE_RUN)
        n = C.c_int64(0)
        wall, kern = [], []
        for rep in range(a.reps + 3):
            R.accumulate()                                   # starts the handle's list of timed kernels (32 entries) anew
            assert lib.dll.uvcgpu_region_sync(R.h) == 0
            t0 = time.perf_counter()
            assert fn(R.h, arr, len(ranges), C.byref(req), buf.ctypes.data, len(buf), C.byref(n)) == 0
            t1 = time.perf_counter()
            if rep >= 3:
                wall.append(t1 - t0); kern.append(kernel_ms())
        assert n.value == len(want) and np.array_equal(buf[:len(want)], want)
        cells = sum(c for c, t in zip(CELLS, md) if t > 0) + (0 if md[0] > 0 else 1)
        floor_us = (4 * cells * n_pos + 16 * len(want)) / (HBM_PEAK_GBS * 1e9) * 1e6
        km, kmin = stats(kern, 1e3)
        print(json.dumps({"what": "uvcgpu_region_callable, " + what + ", " + rname, "ranges": len(ranges), "positions": n_pos, "runs": int(len(want)), "tested_cells_per_position": cells,
                          "kernels_median_us": km, "kernels_min_us": kmin, "call_median_us": stats(wall, 1e6)[0], "call_min_us": stats(wall, 1e6)[1],
                          "byte_floor_us": round(floor_us, 2), "fraction_of_floor": round(floor_us / km, 3) if km else None}))

# the worst case of the emit and of the way home: every position its own range, so every position is a run (16 B per position)
arr = np.empty((npos, 2), np.int32)
arr[:, 0] = np.arange(beg, beg + npos); arr[:, 1] = arr[:, 0] + 1
md, mx = cr.request(*requests["all six at their medians"])
want = np.zeros(npos, cr.RUN)
want["range"], want["pos_beg"], want["pos_end"], want["mask"] = np.arange(npos), arr[:, 0], arr[:, 1], cr.masks_of(m, md, mx)
req = _ffi.UvcCallableRequest((C.c_int32 * 6)(*md), mx)
buf = np.zeros(npos + 1, region.CALLABLE_RUN)
n = C.c_int64(0)
wall, kern = [], []
for rep in range(a.reps + 3):
    R.accumulate()
    assert lib.dll.uvcgpu_region_sync(R.h) == 0
    t0 = time.perf_counter()
    assert fn(R.h, arr.ctypes.data, npos, C.byref(req), buf.ctypes.data, len(buf), C.byref(n)) == 0, lib.last_error()
    t1 = time.perf_counter()
    if rep >= 3:
        wall.append(t1 - t0); kern.append(kernel_ms())
assert n.value == npos and np.array_equal(buf[:npos], want), "every position its own range"
cells = sum(c for c, t in zip(CELLS, md) if t > 0) + (0 if md[0] > 0 else 1)
floor_us = (4 * cells * npos + 16 * npos) / (HBM_PEAK_GBS * 1e9) * 1e6
km, kmin = stats(kern, 1e3)
print(json.dumps({"what": "uvcgpu_region_callable, every position its own range, all six at their medians", "ranges": int(npos), "positions": int(npos), "runs": int(npos), "tested_cells_per_position": cells,
                  "kernels_median_us": km, "kernels_min_us": kmin, "call_median_us": stats(wall, 1e6)[0], "call_min_us": stats(wall, 1e6)[1],
                  "byte_floor_us": round(floor_us, 2), "fraction_of_floor": round(floor_us / km, 3) if km else None}))

if not a.no_fetch:
    def by_fetch():
        return cr.runs_of(measures_by_fetch(), beg, lists["one whole-tile range"], *cr.request(*requests["all six at their medians"]))
    assert np.array_equal(by_fetch(), R.callable(lists["one whole-tile range"], *requests["all six at their medians"])), "the two ways disagree"
    t = []
    for rep in range(max(3, a.reps // 5) + 1):
        t0 = time.perf_counter(); by_fetch(); t.append(time.perf_counter() - t0)
    nbytes = sum(R.lib.call("field_bytes", R.h, _ffi.FIELD_GROUPS[g][0]) for g in ("PREP32", "FRAG", "FAM", "DUPLEX"))
    print(json.dumps({"what": "whole-group fetch of PREP32 + FRAG + FAM + DUPLEX and numpy runs, one whole-tile range, all six", "bytes_copied": int(nbytes),
                      "median_us": stats(t[1:], 1e6)[0], "min_us": stats(t[1:], 1e6)[1]}))
R.close()
