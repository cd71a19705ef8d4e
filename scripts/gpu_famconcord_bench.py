"""Times uvcgpu_region_family_concordance on the bench's two tile shapes -- 1 Mb x 300x without UMIs and 200 kb x 2000x
duplex-UMI (the BASELINE config 4 shape) -- for one whole-tile range and for about 8 000 short ranges, and writes profiles/famconcord_bench.json.
    python scripts/gpu_famconcord_bench.py [--reps 15] [--out profiles/famconcord_bench.json] [--small]
Per tile and range list: the wall clock around the synchronous call after warm-up (median, minimum, maximum of --reps calls) and its two
entries of uvcgpu_region_kernel_times (k_famconc_units, k_famconc_duplex with the fold), five repeats each.  The yardstick is the sum of the
family-pass kernels of the same tile's accumulate (k_fam_p4*, k_fam_p5*, k_duplex*) from the same timing call, five accumulates: the report
evaluates each unit's votes once and does none of the bias arithmetic.  --small: tiles of a twentieth of the size (a dry run)."""
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
ap.add_argument("--reps", type=int, default=15); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "famconcord_bench.json")); ap.add_argument("--small", action="store_true")
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
fn = lib.dll.uvcgpu_region_family_concordance
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
ROW = _ffi.ENUMS["UVC_FAMCONC_ROW"]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()


def kernel_times(R):
    n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    return list(zip(names_buf.value.decode().split(";")[:n], [float(v) for v in list(ms_buf)[:n]]))


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


TILES = [("1mb_300x", dict(seed=777, region_len=1000_000, depth=300, umi=False)), ("200kb_2000x_duplex_umi", dict(seed=777, region_len=200_000, depth=2000, umi=True))]
result = {"what": "uvcgpu_region_family_concordance: wall time of the call and its kernels' times against the family-pass kernels of the same tile's accumulate", "times_in": "ms", "tiles": {}}
for name, kw in TILES:
    if a.small:
        kw = dict(kw, region_len=kw["region_len"] // 20)
    reads = synth.generate_region(**kw)
    R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    fam_pass = []
    for _ in range(5):                                   # the yardstick: the family-pass kernels of five accumulates
        lib.dll.uvcgpu_region_set_profiling(R.h, 1)
        R.accumulate()
        kt = kernel_times(R)
        fam_pass.append({k: v for k, v in kt if k.startswith(("k_fam_p4", "k_fam_p5", "k_duplex"))})
    beg, npos = R.beg, R.npos
    step = max(npos // 8000, 1)
    lists = {"one whole-tile range": [(beg, beg + npos)], "%d ranges of %d bp" % (npos // step, min(25, step)): [(beg + k * step, beg + k * step + min(25, step)) for k in range(npos // step)]}
    tile = {"positions": int(npos), "reads": int(reads["n_reads"]), "family_pass_kernels_of_accumulate": {"per_kernel_median": {k: round(float(np.median([f[k] for f in fam_pass])), 4) for k in fam_pass[0]},
                                                                                                     "sum": spread([sum(f.values()) for f in fam_pass])}, "calls": {}}
    for what, ranges in lists.items():
        arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])   # built once: the C call alone is timed
        out = np.zeros(ROW, np.int64)

        def call():
            assert fn(R.h, arr, len(ranges), out.ctypes.data) == 0, lib.last_error()
        for _ in range(3):
            call()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
        kts = []
        for _ in range(5):
            lib.dll.uvcgpu_region_set_profiling(R.h, 1)  # the list starts anew: the call's two entries alone
            call()
            kts.append(dict(kernel_times(R)))
        tile["calls"][what] = {"ranges": len(ranges), "positions": int(sum(b - q for q, b in ranges)), "wall": spread(wall),
                               "kernels": {k: spread([t[k] for t in kts]) for k in kts[0]}, "kernels_sum": spread([sum(t.values()) for t in kts]),
                               "unit_positions": int(out[_ffi.ENUMS["UVC_FAMCONC_COUNTERS"] + _ffi.ENUMS["UVC_FAMCONCC_unit_positions"]])}
        print(json.dumps({name + ", " + what: tile["calls"][what]}), flush=True)
    result["tiles"][name] = tile
    print(json.dumps({name: tile["family_pass_kernels_of_accumulate"]}), flush=True)
    R.close()
with open(a.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
