"""Times uvcgpu_region_msi on the bench's tile shapes (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE config 4 shape)
(DESIGN.md 4n).
    python scripts/gpu_msi_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--reps 25]
Range lists: one whole-tile range, 1000 windows.  Requests: the defaults (tracts of >= 10 bp and >= 5 units of <= 6 bp) and the stress
request min_tracklen = min_units = 1, under which nearly every start of the repeat walk is a locus.  Every combination is checked against
the numpy restatement (tests/msi_restatement.py over the handle's own fetched planes and allele rows) before it is timed.  The call is
synchronous (table upload, fill of the rows, heads + scan + emit + depth + bin, 4 bytes D2H, 256 bytes per locus D2H); the buffer has room
after the warm-up calls, so one pass returns the rows.  Kernel time: uvcgpu_region_kernel_times, the entries k_msi (one per pass); median
and minimum of --reps calls after 3 warm-up calls.  Byte floor of the two passes over the STR planes: 2 x 12 bytes per position, plus 2 x
256 bytes per locus for the fill and the copy of the rows, over bench.py's HBM peak.  One JSON line per figure."""
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
import msi_restatement as mr               # noqa: E402
from uvc_amd import _ffi, region, synth    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tile-kb", type=int, default=1000); ap.add_argument("--depth", type=int, default=300); ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--umi", action="store_true")
a = ap.parse_args()
HBM_PEAK_GBS = 8000.0   # bench.py's
E = _ffi.ENUMS
ROW = E["UVC_MSI_ROW"]

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.accumulate()
beg, npos = R.beg, R.npos
base = slice(E["UVC_BASE_A"], E["UVC_BASE_NN"] + 1)
frag, fam, dup = R.fetch("FRAG"), R.fetch("FAM"), R.fetch("DUPLEX")
m4 = np.stack([frag[:, E["UVC_FRAG_bDP"], base].sum((0, 1), dtype=np.int64), fam[:, E["UVC_FAM_cDP12"], base].sum((0, 1), dtype=np.int64),
               fam[:, E["UVC_FAM_cDP2"], base].sum((0, 1), dtype=np.int64), dup[E["UVC_DUPLEX_dDP1"], base].sum(0, dtype=np.int64)])
del frag, fam, dup
rtr, alleles = R.fetch("RTR"), R.indel_alleles()
print(json.dumps({"what": "input", "positions": int(npos), "alignments": int(reads["n_reads"]), "allele_rows": len(alleles)}))
lists = {
    "one whole-tile range": [(beg, beg + npos)],
    "1000 windows": [(beg + k * (npos // 1000), beg + (k + 1) * (npos // 1000)) for k in range(1000)],
}
requests = {"defaults (10 bp, 5 units, unit <= 6)": (10, 5, 6), "stress (min_tracklen = min_units = 1)": (1, 1, 6)}
fn = lib.dll.uvcgpu_region_msi
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()


def kernel_ms():
    """(the sum of the k_msi entries, their number: one per pass of the call)"""
    n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    mine = [ms_buf[i] for i in range(n) if i < len(names) and names[i] == "k_msi"]
    return sum(mine), len(mine)


def stats(v, scale):
    return round(float(np.median(v)) * scale, 1), round(float(np.min(v)) * scale, 1)


lib.dll.uvcgpu_region_set_profiling(R.h, 1)
for what, ranges in lists.items():
    n_pos = sum(q - p for p, q in ranges)
    arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])   # built once: the C call alone is timed
    for rname, rq in requests.items():
        want, classes = mr.tally(rtr, beg, ranges, m4, alleles, reads["refseq"], *rq)
        got = R.msi(ranges, *rq)
        assert np.array_equal(got, want), (what, rname)
        req = _ffi.UvcMsiRequest(*rq)
        buf = np.zeros((len(want) + 1, ROW), np.int32)
        n = C.c_int64(0)
        wall, kern, passes = [], [], []
        for rep in range(a.reps + 3):
            R.accumulate()                                   # starts the handle's list of timed kernels (32 entries) anew
            assert lib.dll.uvcgpu_region_sync(R.h) == 0
            t0 = time.perf_counter()
            assert fn(R.h, arr, len(ranges), C.byref(req), buf.ctypes.data, len(buf), C.byref(n)) == 0
            t1 = time.perf_counter()
            if rep >= 3:
                k, p = kernel_ms()
                wall.append(t1 - t0); kern.append(k); passes.append(p)
        assert n.value == len(want) and np.array_equal(buf[:len(want)], want)
        floor_us = (24 * n_pos + 512 * len(want)) / (HBM_PEAK_GBS * 1e9) * 1e6
        km, kmin = stats(kern, 1e3)
        print(json.dumps({"what": "uvcgpu_region_msi, " + what + ", " + rname, "ranges": len(ranges), "positions": n_pos, "loci": int(len(want)), "loci_EDGE": int((want[:, 4] & 1).sum()),
                          "allele_rows_binned": int(sum(v for k, v in classes.items() if k not in ("no_locus", "edge", "tail", "behind_last_unit"))), "passes": int(max(passes)),
                          "kernels_median_us": km, "kernels_min_us": kmin, "call_median_us": stats(wall, 1e6)[0], "call_min_us": stats(wall, 1e6)[1],
                          "byte_floor_us": round(floor_us, 2), "fraction_of_floor": round(floor_us / km, 3) if km else None}))
R.close()
