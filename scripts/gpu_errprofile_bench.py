"""Times uvcgpu_region_error_profile on the bench's tile shape (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE config 4
shape) against the alternative a caller had before it: fetching the FRAG, FAM and DUPLEX plane groups whole and applying the definitions with
numpy.
    python scripts/gpu_errprofile_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--reps 25] [--kernel-only]
Range lists: one whole-tile range, 1000 windows, ~8000 ranges of 120 bp (25 bp on a 200 kb tile: npos / 8000).  The call is synchronous (table upload, two or three kernels, D2H of
the profile, stream synchronise), so the wall clock around it after warm-up is the time a caller sees; the median of --reps calls is printed
with the minimum and the maximum.  The kernel alone comes from a profiler run of this script with --kernel-only (rocprofv3 --kernel-trace
--stats --output-format csv -- python scripts/gpu_errprofile_bench.py --kernel-only): k_errprofile's rows of the trace, ten calls per list, in
list order.  One JSON line per figure."""
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


def numpy_profile(fetch, refseq, npos, gate):
    """The definitions of uvcgpu.h over whole fetched plane groups, every position of the region: what a caller computes today (the form
    tests/errprofile_restatement.py checks the kernel with)."""
    E = _ffi.ENUMS
    code = np.full(256, 4, np.int64)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = k
    sym = np.concatenate([code[np.frombuffer(refseq.encode(), np.uint8)], [4]])   # the region's last position has no reference base
    lft, rgt = np.concatenate([[4], sym[:-1]]), np.concatenate([sym[1:], [4]])
    has = (lft < 4) & (sym < 4) & (rgt < 4)
    ctx = np.where(has, 16 * lft + 4 * sym + rgt, 0)
    at = np.arange(npos)
    frag, fam, dup = fetch("FRAG"), fetch("FAM"), fetch("DUPLEX")
    levels = [frag[:, E["UVC_FRAG_bDP"]].sum(0, dtype=np.int64)] + [fam[:, E[k]].sum(0, dtype=np.int64) for k in ("UVC_FAM_cDP1", "UVC_FAM_cDP12", "UVC_FAM_cDP2")]
    levels.append(dup[E["UVC_DUPLEX_dDP1"]].astype(np.int64))
    out = np.zeros((E["UVC_NERRLEVEL"], E["UVC_ERR_ROW"]), np.int64)
    out[:, E["UVC_ERR_COUNTERS"] + E["UVC_ERRC_no_context"]] = int((~has).sum())
    for L, c in enumerate(levels):
        for first, c0, v, ref in ((E["UVC_ERR_BASE_BINS"], E["UVC_ERRC_BASE_counted"], c[E["UVC_BASE_A"]:E["UVC_BASE_T"] + 1], np.minimum(sym, 3)),
                                  (E["UVC_ERR_LINK_BINS"], E["UVC_ERRC_LINK_counted"], c[E["UVC_LINK_M"]:E["UVC_LINK_I1"] + 1], np.zeros(npos, np.int64))):
            d = v.sum(0)
            alt = v.copy()
            alt[ref, at] = 0
            cls = np.where(d < gate[0], 1, np.where(alt.max(0) * 1000 > gate[1] * d, 2, 0))
            for which in range(3):
                out[L, E["UVC_ERR_COUNTERS"] + c0 + which] = int((has & (cls == which)).sum())
            idx = np.nonzero(has & (cls == 0))[0]
            for s in range(v.shape[0]):
                np.add.at(out[L], first + ctx[idx] * v.shape[0] + s, v[s, idx])
    return out


ap = argparse.ArgumentParser()
ap.add_argument("--tile-kb", type=int, default=1000); ap.add_argument("--depth", type=int, default=300); ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--umi", action="store_true"); ap.add_argument("--kernel-only", action="store_true")
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.accumulate()
beg, npos = R.beg, R.npos
lists = {
    "one whole-tile range": [(beg, beg + npos)],
    "1000 windows": [(beg + k * (npos // 1000), beg + (k + 1) * (npos // 1000)) for k in range(1000)],
    "8000 ranges of 120 bp": [(beg + k * (npos // 8000), beg + k * (npos // 8000) + min(120, npos // 8000)) for k in range(8000)],
}
gate = (20, 50)
E = _ffi.ENUMS
cells = 4 * 2 * 11 + 11                                                      # plane cells per position: 4 levels x 2 strands x 11 symbols + dDP1's 11
print(json.dumps({"what": "byte floor", "positions": int(npos), "bytes_per_position": cells * 4, "us": round(cells * 4 * npos / 8000e9 * 1e6, 2)}))   # bench.py's HBM_PEAK_GBS


def med(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6, float(np.min(t)) * 1e6, float(np.max(t)) * 1e6


fn = lib.dll.uvcgpu_region_error_profile
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
req = _ffi.UvcErrorProfileRequest(*gate)
for what, ranges in lists.items():
    n_pos = sum(b - q for q, b in ranges)
    arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])   # built once: the C call alone is timed
    out = np.zeros((E["UVC_NERRLEVEL"], E["UVC_ERR_ROW"]), np.int64)

    def call():
        assert fn(R.h, arr, len(ranges), C.byref(req), out.ctypes.data) == 0
    if a.kernel_only:
        for _ in range(10):
            call()
        continue
    m, lo, hi = med(call, a.reps)
    print(json.dumps({"what": "uvcgpu_region_error_profile, " + what, "ranges": len(ranges), "positions": n_pos, "median_us": round(m, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                      "floor_us_for_these_positions": round(cells * 4 * n_pos / 8000e9 * 1e6, 2)}))

if not a.kernel_only:
    whole = lists["one whole-tile range"]

    def by_fetch():
        return numpy_profile(R.fetch, reads["refseq"], npos, gate)
    assert np.array_equal(R.error_profile(whole, *gate), by_fetch()), "the two ways disagree"
    m, lo, hi = med(by_fetch, max(3, a.reps // 8))
    nbytes = sum(R.lib.call("field_bytes", R.h, _ffi.FIELD_GROUPS[g][0]) for g in ("FRAG", "FAM", "DUPLEX"))
    print(json.dumps({"what": "whole-group fetch of FRAG + FAM + DUPLEX and the numpy restatement, one whole-tile range", "bytes_copied": int(nbytes), "median_us": round(m, 1), "min_us": round(lo, 1), "max_us": round(hi, 1)}))
R.close()
