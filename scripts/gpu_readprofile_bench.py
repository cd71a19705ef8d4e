"""Times uvcgpu_region_read_profile on the bench's tile shape (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE config 4
shape) and sets it against what a caller has without it: the definitions in vectorised numpy over the same read columns on the host
(DESIGN.md 4m).
    python scripts/gpu_readprofile_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--reps 25] [--baseline-kb 100]
Range lists: one whole-tile range, 1000 windows, 8000 short ranges.  The kernels alone come from the handle's own HIP events
(uvcgpu_region_set_profiling + uvcgpu_region_kernel_times, entries k_readprofile_depth / _status / _bin; median of --reps calls after 3
warm-up calls), the synchronous call from the wall clock around it.  The byte floor is one read of the packed base | quality column (two
bytes per read base), the CIGARs and the status bytes (one per position) at bench.py's 8 TB/s; "bytes_as_built" adds what the two passes
read on top of it (the one-byte bases of the first pass, the status byte once more per read base).  The numpy form holds several 8-byte
columns per read base, so it runs on a smaller tile (--baseline-kb) together with the device call on that same tile.  One JSON line per
figure."""
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

E = _ffi.ENUMS
ROW = E["UVC_READPROF_ROW"]


def numpy_row(reads, gate):
    """The definitions of uvcgpu.h over the columns, whole region, vectorised over the CIGAR ops and then over the bases."""
    min_mapq, min_depth, permille = gate
    beg, npos = int(reads["beg"]), int(reads["end"]) - int(reads["beg"]) + 1
    code = np.full(256, 4, np.int64)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = k
    ref = np.concatenate([code[np.frombuffer(reads["refseq"].encode(), np.uint8)], [4]])
    n = int(reads["n_reads"])
    nc = reads["n_cigar"].astype(np.int64)
    aln = np.repeat(np.arange(n), nc)                                        # the alignment of every op (ops lie back to back in read order)
    ops = np.concatenate([reads["cigars"][int(o):int(o) + int(k)] for o, k in zip(reads["cigar_off"], nc)]) if not np.array_equal(reads["cigar_off"], np.cumsum(nc) - nc) else reads["cigars"]
    op, ln = (ops & 0xF).astype(np.int64), (ops >> 4).astype(np.int64)
    ql = np.where(np.isin(op, (0, 1, 4, 7, 8)), ln, 0)
    rl = np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0)
    first = np.cumsum(nc) - nc                                               # exclusive prefixes inside each alignment
    qs = np.cumsum(ql) - ql; qs -= np.repeat(qs[first], nc)
    ps = np.cumsum(rl) - rl; ps -= np.repeat(ps[first], nc); ps += reads["pos"].astype(np.int64)[aln]
    L, flag, mapq = reads["l_qseq"].astype(np.int64), reads["flag"].astype(np.int64), reads["mapq"].astype(np.int64)
    cls = 2 * ((flag & 0x80) != 0) + ((flag & 0x10) != 0)
    row = np.zeros(ROW, np.int64)

    def bases_of(sel):                                                       # per base of the selected ops: op index, offset inside the op
        idx = np.repeat(np.flatnonzero(sel), ql[sel])
        off = np.arange(len(idx)) - np.repeat(np.cumsum(ql[sel]) - ql[sel], ql[sel])
        return idx, off

    def cycle(a, q):
        return np.minimum(np.where(flag[a] & 0x10, L[a] - 1 - q, q), 255)
    idx, off = bases_of(np.isin(op, (0, 7, 8)))
    a, q, x = aln[idx], qs[idx] + off, ps[idx] + off - beg
    at = reads["seq_off"].astype(np.int64)[a] + q
    base, qual = reads["bases"][at].astype(np.int64), np.minimum(reads["quals"][at].astype(np.int64), 63)
    ok = (mapq[a] >= min_mapq) & (base < 4)
    D = np.bincount(x[ok], minlength=npos)
    X = np.bincount(x[ok & (base != ref[x])], minlength=npos)
    st = np.where(ref > 3, 0, np.where(D < min_depth, 1, np.where(X * 1000 > permille * D, 2, 3)))
    row[E["UVC_READPROF_COUNTERS"] + 6:E["UVC_READPROF_COUNTERS"] + 10] = np.bincount(st, minlength=4)
    cat = np.where(mapq[a] < min_mapq, 0, np.where(st[x] == 0, 1, np.where(base > 3, 2, st[x] + 2)))
    row[E["UVC_READPROF_COUNTERS"]:E["UVC_READPROF_COUNTERS"] + 6] = np.bincount(cat, minlength=6)
    c = cat == 5
    a, q, x, base, qual = a[c], q[c], x[c], base[c], qual[c]
    k = (base != ref[x]).astype(np.int64)
    row += np.bincount((cls[a] * 64 + qual) * 2 + k, minlength=ROW)
    row += np.bincount(E["UVC_READPROF_CYC_BINS"] + (cls[a] * 256 + cycle(a, q)) * 5 + k, minlength=ROW)
    row += np.bincount(E["UVC_READPROF_SUB_BINS"] + cls[a] * 16 + ref[x] * 4 + base, minlength=ROW)
    for code_, kind in ((1, 2), (4, 4)):                                     # inserted and soft-clipped bases, by their anchor
        idx, off = bases_of(op == code_)
        a, q = aln[idx], qs[idx] + off
        x = np.maximum(reads["pos"].astype(np.int64)[a], ps[idx] - 1) - beg
        ok = (mapq[a] >= min_mapq) & (x >= 0) & (x < npos)
        row += np.bincount(E["UVC_READPROF_CYC_BINS"] + (cls[a[ok]] * 256 + cycle(a[ok], q[ok])) * 5 + kind, minlength=ROW)
    d = np.flatnonzero(op == 2)
    a, x = aln[d], ps[d] - beg
    ok = (mapq[a] >= min_mapq) & (x >= 0) & (x < npos) & (L[a] > 0)
    row += np.bincount(E["UVC_READPROF_CYC_BINS"] + (cls[a[ok]] * 256 + cycle(a[ok], np.maximum(qs[d][ok] - 1, 0))) * 5 + 3, minlength=ROW)
    return row


ap = argparse.ArgumentParser()
ap.add_argument("--tile-kb", type=int, default=1000); ap.add_argument("--depth", type=int, default=300); ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--umi", action="store_true"); ap.add_argument("--baseline-kb", type=int, default=100)
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
fn = lib.dll.uvcgpu_region_read_profile
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()
gate = (0, 20, 50)
req = _ffi.UvcReadProfileRequest(*gate)


def open_tile(kb):
    reads = synth.generate_region(seed=777, region_len=kb * 1000, depth=a.depth, umi=a.umi)
    R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    return reads, R


def time_calls(R, ranges, reps):
    arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])   # built once: the C call alone is timed
    out = np.zeros(ROW, np.int64)
    wall, kern = [], {}
    for rep in range(reps + 3):
        R.accumulate()                                   # starts the handle's list of timed kernels (32 entries) anew
        assert lib.dll.uvcgpu_region_sync(R.h) == 0
        t0 = time.perf_counter()
        assert fn(R.h, arr, len(ranges), C.byref(req), out.ctypes.data) == 0, lib.last_error()
        t1 = time.perf_counter()
        n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
        names = names_buf.value.decode().split(";")
        if rep >= 3:
            wall.append(t1 - t0)
            for i in range(min(n, len(names))):
                if names[i].startswith("k_readprofile_"):
                    kern.setdefault(names[i], []).append(ms_buf[i])
    k_us = {k: round(float(np.median(v)) * 1e3, 1) for k, v in kern.items()}
    return out, dict(kernels_median_us=k_us, kernels_sum_us=round(sum(k_us.values()), 1), call_median_us=round(float(np.median(wall)) * 1e6, 1),
                     call_min_us=round(float(np.min(wall)) * 1e6, 1), call_max_us=round(float(np.max(wall)) * 1e6, 1))


reads, R = open_tile(a.tile_kb)
lib.dll.uvcgpu_region_set_profiling(R.h, 1)
beg, npos = R.beg, R.npos
n_bases, n_ops = len(reads["bases"]), len(reads["cigars"])
floor_bytes = 2 * n_bases + 4 * n_ops + int(npos)
built_bytes = floor_bytes + n_bases + n_bases
print(json.dumps({"what": "byte floor", "positions": int(npos), "read_bases": n_bases, "alignments": int(reads["n_reads"]), "bytes": floor_bytes, "us": round(floor_bytes / 8000e9 * 1e6, 1),
                  "bytes_as_built": built_bytes, "us_as_built": round(built_bytes / 8000e9 * 1e6, 1)}))   # bench.py's HBM_PEAK_GBS
lists = {
    "one whole-tile range": [(beg, beg + npos)],
    "1000 windows": [(beg + k * (npos // 1000), beg + (k + 1) * (npos // 1000)) for k in range(1000)],
    "8000 short ranges": [(beg + k * (npos // 8000), beg + k * (npos // 8000) + min(120, npos // 8000)) for k in range(8000)],
}
for what, ranges in lists.items():
    _, t = time_calls(R, ranges, a.reps)
    print(json.dumps(dict(what="uvcgpu_region_read_profile, " + what, ranges=len(ranges), reps=a.reps, **t)), flush=True)
R.close()

if a.baseline_kb > 0:
    reads, R = open_tile(a.baseline_kb)
    lib.dll.uvcgpu_region_set_profiling(R.h, 1)
    whole = [(R.beg, R.beg + R.npos)]
    got, t = time_calls(R, whole, max(3, a.reps // 4))
    t0 = time.perf_counter(); want = numpy_row(reads, gate); t_np = time.perf_counter() - t0
    assert np.array_equal(got, want), "the two ways disagree: %s" % [(int(i), int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:6]]
    print(json.dumps(dict(what="vectorised numpy over the columns against the call, one whole-tile range of a %d kb tile" % a.baseline_kb, read_bases=len(reads["bases"]),
                          numpy_us=round(t_np * 1e6, 1), call_median_us=t["call_median_us"], ratio=round(t_np * 1e6 / t["call_median_us"], 1))))
    R.close()
