"""Times uvcgpu_region_site_reads on the bench's tile shapes (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE
config 4 shape), DESIGN.md 4p.
    python scripts/gpu_sitereads_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--reps 25] [--only K:A]
Site lists: 100 random sites, 10 000 random sites, the dense bases of 300 exons of 120 bp; each with alt_only 0 and 1.
Figures per list: the two stages alone, from HIP events around their launches on the handle's stream (uvcgpu_region_set_profiling +
uvcgpu_region_kernel_times, entries k_sitereads_count and k_sitereads_write; median and minimum of --reps calls after 3 warm-up calls), and
the synchronous call with room for its rows as a caller sees it (sites upload, count, the wait for the sizes and the counts, write, D2H of
the rows; wall clock; arrays prebuilt).  Beside them the rows returned and a byte floor at the 8 TB/s bench.py uses: per alignment the
columns the kernels read once (pos, endpos, l_qseq, n_cigar: 4 B each; mapq 1 B; seq_off, cigar_off: 8 B each), 4 B per CIGAR op, 2 B per
observation (its packed base | quality) and 32 B per row written.  Each list is checked for what holds without a restatement (a 2 M read
walk in Python is minutes): two calls return the same bytes, the rows ascend by (read, site), and with alt_only 0 the rows of a site
number its six kind counts.  One JSON line per list.  --only K:A runs list K (0, 1, 2) with alt_only A alone: under
rocprofv3 --kernel-trace --stats the process then dispatches the call's kernels for that one shape only (every call of a shape does the
same work, checks and warm-up included), so the statistics of a kernel are its dispatch times for the shape."""
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
ap.add_argument("--umi", action="store_true"); ap.add_argument("--only", default="")
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.correct_bq()
R.accumulate()   # (accumulate starts the list of kernel times anew: the calls below come behind it)
beg, npos = R.beg, R.npos
n_alns, n_ops = int(reads["n_reads"]), int(len(reads["cigars"]))
print(json.dumps({"what": "input", "positions": int(npos), "alignments": n_alns, "cigar_ops": n_ops, "read_bases": int(len(reads["bases"]))}), flush=True)

rng = np.random.default_rng(5)
exon_starts = np.sort(rng.choice(np.arange(beg + 1000, beg + npos - 1000, 200), 300, replace=False))
lists = {
    "100 random sites": np.sort(rng.choice(np.arange(beg, beg + npos), 100, replace=False)),
    "10000 random sites": np.sort(rng.choice(np.arange(beg, beg + npos), 10000, replace=False)),
    "300 exons of 120 bp, every base": (exon_starts[:, None] + np.arange(120)[None, :]).ravel(),
}
fn = lib.dll.uvcgpu_region_site_reads
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()


def kernel_ms(name):
    n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    return [ms_buf[i] for i in range(n) if i < len(names) and names[i] == name]


def us(v):
    return {"median": round(float(np.median(v)) * 1e6, 1), "min": round(float(np.min(v)) * 1e6, 1), "max": round(float(np.max(v)) * 1e6, 1)} if len(v) else None


lib.dll.uvcgpu_region_set_profiling(R.h, 1)
only = tuple(int(v) for v in a.only.split(":")) if a.only else None
for k_list, (what, sites) in enumerate(lists.items()):
    sites = np.ascontiguousarray(sites, np.int32)
    for alt_only in (0, 1):
        if only is not None and only != (k_list, alt_only):
            continue
        req = _ffi.UvcSiteReadsRequest(0, alt_only)
        rows, counts = R.site_reads(sites, 0, alt_only)
        rows2, counts2 = R.site_reads(sites, 0, alt_only)
        assert rows.tobytes() == rows2.tobytes() and counts.tobytes() == counts2.tobytes(), what
        assert (np.diff(rows["read"].astype(np.int64) * (1 << 31) + rows["site"]) > 0).all(), what
        if not alt_only:
            assert np.array_equal(np.bincount(rows["site"], minlength=len(sites)), counts[:, :6].sum(1)), what
        n_obs, n = int(counts[:, :6].sum()), len(rows)
        buf, cnt, n_rows = np.zeros(max(n, 1), region.SITE_READ), np.zeros((len(sites), 8), np.int32), C.c_int64(0)
        wall, k_count, k_write = [], [], []
        for rep in range(a.reps + 3):
            R.accumulate()                                   # starts the handle's list of timed kernels (32 entries) anew
            assert lib.dll.uvcgpu_region_sync(R.h) == 0      # accumulate returns before its kernels end: the call below would wait for them
            t0 = time.perf_counter()
            assert fn(R.h, sites.ctypes.data, len(sites), C.byref(req), cnt.ctypes.data, buf.ctypes.data, n, C.byref(n_rows)) == 0
            t1 = time.perf_counter()
            if rep >= 3:
                wall.append(t1 - t0); k_count += [v * 1e-3 for v in kernel_ms("k_sitereads_count")[-1:]]; k_write += [v * 1e-3 for v in kernel_ms("k_sitereads_write")[-1:]]
        assert n_rows.value == n and buf[:n].tobytes() == rows.tobytes()
        floor_bytes = n_alns * (4 * 4 + 1 + 2 * 8) + 4 * n_ops + 2 * n_obs + 32 * n
        print(json.dumps({"what": "uvcgpu_region_site_reads, " + what, "alt_only": alt_only, "sites": len(sites), "reps": a.reps, "observations": n_obs, "rows": n,
                          "count_stage_us": us(k_count), "write_stage_us": us(k_write), "call_us": us(wall), "floor_bytes": floor_bytes, "floor_us_at_8TBps": round(floor_bytes / 8e12 * 1e6, 2)}), flush=True)
R.close()
