"""Times uvcgpu_region_clip_sites on the bench's tile shapes (1 Mb x 300x, non-UMI; --umi --tile-kb 200 --depth 2000: the BASELINE
config 4 shape), DESIGN.md 4q.
    python scripts/gpu_clipsites_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--clip-frac 0.05] [--reps 25] [--hot]
--hot plants one breakpoint: every plain alignment that crosses the tile's middle within its last 40 bases is clipped there with one string,
so one row takes a depth's worth of events (the shape the wave pre-merge of k_cs_fill is for).
One range over the whole tile, min_clip 10, min_mapq 0, gates min_reads 1 and 3, each with and without the event rows.
Figures per gate: the two stages alone, from HIP events around their launches on the handle's stream (uvcgpu_region_set_profiling +
uvcgpu_region_kernel_times, entries k_clipsites_find and k_clipsites_fill; median, minimum and maximum of --reps calls after 3 warm-up
calls), and the synchronous call with room for its rows as a caller sees it (range upload, find, the wait for the sizes, fill, D2H of the
rows; wall clock; arrays prebuilt).  Beside them the sites and event rows returned and a byte floor at the 8 TB/s bench.py uses: per
alignment the columns a pass reads (pos, l_qseq, n_cigar: 4 B each; flag 2 B; mapq 1 B; cigar_off 8 B) and 4 B per CIGAR op, twice (the
find and the fill pass), plus 1 408 B per site row and 16 B per event row written.  Each gate is checked for what holds without a
restatement (a 2 M read walk in Python is minutes): two calls return the same bytes, the sites ascend by (pos, side), the event rows by
(read, side of their site), a site's `reads` is the number of its event rows and at least min_reads, and the totals add up.  One JSON
line per gate."""
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
ap.add_argument("--umi", action="store_true"); ap.add_argument("--clip-frac", type=float, default=0.05); ap.add_argument("--hot", action="store_true")
a = ap.parse_args()

lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi, clip_frac=a.clip_frac)
if a.hot:   # a real breakpoint: every alignment that ends inside the 40 positions in front of the tile's middle is clipped there, 40 bases of one string
    L, mid, rng = 150, int(reads["beg"]) + a.tile_kb * 500, np.random.default_rng(1)
    s = rng.integers(0, 4, 40).astype(np.uint8)
    plain = (reads["n_cigar"] == 1) & (reads["pos"] + L > mid) & (reads["pos"] + L <= mid + 40)
    assert (reads["cigar_off"] == np.concatenate([[0], np.cumsum(reads["n_cigar"][:-1])])).all()
    cig = []
    for i in range(int(reads["n_reads"])):
        co, nc = int(reads["cigar_off"][i]), int(reads["n_cigar"][i])
        if plain[i]:
            m = mid - int(reads["pos"][i])
            cig += [(m << 4) | 0, ((L - m) << 4) | 4]
            reads["bases"][i * L + m:(i + 1) * L] = s[:L - m]
        else:
            cig += list(reads["cigars"][co:co + nc])
    reads["n_cigar"] = np.where(plain, 2, reads["n_cigar"]).astype(np.int32)
    reads["cigar_off"] = np.concatenate([[0], np.cumsum(reads["n_cigar"][:-1])]).astype(np.int64)
    reads["cigars"] = np.array(cig, np.uint32)
R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
R.accumulate()   # (accumulate starts the list of kernel times anew: the calls below come behind it)
beg, npos = R.beg, R.npos
n_alns, n_ops = int(reads["n_reads"]), int(len(reads["cigars"]))
print(json.dumps({"what": "input", "positions": int(npos), "alignments": n_alns, "cigar_ops": n_ops, "read_bases": int(len(reads["bases"])), "clip_frac": a.clip_frac}), flush=True)

fn = lib.dll.uvcgpu_region_clip_sites
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()
ROW = _ffi.ENUMS["UVC_CLIPSITE_ROW"]


def kernel_ms(name):
    n = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    return [ms_buf[i] for i in range(n) if i < len(names) and names[i] == name]


def us(v):
    return {"median": round(float(np.median(v)) * 1e6, 1), "min": round(float(np.min(v)) * 1e6, 1), "max": round(float(np.max(v)) * 1e6, 1)} if len(v) else None


lib.dll.uvcgpu_region_set_profiling(R.h, 1)
whole = [(beg, beg + npos)]
arr, pairs = region._coverage_ranges(whole)
for min_reads in (1, 3):
    totals, rows, ev = R.clip_sites(whole, 0, 10, min_reads, want_reads=True)
    t2, rows2, ev2 = R.clip_sites(whole, 0, 10, min_reads, want_reads=True)
    assert totals.tobytes() == t2.tobytes() and rows.tobytes() == rows2.tobytes() and ev.tobytes() == ev2.tobytes()
    ns, nr = len(rows), len(ev)
    assert (np.diff(rows[:, 1] * 2 + rows[:, 2]) > 0).all() and (rows[:, 3] >= min_reads).all()
    assert np.array_equal(np.bincount(ev["site"], minlength=ns), rows[:, 3]) and totals[4] == nr == rows[:, 3].sum() and totals[1] >= totals[4]
    assert (np.diff(ev["read"].astype(np.int64) * 2 + rows[ev["site"], 2]) > 0).all()
    assert np.array_equal(rows[:, 16:].reshape(ns, 32, 5).sum(2)[:, 0], rows[:, 3] - np.bincount(ev["site"], weights=ev["soft_len"] == 0, minlength=ns).astype(np.int64))   # every event with a soft-clipped base votes at k = 0
    for want_reads in (1, 0):
        req = _ffi.UvcClipSitesRequest(0, 10, min_reads, want_reads)
        tot, buf, evb, n_s, n_r = np.zeros(8, np.int64), np.zeros((max(ns, 1), ROW), np.int64), np.zeros(max(nr, 1), region.CLIP_READ), C.c_int64(0), C.c_int64(0)
        wall, k_find, k_fill = [], [], []
        for rep in range(a.reps + 3):
            R.accumulate()                                   # starts the handle's list of timed kernels (32 entries) anew
            assert lib.dll.uvcgpu_region_sync(R.h) == 0      # accumulate returns before its kernels end: the call below would wait for them
            t0 = time.perf_counter()
            assert fn(R.h, arr, len(pairs), C.byref(req), tot.ctypes.data, buf.ctypes.data, ns, C.byref(n_s), evb.ctypes.data if want_reads else None, nr if want_reads else 0, C.byref(n_r)) == 0
            t1 = time.perf_counter()
            if rep >= 3:
                wall.append(t1 - t0); k_find += [v * 1e-3 for v in kernel_ms("k_clipsites_find")[-1:]]; k_fill += [v * 1e-3 for v in kernel_ms("k_clipsites_fill")[-1:]]
        assert n_s.value == ns and n_r.value == nr and buf[:ns].tobytes() == rows.tobytes() and (not want_reads or evb[:nr].tobytes() == ev.tobytes())
        floor_bytes = 2 * (n_alns * (3 * 4 + 2 + 1 + 8) + 4 * n_ops) + 8 * ROW * ns + (16 * nr if want_reads else 0)
        print(json.dumps({"what": "uvcgpu_region_clip_sites, one range over the tile", "min_clip": 10, "min_reads": min_reads, "want_reads": want_reads, "reps": a.reps, "totals": totals[:5].tolist(), "sites": ns,
                          "event_rows": nr, "hottest_site_reads": int(rows[:, 3].max()) if ns else 0, "find_stage_us": us(k_find), "fill_stage_us": us(k_fill), "call_us": us(wall), "floor_bytes": floor_bytes,
                          "floor_us_at_8TBps": round(floor_bytes / 8e12 * 1e6, 2)}), flush=True)
R.close()
