#!/usr/bin/env python3
"""GPU-box helper: one -A tile scored by one call and as a stream (uvcgpu_region_score_stream_*), on one accumulated handle.
    python scripts/gpu_score_stream.py --kb 200 [--parent-lib other/libuvcgpu.so] [--chunks 8] [--reps 7]
    python scripts/gpu_score_stream.py --kb 1000 --mem-mb 2048 --no-one-call
The tile is the one bench.py --full gives its all-out leg (seed 5000, 300x).  Per repetition the legs alternate: the parent library's one
call (if given: another build of the same ABI, bound next to this one), this library's one call, this library's stream.  One line per leg
and repetition: ms of the score (records on the host in page-locked memory, nothing formatted), records, chunks, the scoring footprint
(uvcgpu_score_stream_footprint) and the lowest free device memory seen (uvcgpu_device_memory), then the medians."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uvc_amd import _ffi, region, synth   # noqa: E402


def free_bytes(lib):
    f, t = C.c_int64(0), C.c_int64(0)
    lib.dll.uvcgpu_device_memory.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert lib.dll.uvcgpu_device_memory(C.byref(f), C.byref(t)) == 0
    return f.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kb", type=int, default=200)
    ap.add_argument("--depth", type=int, default=300)
    ap.add_argument("--chunks", type=int, default=8, help="chunk_records = records / chunks (at least this many chunks)")
    ap.add_argument("--mem-mb", type=int, default=0, help="instead of --chunks: chunk_records = MiB / bytes_per_record, as uvc1-mi355x --score-mem-mb")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-one-call", action="store_true", help="the stream alone (a tile whose one-call buffers are not wanted)")
    a = ap.parse_args()
    libs = [("this", region.gpu_lib())]
    if a.parent_lib:
        libs.insert(0, ("parent", _ffi.Lib(a.parent_lib, "uvcgpu_")))
    for _, lib in libs:
        assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
    t0 = time.perf_counter()
    reads = synth.generate_region(seed=5000, region_len=a.kb * 1000, depth=a.depth, beg=1000000, umi=False)
    print("# tile: %d positions, %d reads, generated in %.1f s" % (reads["end"] - reads["beg"], reads["n_reads"], time.perf_counter() - t0), flush=True)
    base_free = free_bytes(libs[-1][1])
    R = {}
    for name, lib in libs:
        R[name] = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        R[name].set_reads(reads)
        R[name].accumulate()
    this = R["this"]
    bpr = this.score_stream_bytes_per_record()
    npos = reads["end"] - reads["beg"]
    n_upper = 14 * (npos + 1)
    chunk_records = (a.mem_mb << 20) // bpr if a.mem_mb else None
    ms = {}
    low = {}

    def note(leg, dt, n, chunks, lib):
        ms.setdefault(leg, []).append(dt * 1e3)
        low[leg] = min(low.get(leg, 1 << 62), free_bytes(lib))
        print("%-14s %9.2f ms  records %d  chunks %d  footprint %.1f MB  device memory in use %.2f GB" % (leg, dt * 1e3, n, chunks, this.score_stream_footprint() / 1e6, (base_free - low[leg]) / 1e9), flush=True)
    for rep in range(a.reps):
        if not a.no_one_call:
            for name, lib in libs:
                t = time.perf_counter()
                rec = R[name].score(all_out=True, capacity=n_upper, copy=False)
                note(name + " one call", time.perf_counter() - t, len(rec["refpos"]), 1, lib)
                n_rec = len(rec["refpos"])
        else:
            n_rec = n_upper
        c = chunk_records if chunk_records else -(-n_rec // a.chunks)
        t = time.perf_counter()
        n = k = 0
        for rec, cov in this.score_stream(c, all_out=True, copy=False):
            n += len(rec["refpos"]); k += 1
            if k == 2:
                low["this stream"] = min(low.get("this stream", 1 << 62), free_bytes(libs[-1][1]))
        note("this stream", time.perf_counter() - t, n, k, libs[-1][1])
    rec_b = 4 * _ffi.NUM_SCORE_FIELDS
    rows = bpr // 2 - 3 * rec_b                                             # device rows of one set per record
    print("# bytes per unit of chunk_records %d (rows %d + records %d + kept copy %d + host buffer %d, twice); chunk_records %d" % (bpr, rows, rec_b, rec_b, rec_b, c))
    grp_rows = 692                                                          # of `rows`: the rows per group, of which a call holds min(2 x positions, capacity)
    print("# one call for %d records by the layout formulas: %.2f GB on the device (rows with 12.5 %% slack + records), %.2f GB of host buffer; the stream: %.2f GB in all"
          % (n_rec, (((rows - grp_rows) * n_upper + grp_rows * min(2 * npos, n_upper)) * 1.125 + n_upper * rec_b) / 1e9, n_upper * rec_b / 1e9, c * bpr / 1e9))
    for leg, v in ms.items():
        print("# %-14s median %.2f ms  min %.2f  max %.2f  (n = %d)" % (leg, statistics.median(v), min(v), max(v), len(v)))
    for q in R.values():
        q.close()


if __name__ == "__main__":
    main()
