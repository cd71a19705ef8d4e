"""Times uvcgpu_region_clip_mates on the tile shapes the clip-site call was measured on (1 Mb x 300x, non-UMI; --umi --tile-kb 200
--depth 2000: the BASELINE config 4 shape), DESIGN.md 4s.
    python scripts/gpu_clipmates_bench.py [--tile-kb 1000] [--depth 300] [--umi] [--clip-frac 0.05] [--share 0.02] [--reps 25] [--hot 1000,2000,4000,8000]
The synthetic reads are all concordant pairs.  A seeded share of the alignments (--share, 2 %) is made discordant, a third each: the mate
on another contig at a position below 50 000, the mate on the read's own strand, the mate 100 kb away.  One hot site is added in the middle
of the tile: every forward pair read that faces it gets its mate on a third contig inside 300 bp, so the site's witnesses number what the
depth gives (reported as largest_site).  The site rows are those Region.clip_sites returns over the whole tile at min_clip 10, min_mapq 0
and min_reads 3, plus the hot site; the request is the command line's default one (window 500, overhang 5, min_dist 1000, max_gap 500,
min_pairs 2), with the witness rows.
Figures: the five stages alone, from HIP events around their launches on the handle's stream (uvcgpu_region_set_profiling +
uvcgpu_region_kernel_times, entries k_clipmates_count / _scatter / _rank / _cut / _reduce; median, minimum and maximum of --reps calls
after 3 warm-up calls) and the synchronous call as a caller sees it (uploads, the stages, three waits, D2H of the rows; wall clock; arrays
prebuilt).  Beside them the bytes the two passes over the alignments read (23 B per alignment each) with their time at 8 TB/s, and the
sum over the sites of the squared witness counts, which the rank stage's work is proportional to.
Then, on a small handle of its own, one site with --hot witnesses each: the rank stage against the square of the site size.
Each list is checked for what holds without a restatement: two calls return the same bytes, the totals add up.  One JSON line per list."""
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
ap.add_argument("--umi", action="store_true"); ap.add_argument("--clip-frac", type=float, default=0.05); ap.add_argument("--share", type=float, default=0.02)
ap.add_argument("--hot", default="1000,2000,4000,8000")
a = ap.parse_args()

STAGES = ["k_clipmates_count", "k_clipmates_scatter", "k_clipmates_rank", "k_clipmates_cut", "k_clipmates_reduce"]
E = _ffi.ENUMS
SROW, CROW, CSROW = E["UVC_CLIPMATE_SITE_ROW"], E["UVC_CLIPMATE_ROW"], E["UVC_CLIPSITE_ROW"]
SW = {n: f for n, f, _ in _ffi.CLIPMATE_SITE_WORDS}
CW = {n: f for n, f, _ in _ffi.CLIPMATE_CLUSTER_WORDS}
CSW = {n: f for n, f, _ in _ffi.CLIPSITE_SECTIONS}
REQ = dict(min_mapq=0, window=500, overhang=5, min_dist=1000, max_gap=500, min_pairs=2)
lib = region.gpu_lib()
assert lib.dll.uvcgpu_init(0) == 0, lib.last_error()
lib.dll.uvcgpu_region_set_profiling.argtypes = [C.c_void_p, C.c_int]
lib.dll.uvcgpu_region_sync.argtypes = [C.c_void_p]
lib.dll.uvcgpu_region_kernel_times.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.c_int]
fn = lib.dll.uvcgpu_region_clip_mates
fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
names_buf, ms_buf = C.create_string_buffer(4096), (C.c_float * 64)()


def kernel_ms(R):
    k = lib.dll.uvcgpu_region_kernel_times(R.h, names_buf, 4096, ms_buf, 64)
    names = names_buf.value.decode().split(";")
    return [(names[i], ms_buf[i]) for i in range(k) if i < len(names)]


def us(v):
    return {"median": round(float(np.median(v)) * 1e6, 1), "min": round(float(np.min(v)) * 1e6, 1), "max": round(float(np.max(v)) * 1e6, 1)} if len(v) else None


def ref_ends(reads):
    """pos + the reference length of every alignment's CIGAR"""
    cig = np.asarray(reads["cigars"]).astype(np.int64)
    op, ln = cig & 0xF, cig >> 4
    step = np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0)
    cum = np.concatenate([[0], np.cumsum(step)])
    co, nc = np.asarray(reads["cigar_off"]).astype(np.int64), np.asarray(reads["n_cigar"]).astype(np.int64)
    return np.asarray(reads["pos"]).astype(np.int64) + cum[co + nc] - cum[co]


def site_row(pos, side):
    row = np.zeros(CSROW, np.int64)
    row[CSW["pos"]], row[CSW["side"]] = pos, side
    return row


def measure(what, R, reads, rows, mtid, tid, reps):
    """reps timed calls after 3 warm-up calls -> one JSON line"""
    ns = len(rows)
    req = _ffi.UvcClipMatesRequest(tid, REQ["min_mapq"], REQ["window"], REQ["overhang"], REQ["min_dist"], REQ["max_gap"], REQ["min_pairs"], 1)
    totals, srows = np.zeros(8, np.int64), np.zeros((max(ns, 1), SROW), np.int64)
    nc, nr = C.c_int64(0), C.c_int64(0)
    head = (R.h, rows.ctypes.data, ns, mtid.ctypes.data, C.byref(req), totals.ctypes.data, srows.ctypes.data)
    rc = fn(*head, None, 0, C.byref(nc), None, 0, C.byref(nr))
    assert rc in (0, E["UVCGPU_ENOMEM"]), lib.last_error()
    out, wit = np.zeros((max(nc.value, 1), CROW), np.int64), np.zeros((max(nr.value, 1), 4), np.int32)
    wall, stage, want = [], {s: [] for s in STAGES}, None
    for rep in range(reps + 3):
        lib.dll.uvcgpu_region_set_profiling(R.h, 1)          # starts the handle's list of timed kernels (32 entries) anew; the call is legal without an accumulate
        t0 = time.perf_counter()
        assert fn(*head, out.ctypes.data, len(out), C.byref(nc), wit.ctypes.data, len(wit), C.byref(nr)) == 0, lib.last_error()
        t1 = time.perf_counter()
        got = (totals.tobytes(), srows.tobytes(), out.tobytes(), wit.tobytes())
        if want is None:
            want = got                                       # two calls: the same bytes
        assert got == want, (what, rep)
        if rep >= 3:
            wall.append(t1 - t0)
            last = dict(kernel_ms(R)[-len(STAGES):])
            for s in STAGES:
                if s in last:
                    stage[s].append(last[s] * 1e-3)
    sr, cl = srows[:ns], out[:nc.value]
    per_site = sr[:, SW["other_contig"]] + sr[:, SW["same_strand"]] + sr[:, SW["far"]]
    assert totals[1] == sr[:, SW["facing"]].sum() and totals[2] == sr[:, SW["concordant"]].sum() and totals[3] == per_site.sum() == nr.value and totals[1] == totals[2] + totals[3]
    assert totals[4] == sr[:, SW["clusters"]].sum() and totals[5] == sr[:, SW["clusters_kept"]].sum() == nc.value and totals[6] == (sr[:, SW["clusters_kept"]] > 0).sum()
    n_alns = int(reads["n_reads"])
    pass_bytes = 2 * 23 * n_alns
    sq = int((per_site.astype(np.int64) ** 2).sum())
    rank = float(np.median(stage["k_clipmates_rank"])) if stage["k_clipmates_rank"] else 0.0
    print(json.dumps({"what": what, "reps": reps, "alignments": n_alns, "sites": ns, "totals": totals[:7].tolist(), "witnesses": int(nr.value), "largest_site": int(per_site.max()) if ns else 0,
                      "largest_cluster": int(cl[:, CW["pairs"]].max()) if len(cl) else 0, "sum_of_squared_site_sizes": sq,
                      "count_stage_us": us(stage["k_clipmates_count"]), "scatter_stage_us": us(stage["k_clipmates_scatter"]), "rank_stage_us": us(stage["k_clipmates_rank"]),
                      "cut_stage_us": us(stage["k_clipmates_cut"]), "reduce_stage_us": us(stage["k_clipmates_reduce"]), "call_us": us(wall),
                      "bytes_read_by_the_two_passes": pass_bytes, "their_floor_us_at_8TBps": round(pass_bytes / 8e12 * 1e6, 2),
                      "rank_pair_compares_per_s": round(sq / rank, 1) if rank > 0 else None}), flush=True)


# ---- the tile
reads = synth.generate_region(seed=777, region_len=a.tile_kb * 1000, depth=a.depth, umi=a.umi, clip_frac=a.clip_frac)
n, tid = int(reads["n_reads"]), int(reads["tid"])
rng = np.random.default_rng(12345)
mtid = np.full(n, tid, np.int32)
flag, mpos, pos = reads["flag"].copy(), reads["mpos"].astype(np.int64), reads["pos"].astype(np.int64)
pick = rng.random(n) < a.share
kind = rng.integers(0, 3, n)
other, same, far = pick & (kind == 0), pick & (kind == 1), pick & (kind == 2)
mtid[other] = tid + 1
mpos[other] = rng.integers(0, 50_000, int(other.sum()))
flag[same] = (flag[same] & ~np.uint16(0x20)) | ((flag[same] & 0x10) << 1).astype(np.uint16)
mpos[far] = pos[far] + 100_000
hot = int(reads["beg"]) + a.tile_kb * 500
rend = ref_ends(reads)
facing = ((flag & 0x10) == 0) & (pos < hot) & (rend > hot - REQ["window"]) & (rend <= hot + REQ["overhang"])
mtid[facing] = tid + 2
mpos[facing] = 7_000 + rng.integers(0, 300, int(facing.sum()))
reads = dict(reads, flag=flag, mpos=mpos.astype(np.int32))
R = region.Region(lib, region.default_params(lib), tid, reads["beg"], reads["end"], reads["refseq"])
R.set_reads(reads)
lib.dll.uvcgpu_region_set_profiling(R.h, 1)
rows = R.clip_sites([(R.beg, R.beg + R.npos)], 0, 10, 3)[1]
keys = [(int(r[CSW["pos"]]), int(r[CSW["side"]])) for r in rows]
if (hot, 1) not in keys:
    at = int(np.searchsorted(np.array([k[0] * 2 + k[1] for k in keys], np.int64), hot * 2 + 1))
    rows = np.concatenate([rows[:at], site_row(hot, 1)[None], rows[at:]])
rows = np.ascontiguousarray(rows)
print(json.dumps({"what": "input", "positions": int(R.npos), "alignments": n, "clip_frac": a.clip_frac, "discordant_share": a.share, "made_discordant": int(pick.sum()), "hot_site_reads": int(facing.sum())}), flush=True)
measure("uvcgpu_region_clip_mates on the rows of clip_sites over the tile and one hot site", R, reads, rows, mtid, tid, a.reps)
R.close()

# ---- one site of a given size on a small handle: the rank stage against the square of the site size
for size in [int(v) for v in a.hot.split(",") if v]:
    beg, ref_len, p = 1_000_000, 2000, 1_001_000
    rng = np.random.default_rng(size)
    small = dict(n_reads=size, tid=0, beg=beg, end=beg + ref_len, refseq="".join("ACGT"[i] for i in rng.integers(0, 4, ref_len)), n_fams=size, fam_dflag=np.zeros(size, np.uint8),
                 pos=(p - 60 - rng.integers(0, 40, size)).astype(np.int32), mpos=rng.integers(0, 3000, size).astype(np.int32), isize=np.zeros(size, np.int32), flag=np.full(size, 0x61, np.uint16),
                 mapq=np.full(size, 60, np.uint8), nm=np.zeros(size, np.int32), l_qseq=np.full(size, 50, np.int32), seq_off=np.arange(size, dtype=np.int64) * 50, cigar_off=np.arange(size, dtype=np.int64),
                 n_cigar=np.ones(size, np.int32), frag_id=np.arange(size, dtype=np.int32), fam_id=np.arange(size, dtype=np.int32), fam_strand=np.zeros(size, np.uint8),
                 bases=np.zeros(size * 50, np.uint8), quals=np.full(size * 50, 30, np.uint8), cigars=np.full(size, 50 << 4, np.uint32))
    order = np.argsort(small["pos"], kind="stable")
    for k in ("pos", "mpos"):
        small[k] = small[k][order]
    S = region.Region(lib, region.default_params(lib), 0, small["beg"], small["end"], small["refseq"])
    S.set_reads(small)
    measure("one site of %d witnesses" % size, S, small, np.ascontiguousarray(site_row(p, 1)[None]), np.full(size, 1, np.int32), 0, a.reps)
    S.close()
