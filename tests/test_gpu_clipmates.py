"""The clip-site mates of the HIP library (uvcgpu_region_clip_mates, Region.clip_mates) and the P and M lines built from them
(uvc1-mi355x --clip-sites-mates 1).  Every number is an integer and is compared for equality with the restatement of the definitions
(tests/clipmates_restatement.py).  Sites are crafted directly (the call reads pos and side of a row) on regions of a few kb:
  * 0..257 alignments and 0..257 sites; every edge of the facing rules, of min_dist, max_gap and min_pairs;
  * one site with 255, 256, 257 and 600 witnesses that share (mt, strand, mpos), so that the read index breaks the ties: the LDS tile edge
    and more than one block per site of the rank kernel; the same witnesses in two alignment orders;
  * mtid NULL, mt 0 and 2^20, two sites 3 bp apart that share all their witnesses;
  * every refusal by its message with nothing written, sizes first, the legality window, two calls returning the same bytes;
  * one chain of synthetic reads with a planted translocation through clip_sites and clip_mates;
  * the report of the command line on a two-contig BAM against the Python chain and the restatement text."""
import ctypes as C
import os

import numpy as np
import pytest

import bamwriter
import clipmates_restatement as cm
import clipsites_restatement as cr
import test_clipmates_cpu as cpu
from test_gpu_coverage import run_cli
from test_gpu_readprofile import open_region
from uvc_amd import _ffi, io as uio, pipeline, region

pytestmark = pytest.mark.gpu

EXE = cpu.EXE
EINVAL, ENOMEM = _ffi.ENUMS["UVCGPU_EINVAL"], _ffi.ENUMS["UVCGPU_ENOMEM"]
BEG, TID, FWD, REV = cpu.BEG, cpu.TID, cpu.FWD, cpu.REV
LEFT, RIGHT = cm.LEFT, cm.RIGHT
REQ = dict(min_mapq=0, window=100, overhang=5, min_dist=1000, max_gap=50, min_pairs=2)


def check(R, reads, rows, mtid, what="", **req):
    """Region.clip_mates against the restatement -> (totals, site rows, cluster rows, witness rows) of the restatement"""
    want = cm.run(reads, rows, mtid, TID, **req)
    totals, sr, cl, wit = R.clip_mates(rows, mtid, TID, **req)
    got_wit = np.stack([wit[n] for n in ("site", "read", "cluster", "klass")], 1).astype(np.int64) if len(wit) else np.zeros((0, 4), np.int64)
    for name, g, w in (("totals", totals, want[0]), ("site rows", sr, want[1]), ("clusters", cl, want[2]), ("witnesses", got_wit, want[3])):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, req, [(tuple(int(v) for v in ij), int(g[tuple(ij)]), int(w[tuple(ij)])) for ij in np.argwhere(g != w)[:8]])
    t2, sr2, cl2, none = R.clip_mates(rows, mtid, TID, want_reads=False, **req)
    assert none is None and t2.tobytes() == totals.tobytes() and sr2.tobytes() == sr.tobytes() and cl2.tobytes() == cl.tobytes(), what
    return want


def mixed(n, seed, n_sites=6, ref_len=cpu.REF_LEN):
    """n pair reads of every kind around n_sites sites of both sides"""
    rng = np.random.default_rng(seed)
    sites = sorted({(BEG + int(x), int(s)) for x, s in zip(rng.integers(200, ref_len - 200, n_sites * 2), rng.integers(0, 2, n_sites * 2))})[:n_sites]
    specs = []
    for i in range(n):
        p, side = sites[int(rng.integers(0, len(sites)))] if sites else (BEG + 1000, RIGHT)
        ln = 50
        off = (p - BEG) - ln - int(rng.integers(-8, 110)) if side == RIGHT else (p - BEG) + int(rng.integers(-8, 110))
        flag = (FWD if side == RIGHT else REV) ^ (0x20 if rng.random() < 0.2 else 0) | (0x800 if rng.random() < 0.05 else 0) | (0x8 if rng.random() < 0.05 else 0)
        if rng.random() < 0.05:
            flag &= ~0x1
        mt = [TID, TID, 5, 9, -1][int(rng.integers(0, 5))]
        mpos = BEG + off + int(rng.integers(-1200, 1200)) if mt == TID else int(rng.integers(0, 400))
        specs.append((max(off, 0), flag, ln, mpos, mt, int(rng.integers(0, 61))))
    reads, mtid = cpu.pair_reads(specs, ref_len) if n else (None, None)
    return reads, mtid, cpu.site_rows(sites)[0]


def no_reads(reads):
    none = dict(reads, n_reads=0, n_fams=0)
    for k in ("pos", "mpos", "isize", "flag", "mapq", "nm", "l_qseq", "seq_off", "cigar_off", "n_cigar", "frag_id", "fam_id", "fam_strand", "bases", "quals", "cigars", "fam_dflag"):
        none[k] = reads[k][:0]
    return none


# ------------------------------------------------------------------------------------------------ shapes
def test_the_hand_written_set(gpu_lib):
    reads, mtid, rows = cpu.hand_made()
    R = open_region(gpu_lib, reads)
    want = check(R, reads, rows, mtid, "hand", **cpu.HAND_REQ)
    assert want[0].tolist() == [10, 11, 1, 10, 5, 4, 2, 0]
    check(R, reads, rows, mtid, "hand, joined", **dict(cpu.HAND_REQ, max_gap=51, min_pairs=1))
    check(R, reads, rows, None, "hand, mtid NULL", **cpu.HAND_REQ)
    R.close()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_alignment_counts_around_a_block_step(n, gpu_lib):
    reads, mtid, rows = mixed(max(n, 1), 100 + n)
    if n == 0:
        reads, mtid = no_reads(reads), mtid[:0]
    R = open_region(gpu_lib, reads)
    for req in (dict(REQ, min_mapq=30, min_pairs=1), dict(REQ, window=30, overhang=0, max_gap=0), REQ):
        want = check(R, reads, rows, mtid, n, **req)
    assert n < 255 or (want[0][1] > 50 and want[0][3] > 20 and want[0][4] > 5), want[0].tolist()
    assert n > 0 or (not want[0].any() and want[1][:, 0].tolist() == list(range(len(rows))))
    R.close()


@pytest.mark.parametrize("n_sites", [0, 1, 64, 65, 257])
def test_site_counts(n_sites, gpu_lib):
    reads, mtid, rows = mixed(400, 7 + n_sites, n_sites)
    assert len(rows) == n_sites
    R = open_region(gpu_lib, reads)
    want = check(R, reads, rows, mtid, n_sites, **dict(REQ, min_pairs=1))
    assert n_sites == 0 or want[0][1] > 100
    assert n_sites > 0 or not want[0].any()
    R.close()


def test_the_edges_of_the_facing_rules_of_min_dist_and_of_max_gap(gpu_lib):
    p, q, w, o = BEG + 1000, BEG + 2000, REQ["window"], REQ["overhang"]
    specs = []
    for rend, faces in ((p - w, 0), (p - w + 1, 1), (p + o, 1), (p + o + 1, 0)):                 # a RIGHT site: p - window < rend <= p + overhang
        specs.append((rend - 50 - BEG, FWD, 50, 100, 7))
    specs.append((p - BEG, FWD, 5, 100, 7))                                                     # pos < p fails: pos = p
    specs.append((p - 1 - BEG, FWD, 5, 100, 7))                                                 # pos = p - 1
    for pos, faces in ((q - o - 1, 0), (q - o, 1), (q + w - 1, 1), (q + w, 0)):                 # a LEFT site: p - overhang <= pos < p + window
        specs.append((pos - BEG, REV, 50, 100, 7))
    specs.append((q - o - BEG, REV, o, 100, 7))                                                 # rend > p fails: rend = q
    specs.append((q - o - BEG, REV, o + 1, 100, 7))                                             # rend = q + 1
    # on the wrong strand for their site
    specs += [(p - 60 - BEG, REV, 50, 100, 7), (q + 10 - BEG, FWD, 50, 100, 7)]
    # min_dist at |mpos - pos| = min_dist - 1 and min_dist, on either side of pos
    d = REQ["min_dist"]
    for delta in (d - 1, d, -(d - 1), -d):
        specs.append((p - 60 - BEG, FWD, 50, p - 60 + delta, TID))
    reads, mtid = cpu.pair_reads(specs)
    rows, _ = cpu.site_rows([(p, RIGHT), (q, LEFT)])
    R = open_region(gpu_lib, reads)
    _, sr, cl, wit = check(R, reads, rows, mtid, "edges", **dict(REQ, min_pairs=1))
    assert sr[0].tolist()[1:6] == [3 + 4, 2, 3, 0, 2] and sr[1].tolist()[1:6] == [3, 0, 3, 0, 0]
    assert sorted(int(a) for s, a, c, k in wit if s == 0 and k == cm.OTHER_CONTIG) == [1, 2, 5] and sorted(int(a) for s, a, c, k in wit if s == 1) == [7, 8, 11]
    assert sorted(int(a) for s, a, c, k in wit if k == cm.FAR) == [15, 17]
    # gaps of max_gap and max_gap + 1, and min_pairs 1, 2 and 3 on clusters of 1 and 2
    g = REQ["max_gap"]
    specs = [(p - 60 - BEG, FWD, 50, m, 7) for m in (1000, 1000 + g, 1000 + 2 * g + 1, 5000, 9000, 9000)]
    reads, mtid = cpu.pair_reads(specs)
    R.reset(TID, BEG, BEG + cpu.REF_LEN, reads["refseq"])
    R.set_reads(reads)
    for mp, n_kept in ((1, 4), (2, 2), (3, 0)):
        _, sr, cl, _ = check(R, reads, rows[:1], mtid, "gaps", **dict(REQ, min_pairs=mp))
        assert sr[0].tolist() == [0, 6, 0, 6, 0, 0, 4, n_kept] and (mp > 1 or cl[:, cm.CW["pairs"]].tolist() == [2, 1, 1, 2])
    R.close()


@pytest.mark.parametrize("n", [255, 256, 257, 600])
def test_one_hot_site_and_the_rank_kernels_tile_edges(n, gpu_lib):
    """n witnesses at one site that share (mt, strand, mpos) in groups, so that the read index breaks the ties, given in two alignment
    orders: the cluster rows are equal, and the witness rows name the same reads."""
    p = BEG + 1000
    rng = np.random.default_rng(n)
    groups = [(7, 0x20, 500), (7, 0x20, 500 + REQ["max_gap"]), (7, 0x00, 500), (2, 0x20, 123), (2 ** 20, 0x20, 77), (0, 0x20, 5)]
    specs = []
    for i in range(n):
        mt, mstrand, mpos = groups[int(rng.integers(0, len(groups)))] if i % 3 else groups[0]
        specs.append((p - 60 - BEG - (i % 40), (FWD & ~0x20) | mstrand, 50, mpos, mt, 10 + i % 50))
    reads, mtid = cpu.pair_reads(specs)
    rows, _ = cpu.site_rows([(p, RIGHT)])
    R = open_region(gpu_lib, reads)
    _, sr, cl, wit = check(R, reads, rows, mtid, n, **REQ)
    assert sr[0, cm.SW["facing"]] == n and sr[0, cm.SW["concordant"]] == 0 and cl[:, cm.CW["pairs"]].sum() == n and len(cl) == 5
    assert cl[:, cm.CW["mtid"]].tolist() == [0, 2, 7, 7, 2 ** 20] and (np.diff(wit[:, 1][wit[:, 2] == 2]) > 0).all()
    order = np.random.default_rng(1).permutation(n)
    reads2, mtid2 = cpu.pair_reads([specs[i] for i in order])
    R.reset(TID, BEG, BEG + cpu.REF_LEN, reads2["refseq"])
    R.set_reads(reads2)
    _, sr2, cl2, wit2 = check(R, reads2, rows, mtid2, (n, "shuffled"), **REQ)
    assert cl2.tobytes() == cl.tobytes() and sr2.tobytes() == sr.tobytes()
    assert sorted(zip(wit2[:, 2].tolist(), order[wit2[:, 1]].tolist())) == sorted(zip(wit[:, 2].tolist(), wit[:, 1].tolist()))
    R.close()


def test_two_sites_three_bp_apart_share_their_witnesses(gpu_lib):
    p = BEG + 1500
    specs = [(p - 80 - BEG + (i % 7), FWD, 50, 3000 + 10 * i, 4) for i in range(70)] + [(p + 10 - BEG - (i % 5), REV, 50, 100 + i, TID) for i in range(70)]
    reads, mtid = cpu.pair_reads(specs)
    rows, _ = cpu.site_rows([(p, RIGHT), (p + 3, RIGHT), (p, LEFT), (p + 3, LEFT)])
    R = open_region(gpu_lib, reads)
    _, sr, cl, wit = check(R, reads, rows, mtid, "3 bp", **REQ)
    assert sr[:, cm.SW["facing"]].tolist() == [70] * 4 and len(wit) == 280 and len(cl) == 4 and cl[:, cm.CW["pairs"]].tolist() == [70] * 4
    R.close()


# ------------------------------------------------------------------------------------------------ the ABI
def raw_fn(lib):
    fn = lib.dll.uvcgpu_region_clip_mates
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return fn


SENTINEL = -123456789


def raw_call(lib, R, rows, mtid, req=None, want_reads=1, clus_cap=0, read_cap=0, n=None, null=(), tid=TID):
    """One call of the ABI with every output filled with a sentinel first -> rc, totals, site rows, clusters, n_clusters, reads, n_reads, message"""
    q = dict(REQ, **(req or {}))
    rq = _ffi.UvcClipMatesRequest(tid, q["min_mapq"], q["window"], q["overhang"], q["min_dist"], q["max_gap"], q["min_pairs"], want_reads)
    rows = np.ascontiguousarray(rows, np.int64)
    totals = np.full(8, SENTINEL, np.int64)
    sr = np.full((max(len(rows), 1), cm.SITE_ROW), SENTINEL, np.int64)
    cl = np.full((max(abs(clus_cap), 1), cm.ROW), SENTINEL, np.int64)
    ev = np.full((max(abs(read_cap), 1), 4), SENTINEL, np.int32)
    nc, nr = C.c_int64(SENTINEL), C.c_int64(SENTINEL)
    p = lambda name, v: None if name in null else v                                           # noqa: E731
    rc = raw_fn(lib)(R.h, p("sites", rows.ctypes.data), len(rows) if n is None else n, None if mtid is None else mtid.ctypes.data, p("req", C.byref(rq)), p("totals", totals.ctypes.data),
                     p("site_rows", sr.ctypes.data), p("clusters", cl.ctypes.data), clus_cap, p("n_clusters", C.byref(nc)), p("reads", ev.ctypes.data), read_cap, p("n_reads", C.byref(nr)))
    return rc, totals, sr, cl, nc.value, ev, nr.value, lib.last_error()


def test_sizes_first_and_two_calls_return_the_same_bytes(gpu_lib):
    reads, mtid, rows = mixed(600, 5, 12)
    R = open_region(gpu_lib, reads)
    wt, wsr, wcl, wwit = cm.run(reads, rows, mtid, TID, **REQ)
    nc, nr = len(wcl), len(wwit)
    assert nc > 5 and nr > nc
    for kw in (dict(clus_cap=0, read_cap=0, null=("clusters", "reads")), dict(clus_cap=nc - 1, read_cap=nr), dict(clus_cap=nc, read_cap=nr - 1), dict(clus_cap=0, read_cap=0)):
        rc, totals, sr, cl, n_c, ev, n_r, msg = raw_call(gpu_lib, R, rows, mtid, **kw)
        assert rc == ENOMEM and n_c == nc and n_r == nr and totals.tolist() == wt.tolist() and np.array_equal(sr, wsr) and (cl == SENTINEL).all() and (ev == SENTINEL).all() and "clip_mates" in msg, (kw, rc, msg)
        assert str(nc if kw["clus_cap"] < nc else nr) in msg
    rc, totals, sr, cl, n_c, ev, n_r, msg = raw_call(gpu_lib, R, rows, mtid, clus_cap=nc, read_cap=nr)
    assert rc == 0 and n_c == nc and n_r == nr and totals.tolist() == wt.tolist() and np.array_equal(sr, wsr) and np.array_equal(cl, wcl) and np.array_equal(ev, wwit), msg
    rc2, t2, sr2, cl2, _, ev2, _, _ = raw_call(gpu_lib, R, rows, mtid, clus_cap=nc, read_cap=nr)   # a second identical call: the same bytes
    assert rc2 == 0 and t2.tobytes() == totals.tobytes() and sr2.tobytes() == sr.tobytes() and cl2.tobytes() == cl.tobytes() and ev2.tobytes() == ev.tobytes()
    rc, _, _, cl3, n3, ev3, r3, _ = raw_call(gpu_lib, R, rows, mtid, clus_cap=nc + 3, read_cap=nr + 5)   # more room than rows: nothing behind them
    assert rc == 0 and n3 == nc and r3 == nr and np.array_equal(cl3[:nc], wcl) and (cl3[nc:] == SENTINEL).all() and np.array_equal(ev3[:nr], wwit) and (ev3[nr:] == SENTINEL).all()
    for kw in (dict(read_cap=0, null=("reads",)), dict(read_cap=2)):   # want_reads = 0 with no room for reads: the clusters, *n_reads, no witness row
        rc, totals, sr, cl, n_c, ev, n_r, msg = raw_call(gpu_lib, R, rows, mtid, want_reads=0, clus_cap=nc, **kw)
        assert rc == 0 and n_c == nc and n_r == nr and np.array_equal(cl, wcl) and (ev == SENTINEL).all(), (kw, rc, msg)
    R.close()


def test_refusals_and_the_legal_window(gpu_lib):
    reads, mtid, rows = mixed(300, 11, 8)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), TID, reads["beg"], reads["end"], reads["refseq"])
    npos = R.npos

    def refused(what, word, **kw):
        rc, totals, sr, cl, n_c, ev, n_r, msg = raw_call(gpu_lib, R, kw.pop("rows", rows), mtid, clus_cap=kw.pop("clus_cap", 4), read_cap=kw.pop("read_cap", 4), **kw)
        assert rc == EINVAL and word in msg and "clip_mates" in msg, (what, rc, msg)
        assert (totals == SENTINEL).all() and (sr == SENTINEL).all() and (cl == SENTINEL).all() and (ev == SENTINEL).all() and n_c == SENTINEL and n_r == SENTINEL, what

    def moved(k, pos=None, side=None):
        out = rows.copy()
        if pos is not None:
            out[k, cr.W["pos"]] = pos
        if side is not None:
            out[k, cr.W["side"]] = side
        return out

    refused("before set_reads", "set_reads")
    R.set_reads(reads)
    check(R, reads, rows, mtid, "before accumulate", **REQ)
    for what, word, kw in [
        ("NULL req", "NULL", dict(null=("req",))), ("NULL totals", "NULL", dict(null=("totals",))), ("NULL n_clusters", "NULL", dict(null=("n_clusters",))),
        ("NULL n_reads", "NULL", dict(null=("n_reads",))), ("NULL site_rows", "NULL", dict(null=("site_rows",))), ("NULL sites", "NULL", dict(null=("sites",))),
        ("a negative count", "n_sites", dict(n=-1)), ("tid -1", "tid", dict(tid=-1)),
        ("min_mapq -1", "min_mapq", dict(req=dict(min_mapq=-1))), ("min_mapq 256", "min_mapq", dict(req=dict(min_mapq=256))),
        ("window 0", "window", dict(req=dict(window=0))), ("overhang -1", "overhang", dict(req=dict(overhang=-1))), ("min_dist 0", "min_dist", dict(req=dict(min_dist=0))),
        ("max_gap -1", "max_gap", dict(req=dict(max_gap=-1))), ("min_pairs 0", "min_pairs", dict(req=dict(min_pairs=0))),
        ("want_reads -1", "want_reads", dict(want_reads=-1)), ("want_reads 2", "want_reads", dict(want_reads=2)),
        ("a negative cluster capacity", "cluster_capacity", dict(clus_cap=-1)), ("a negative read capacity", "read_capacity", dict(read_cap=-1)),
        ("NULL clusters with room", "clusters is NULL", dict(null=("clusters",))), ("NULL reads with room", "reads is NULL", dict(null=("reads",))),
        ("a row in front of the region", "row 0", dict(rows=moved(0, pos=BEG - 1))), ("a row behind the region", "row 7", dict(rows=moved(7, pos=BEG + npos))),
        ("side 2", "side 2", dict(rows=moved(3, side=2))), ("side -1", "side -1", dict(rows=moved(3, side=-1))),
        ("rows out of order", "row 5", dict(rows=moved(5, pos=int(rows[4, cr.W["pos"]]), side=int(rows[4, cr.W["side"]])))),
        ("rows descending", "row 1", dict(rows=rows[::-1])),
    ]:
        refused(what, word, **kw)
    check(R, reads, rows, mtid, "after the refusals", **REQ)   # the handle is as usable as before
    rc, totals, sr, cl, n_c, ev, n_r, msg = raw_call(gpu_lib, R, rows[:0], mtid, null=("sites", "site_rows", "clusters", "reads"))   # no site: zero totals and success
    assert rc == 0 and not totals.any() and n_c == 0 and n_r == 0, msg
    # legal after accumulate, after a score with released planes, while a score stream is open; refused after a reset
    R.accumulate()
    check(R, reads, rows, mtid, "after accumulate", **dict(REQ, min_mapq=20))
    R.score(release_state=True)
    check(R, reads, rows, mtid, "after a releasing score", **REQ)
    R.accumulate()
    gen = R.score_stream(4096)
    next(gen)
    check(R, reads, rows, mtid, "while a score stream is open", **dict(REQ, min_pairs=1))
    gen.close()
    R.reset(TID, reads["beg"], reads["end"], reads["refseq"])
    refused("after a reset", "set_reads")
    R.close()


# ------------------------------------------------------------------------------------------------ the chain and the command line
from test_bq_correction import make_reads  # noqa: E402

GATE = (0, 10, 3)
MREQ = dict(window=100, overhang=5, min_dist=1000, max_gap=50, min_pairs=2)
CLIP = "ACGTTGCAAGGCTTAGCCTA"
P_SITE, Q_SITE = 1500, 2200


def translocation(ref, beg, tid, other):
    """(x, flag, cigar, sequence, mpos, mt, qname) per alignment: 40 forward reads clipped at the RIGHT site beg + 1500 whose mates lie on
    contig `other` 7 bp apart (a planted translocation), 12 reverse reads clipped at the LEFT site beg + 2200 whose mates lie 5 kb in
    front on the same contig, and 30 concordant pairs over the region."""
    specs = []
    for i in range(40):
        x = P_SITE - 50 - (i % 25)
        specs.append((x, FWD, [(0, P_SITE - x), (4, 20)], ref[x:P_SITE] + CLIP, 5000 + 7 * i, other, "t%d" % i))
    for i in range(12):
        ln = 50 + (i % 20)
        specs.append((Q_SITE, REV, [(4, 20), (0, ln)], CLIP[::-1] + ref[Q_SITE:Q_SITE + ln], beg + Q_SITE - 5000 - 3 * i, tid, "u%d" % i))
    for i, x in enumerate(range(300, 2600, 77)):
        specs.append((x, FWD, [(0, 60)], ref[x:x + 60], beg + x + 200, tid, "b%d" % i))
        specs.append((x + 200, REV, [(0, 60)], ref[x + 200:x + 260], beg + x, tid, "b%d" % i))
    return specs


def codes(s):
    return ["ACGT".index(c) for c in s]


def test_reads_to_sites_to_mates_a_planted_translocation(gpu_lib, tmp_path):
    ref = "".join("ACGT"[i] for i in np.random.default_rng(77).integers(0, 4, 3000))
    specs = translocation(ref, BEG, TID, 1)
    reads = make_reads([(x, fl, cg, codes(seq), [30] * len(seq)) for x, fl, cg, seq, mpos, mt, qn in specs], beg=BEG, ref_len=len(ref))
    reads["refseq"], reads["tid"] = ref, TID
    reads["mpos"] = np.array([s[4] for s in specs], np.int32)
    reads["qnames"] = [s[6] for s in specs]
    mtid = np.array([s[5] for s in specs], np.int32)
    R = open_region(gpu_lib, reads)
    totals, rows, ev = R.clip_sites([(BEG, BEG + 3001)], *GATE, want_reads=True)
    assert [(int(r[cr.W["pos"]]) - BEG, int(r[cr.W["side"]])) for r in rows] == [(P_SITE, RIGHT), (Q_SITE, LEFT)]
    wt, wsr, wcl, wwit = check(R, reads, rows, mtid, "translocation", **MREQ)
    assert wcl[:, [cm.CW[n] for n in ("site", "mtid", "mate_strand", "mpos_min", "mpos_max", "pairs", "other_contig", "far")]].tolist() == [[0, 1, 1, 5000, 5273, 40, 40, 0], [1, TID, 0, BEG + Q_SITE - 5033, BEG + Q_SITE - 5000, 12, 0, 12]]
    assert wsr[0, cm.SW["concordant"]] > 0
    got = R.clip_mates(rows, mtid, TID, **MREQ)
    with uio.ClipSites(*GATE, 0) as st:
        st.set_mates(**MREQ, contig_names=["chr%d" % k for k in range(TID + 1)])
        st.add(TID, "chr3", rows, ev, reads, reads["qnames"], mates=got[1:])
        st.write(tmp_path / "t.tsv")
    m = [l.split("\t") for l in (tmp_path / "t.tsv").read_text().splitlines() if l.startswith("M\t")]
    assert [f for f in m if f[8] == "40"] == [["M", "chr3", str(BEG + P_SITE + 1), "R", "chr1", "5001", "5274", "-", "40", "40", "0", "0", "2400", "40", "40", "0"]], m
    assert len(m) == 2 and m[1][4] == "chr3" and m[1][8] == "12"
    R.close()


def two_contig_panel(d):
    """chrA holds the 3 kb region of the chain test from 20 000 on with its reads, chrB is where the mates of the translocation lie; a BED
    line over the region.  The records carry their own mtid."""
    ref = "".join("ACGT"[i] for i in np.random.default_rng(77).integers(0, 4, 3000))
    off = 20_000
    rng = np.random.default_rng(6)
    flank = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))                        # noqa: E731
    chr_a, chr_b = flank(off) + ref + flank(4000), flank(9000)
    recs = [dict(tid=0, pos=off + x, qname=qn, flag=fl, mapq=60, cigar=cg, bases=codes(seq), quals=[30] * len(seq), mtid=mt, mpos=mpos, tlen=0, nm=0)
            for x, fl, cg, seq, mpos, mt, qn in translocation(ref, off, 0, 1)]
    recs.sort(key=lambda r: r["pos"])
    bam, fa, bed = os.path.join(d, "m.bam"), os.path.join(d, "m.fa"), os.path.join(d, "m.bed")
    bamwriter.write_bam(bam, [("chrA", len(chr_a)), ("chrB", len(chr_b))], recs)
    bamwriter.write_fasta(fa, [("chrA", chr_a), ("chrB", chr_b)])
    lines = [("chrA", off + 100, off + 2900)]
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % l for l in lines))
    return bam, fa, bed, lines, off


def chain(gpu_lib, hb, hf, lines, path, mates):
    """The report of the Python chain: every BED line its own region, Region.clip_sites over the positions it owns, Region.clip_mates on
    those rows with the fetch's mate contigs, io.ClipSites; and the same text from the restatements on the chain's rows."""
    calls, restated = [], []
    names = [n for n, _ in hb.refs]
    req = tuple(MREQ[k] for k in ("window", "overhang", "min_dist", "max_gap", "min_pairs"))
    with uio.ClipSites(*GATE, 1) as st:
        if mates:
            st.set_mates(*req, contig_names=names)
        for chrom, b, e in lines:
            res = pipeline.call_region(gpu_lib, hb, hf, chrom, b, e, keep_handle=True)
            a, z = res["score_range"][0], min(res["score_range"][1], e)
            R, tid = res["region"], hb.tid(chrom)
            totals, rows, ev = R.clip_sites([(a, z)], *GATE, want_reads=True)
            got = R.clip_mates(rows, res["mtid"], tid, min_mapq=GATE[0], **MREQ)
            want = cm.run(res["reads"], rows, res["mtid"], tid, min_mapq=GATE[0], **MREQ)
            assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and [tuple(int(v) for v in w) for w in got[3]] == [tuple(int(v) for v in w) for w in want[3]]
            qn = [res["qnames"][int(i)] for i in res["order"]]
            st.add(tid, chrom, rows, ev, res["reads"], qn, mates=got[1:] if mates else None)
            evs = np.stack([ev[k] for k in region.CLIP_READ.names], axis=1).astype(np.int64).reshape(-1, 4)
            calls.append((tid, chrom, rows, evs, dict(res["reads"], qnames=qn)))
            restated.append(want[1:])
            R.close()
        st.write(path)
    text = open(path).read()
    plain = cr.report_text(calls, *GATE, 1)
    assert text == (cm.report_text(plain, calls, names, restated, req) if mates else plain)
    return text


def test_cli_mate_lines_on_a_two_contig_bam(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, off = two_contig_panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    want = chain(gpu_lib, hb, hf, lines, o("chain.tsv"), True)
    plain = chain(gpu_lib, hb, hf, lines, o("chain0.tsv"), False)
    ml = [l.split("\t") for l in want.splitlines() if l.startswith("M\t")]
    assert [f[:12] for f in ml] == [["M", "chrA", str(off + P_SITE + 1), "R", "chrB", "5001", "5274", "-", "40", "40", "0", "0"],
                                    ["M", "chrA", str(off + Q_SITE + 1), "L", "chrA", str(off + Q_SITE - 5033 + 1), str(off + Q_SITE - 5000 + 1), "+", "12", "0", "0", "12"]], ml
    mopts = ["--clip-sites-mates", "1", "--clip-sites-mate-window", "100", "--clip-sites-mate-max-gap", "50"]
    vcf_without = run_cli(bam, fa, o("p.vcf.gz"), "-R", bed, "-t", "2", "--clip-sites-out", o("p.tsv"), "--clip-sites-reads", "1", "--clip-sites-junctions", "1")
    vcf_with = run_cli(bam, fa, o("m.vcf.gz"), "-R", bed, "-t", "2", "--clip-sites-out", o("m.tsv"), "--clip-sites-reads", "1", "--clip-sites-junctions", "1", *mopts)
    run_cli(bam, fa, o("n.vcf.gz"), "-R", bed, "-t", "2", "--clip-sites-out", o("n.tsv"), "--clip-sites-reads", "1", *mopts)
    got, got_without, got_nojunc = open(o("m.tsv")).read(), open(o("p.tsv")).read(), open(o("n.tsv")).read()
    assert got_nojunc == want, [(g, w) for g, w in zip(got_nojunc.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100
    mate_only = ("P\t", "M\t", "#P\t", "#M\t", "##clip_sites_mate_")
    assert [l for l in got.splitlines() if not l.startswith(mate_only)] == got_without.splitlines()      # the S, R and J lines are those without the option
    assert [l for l in got_nojunc.splitlines() if not l.startswith(mate_only)] == plain.splitlines()
    assert [l for l in got.splitlines() if l.startswith(mate_only[:2])] == [l for l in want.splitlines() if l.startswith(mate_only[:2])] and sum(l.startswith("J\t") for l in got.splitlines()) == 2
