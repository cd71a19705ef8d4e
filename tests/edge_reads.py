"""Reads on either side of the 16-bit fields and fall-backs of the accumulate work list ("Packed fields"), and the long
reads the fuzz comparison never had: a small background of tests/test_gpu_fuzz.py::weird_region plus reads placed by hand (add_read).
tests/test_edge_reads_cpu.py holds the preconditions (which side of its edge every placed read is on, that the oracle accepts the input and
counts what the case is about); tests/test_gpu_edge_reads.py compares the HIP path with the oracle.

Every case is a dict: reads (the input), placed ([{name, index, ops, ...}] of the hand-placed alignments), platform, and what else its tests
need.  The restatements of the guards are plain Python written from the guard expressions:

  classify       simple / kind 1 / kind 2 of k_read_facts (uvc_prep.hip, "P2 work list") and the demotion of k_aln_prelude (has_lowbq_indel)
  runs_b_ok      aln_runs of k_fragstat_fast: at most one InDel, no reference skip, special range (deletion + 1) below 32 768
  frag_span      FragRec::end - beg with the reference's "+ 1 per alignment", clamped to the region (the FF_RUNS_B form needs < 65 536)
  penalty        by_nm + by_clip of the prelude (tests/p2_restatement.py:127, C integer division)"""
import functools

import numpy as np

from test_gpu_fuzz import add_read, weird_region

M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
LOWBQ_THRES = 21          # bias_thres_interfering_indel_BQ (include/uvc_params.def)
CLIP_MIN_LEN = 12         # microadjust_alignment_clip_min_len
NEAR_CLIP_DIST = 2        # microadjust_near_clip_dist
EUNSUPPORTED = -3         # UVCGPU_EUNSUPPORTED
LONG_LENGTHS = (1, 5, 60, 150, 300, 700, 1500, 3000)


def cdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


# ---- the guards, restated ----
def ref_len_of(ops):
    return max(1, sum(l for o, l in ops if o in (M, D, N)))


def is_simple(ops):
    n_m = sum(1 for o, l in ops if o == M)
    if n_m != 1 or len(ops) > 3 or any(o not in (M, S, H) for o, l in ops):
        return False
    return not (len(ops) == 3 and (ops[0][0] == M or ops[2][0] == M))


def run_offsets_of(ops):
    """[(offset of the M run from the alignment's begin, offset of its end from the alignment's end)]"""
    span, rp, out = ref_len_of(ops), 0, []
    for o, l in ops:
        if o == M:
            out.append((rp, span - (rp + l))); rp += l
        elif o in (D, N):
            rp += l
    return out


def has_lowbq_indel(ops, quals, thres=LOWBQ_THRES):
    lq = len(quals)
    Q = lambda q: int(quals[min(max(q, 0), lq - 1)])
    qpos = 0
    for o, l in ops:
        if o in (M, S):
            qpos += l
        elif o == I:
            if any(Q(q2) < thres for q2 in range(qpos - min(qpos, 1), qpos + l + 1)):   # (the reference's bound is a reference position, far beyond the read)
                return True
            qpos += l
        elif o == D and min(Q(max(1, qpos) - 1), Q(qpos)) <= thres:
            return True
    return False


def classify(ops, quals, region_beg, platform):
    """0: simple (one work-list entry), 2: its M runs are on the work list, 1: the per-read path."""
    if is_simple(ops):
        return 0
    seg_eligible = (platform != 2) and region_beg >= 65536
    ok = seg_eligible and all(o != N for o, l in ops) and all(a <= 65535 and b <= 65535 for a, b in run_offsets_of(ops))
    if ok and has_lowbq_indel(ops, quals):
        ok = False
    return 2 if ok else 1


def runs_b_ok(ops):
    n_runs = n_indel = sp_len = 0
    for o, l in ops:
        if o == M:
            n_runs += 1
        elif o == I:
            n_indel += 1; sp_len = 1
        elif o == D:
            n_indel += 1; sp_len = l + 1
        elif o not in (S, H):
            return False
    return 1 <= n_runs <= 2 and n_indel <= 1 and sp_len < 32768


def frag_span(alns, region_end):
    """alns = [(pos, ops)] of one fragment in read order."""
    beg, end = 2 ** 31 - 1, 0
    for pos, ops in alns:
        beg = min(beg, pos); end = max(end, pos + ref_len_of(ops)) + 1
    return min(end, region_end) - beg


def penalty(ops, nm):
    span = ref_len_of(ops)
    nge = sum(l for o, l in ops if o in (I, D)); ngo = sum(1 for o, l in ops if o in (I, D))
    nm_cnt = nm if nm >= 0 else nge
    xm1500 = cdiv((nm_cnt - nge) * 1500, span); go1500 = cdiv(ngo * 1500, span)
    lclip = ops[0][1] if ops[0][0] == S else 0
    rclip = ops[-1][1] if ops[-1][0] == S else 0
    return cdiv(xm1500 + go1500, 30) + cdiv(max(lclip, rclip), 6)


def clip_cells(pos, ops):
    """[(position, op length)] of the S / H ops: where update_seg_format_prep_sets_by_aln counts a clip (main.hpp:1183-1199)."""
    out, rp = [], pos
    for k, (o, l) in enumerate(ops):
        if o in (S, H):
            out.append((rp + (0 if k == 0 else -1), l))
        elif o in (M, D, N):
            rp += l
    return out


# ---- building blocks ----
class Placer:
    """add_read with bookkeeping: every placed alignment is a fragment and family of its own unless `mate_of_last`."""
    def __init__(self, reads, seed):
        self.reads, self.rng, self.placed = reads, np.random.default_rng(seed), []
        self.frag, self.fam = int(reads["frag_id"].max()) + 1, int(reads["n_fams"])

    def add(self, name, start, ops, qual=35, nm=-1, reverse=False, flag=None, dflag=0, mate_of_last=False, mismatch=0.0, low_at=(), **facts):
        r = self.reads
        if mate_of_last:
            self.frag -= 1; self.fam -= 1
        fl = flag if flag is not None else (0x10 if reverse else 0)
        strand = self.placed[-1]["strand"] if mate_of_last else int(reverse)
        add_read(r, r["beg"] + start, ops, qual, nm, self.rng, self.frag, self.fam, strand=strand, flag=fl)
        if mate_of_last:
            r["n_fams"] -= 1; r["fam_dflag"] = r["fam_dflag"][:-1]
        else:
            r["fam_dflag"][-1] = dflag
        i = int(r["n_reads"]) - 1
        so, lq = int(r["seq_off"][i]), int(r["l_qseq"][i])
        if mismatch:
            hit = self.rng.random(lq) < mismatch
            r["bases"][so:so + lq][hit] = (r["bases"][so:so + lq][hit] + self.rng.integers(1, 4, int(hit.sum()))) % 4
        for q in low_at:
            r["quals"][so + q] = 2
        self.frag += 1; self.fam += 1
        self.placed.append(dict(name=name, index=i, pos=int(r["beg"]) + start, ops=list(ops), strand=strand, **facts))
        return i


def quals_of(reads, p):
    so = int(reads["seq_off"][p["index"]])
    return reads["quals"][so:so + int(reads["l_qseq"][p["index"]])]


def cigar_text(ops):
    return "".join("%d%s" % (l, "MIDNSH"[o]) for o, l in ops)


# ---- clips ----
CLIP_READS = [   # (ops, True: the clip is long for the HIP path too before the repair / the half of FastRec::clips is below 65 535)
    ([(H, 65535), (M, 60)], True), ([(H, 65536), (M, 60)], False), ([(H, 65539), (M, 60)], False), ([(M, 60), (H, 65536)], False),
    ([(M, 60), (H, 131075)], False), ([(S, 65537), (M, 50)], False), ([(M, 50), (S, 65540)], False), ([(M, 60), (H, 65535)], True),
    ([(S, 32767), (M, 50)], True), ([(M, 50), (S, 32768)], True),
]
CLIP_CONTROL = [(H, 5), (S, 10), (M, 100)]


@functools.lru_cache(maxsize=None)
def clips(amplicon, reverse):
    """Simple alignments whose clip op length straddles 16 bits, and 5H10S100M: not a simple alignment, both clips short."""
    reads = weird_region(41, n_frag=40, ref_len=600, beg=1_000_000)
    background = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in reads.items()}
    P = Placer(reads, 410)
    for k, (ops, fits) in enumerate(CLIP_READS):
        P.add(cigar_text(ops), 20 + 47 * k, ops, dflag=(4 if amplicon else 0), reverse=reverse, fits_16_bits=fits, control=False)
    P.add(cigar_text(CLIP_CONTROL), 480, CLIP_CONTROL, dflag=(4 if amplicon else 0), reverse=reverse, fits_16_bits=True, control=True)
    return dict(reads=reads, background=background, placed=P.placed, platform=1, amplicon=amplicon)


# ---- run offsets ----
def long_indel_ops(first_len, last_len, total=66000, n_indel=60):
    """first_len M, then n_indel InDels (2I and 3D in turn) about every 1.1 kb, last_len M at the end; `total` reference bases."""
    n_del = n_indel // 2
    mid = total - first_len - last_len - 3 * n_del            # reference bases of the n_indel - 1 M runs in between
    each = mid // (n_indel - 1)
    ops = [(M, first_len)]
    for k in range(n_indel):
        ops.append((I, 2) if k % 2 == 0 else (D, 3))
        if k < n_indel - 1:
            ops.append((M, each + (mid - each * (n_indel - 1) if k == n_indel - 2 else 0)))
    ops.append((M, last_len))
    assert ref_len_of(ops) == total
    return ops


DELETION_READS = [[(M, 40), (D, 65536), (M, 40)], [(M, 40), (D, 65535), (M, 40), (I, 3), (M, 10)], [(M, 40), (D, 32766), (M, 40)], [(M, 40), (D, 32767), (M, 40)],
                  [(M, 40), (N, 66000), (M, 40)]]


@functools.lru_cache(maxsize=None)
def run_offsets(beg):
    """A 66.5 kb region.  One M run beyond 65 535 from either end makes the WHOLE read kind 1, so the two sides of that edge are separate reads:
    66 000 reference bases, sixty InDels, the last run beginning at 65 535 (465 bases long) or 65 536 (464), the first ending 65 535 or
    65 536 before the end; a copy whose first InDel has quality 2 beside it (demoted by the prelude; distances to it reach 65 535 and
    more).  Then 66000M, the deletions and the skip, the deletions again with quality 2 beside them, and three mate pairs by fragment span."""
    ref_len = 66500
    reads = weird_region(42, n_frag=100, ref_len=ref_len, beg=beg)
    P = Placer(reads, 420)
    # the last M run begins 65 535 / 65 536 from the alignment's begin, the first ends 65 535 / 65 536 before its end
    for name, first, last in (("both offsets 65535", 465, 465), ("begin offset 65536", 465, 464), ("end offset 65536", 464, 465)):
        ops = long_indel_ops(first, last)
        P.add(name, 100 + 7 * len(P.placed), ops, nm=sum(l for o, l in ops if o in (I, D)), max_offsets=(66000 - last, 66000 - first), kind=(2 if first == last else 1))
    ops = long_indel_ops(465, 465)
    P.add("both offsets 65535, first InDel of low quality", 130, ops, low_at=(464, 465), max_offsets=(65535, 65535), kind=1)
    P.add("66000M reverse", 150, [(M, 66000)], reverse=True, mismatch=0.002, kind=0)
    for k, ops in enumerate(DELETION_READS):
        P.add(cigar_text(ops), 200 + 11 * k, ops, nm=0 if k % 2 else -1, reverse=bool(k % 2), kind=(1, 1, 2, 2, 1)[k], runs_b=(k == 2))
    for k, ops in enumerate(DELETION_READS[:4]):   # quality 2 either side of the deletion: the item path (k_p2_items)
        P.add(cigar_text(ops) + " low quality", 260 + 11 * k, ops, qual=30, low_at=(39, 40), reverse=not k % 2, kind=1, runs_b=(k == 2))
    for k, want in enumerate((65535, 65536, 65537)):   # mates of one fragment: a simple one and 20M2I30M, fragment span = want
        a = 300 + 13 * k
        P.add("mate 60M, span %d" % want, a, [(M, 60)], qual=30, flag=0x1 | 0x40, kind=0)
        P.add("mate 20M2I30M, span %d" % want, a + want - 51, [(M, 20), (I, 2), (M, 30)], qual=30, flag=0x1 | 0x80 | 0x10, mate_of_last=True, span=want, kind=2)
    return dict(reads=reads, placed=P.placed, beg=beg)


# ---- region begin ----
@functools.lru_cache(maxsize=None)
def region_begin(beg):
    return dict(reads=weird_region(43, n_frag=120, ref_len=700, beg=beg), placed=[], platform=1)


# ---- NM penalty ----
# 5M<k>I5M with NM 0 spans 10 reference bases: xm1500 = -150 k, go1500 = 150, by_nm = -5 (k - 1), always a multiple of 5.  -30 000 is k = 6001;
# -30 001 needs by_clip: k = 6002 gives -30 005, a soft clip of 24 adds 4 and one of 30 adds 5.
NM_AT = [[(M, 5), (I, 6001), (M, 5)], [(S, 30), (M, 5), (I, 6002), (M, 5)]]
NM_BELOW = [(S, 24), (M, 5), (I, 6002), (M, 5)]


@functools.lru_cache(maxsize=None)
def nm_penalty(below):
    reads = weird_region(44, n_frag=40, ref_len=700, beg=1_000_000)
    P = Placer(reads, 440)
    for k, ops in enumerate(NM_AT):
        P.add(cigar_text(ops), 100 + 200 * k, ops, nm=0, reverse=bool(k), want=-30000)
    if below:
        P.add(cigar_text(NM_BELOW), 500, NM_BELOW, nm=0, want=-30001)
    return dict(reads=reads, placed=P.placed, platform=1)


# ---- long reads ----
@functools.lru_cache(maxsize=None)
def long_fuzz(which):
    if which == "umi_9000":
        return dict(reads=weird_region(1, n_frag=150, ref_len=9000, umi=True, lengths=LONG_LENGTHS), placed=[], platform=1)
    if which == "dense_4100":
        return dict(reads=weird_region(2, n_frag=400, ref_len=4100, lengths=LONG_LENGTHS), placed=[], platform=1)
    reads = weird_region(3, n_frag=60, ref_len=9000, lengths=LONG_LENGTHS)
    P = Placer(reads, 450)
    for k, ln in enumerate((4095, 4096, 4097, 8200) * 3):   # single M runs around the 4 096-position window of k_fragstat_sweep
        ln += (0, 0, 13)[k // 4] if ln == 8200 else 0
        start = 10 + 37 * k
        if which == "runs_4096":
            ops = [(M, ln)]
        else:                                               # which == "runs_4096_del": the same reads with one 3-base deletion in the middle
            ops = [(M, ln // 2), (D, 3), (M, ln - ln // 2 - 3)]
        P.add(cigar_text(ops), start, ops, qual=(30, 37, 20)[k % 3], reverse=bool(k % 2), mismatch=0.01, run=ln)
    return dict(reads=reads, placed=P.placed, platform=1)


LONG_FUZZ = ("umi_9000", "dense_4100", "runs_4096", "runs_4096_del")


# ---- planted haplotypes ----
HAP_START, HAP_LEN = 200, 700
HAP_SNV_OFFSETS = (0, 63, 64, 128, 640)     # read offsets (= reference offsets from HAP_START) of the SNVs
HAP_INS_BEFORE = 128                          # 128M2I572M: the insertion directly in front of the SNV at offset 128


@functools.lru_cache(maxsize=None)
def planted_haplotypes():
    """Random errors never repeat, so fuzzed reads give no haplotype link.  Here 40 one-read fragments and 12 UMI families of 3 .. 5 fragments on
    both strands start at one position and carry the same five SNVs and one insertion (at read offsets 0, 63, 64, 127 | 128, 128, 640: the first
    and the last ten 64-position chunks apart); one 3 000-base fragment with 3 % mismatches has about 90 events in one object."""
    rng = np.random.default_rng(46)
    reads = weird_region(46, n_frag=30, ref_len=4000, beg=1_000_000)
    ref = np.array(["ACGT".index(c) for c in reads["refseq"]])
    P = Placer(reads, 460)
    ops = [(M, HAP_INS_BEFORE), (I, 2), (M, HAP_LEN - HAP_INS_BEFORE)]

    def plant(reverse, dflag=0, same_family=False):
        i = P.add("haplotype read", HAP_START, ops, qual=37, nm=7, reverse=reverse, dflag=dflag)
        r = reads
        so = int(r["seq_off"][i])
        for off in HAP_SNV_OFFSETS:
            q = off + (2 if off >= HAP_INS_BEFORE else 0)
            r["bases"][so + q] = (ref[HAP_START + off] + 1) % 4
        r["bases"][so + HAP_INS_BEFORE: so + HAP_INS_BEFORE + 2] = (0, 2)     # every read inserts the same two bases
        if same_family:                                                        # joins the family of the read before it
            r["fam_id"][i] -= 1; r["n_fams"] -= 1; r["fam_dflag"] = r["fam_dflag"][:-1]; P.fam -= 1
        return i

    for k in range(40):
        plant(reverse=bool(k % 2))
    for k in range(12):
        n = 3 + k % 3
        n0 = 1 + k % (n - 1)                                                   # fragments on strand 0 first, then strand 1: both strands in every family
        for j in range(n):
            plant(reverse=(j >= n0), dflag=0x3, same_family=(j > 0))
    P.add("3000M at 3 % mismatches", 900, [(M, 3000)], qual=37, mismatch=0.03)
    return dict(reads=reads, placed=P.placed, platform=1)
