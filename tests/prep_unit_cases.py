"""The inputs of tests/test_gpu_prep_units.py (the device read preparation against tests/prep_units_restatement.py), each built
deterministically, and the files the probe program (tests/native/prep_probe_main.cpp) reads and writes.  tests/test_prep_units_cpu.py
holds the preconditions: that each case reaches the edge it is about.

A preparation case is a dict: reads (the UvcReadSoA columns, tests' convention), rbeg / rend / npos, platform, overrides (UvcParams fields
moved off their defaults), zero_qual (UvcPrepIn::zero_qual: None = NULL).

  nesting   6 201 reads = three tiles of 2 048 and a ragged fourth: every CIGAR shape, fragments of 1-3 alignments, units of 1, 2 and 5
            fragments, families with one and with both strands, every fam_dflag, heads forced onto the thread / wave / tile edges.  Four arms.
  carry     2 x 1 024 x 2 048 + 2 048 + 1 reads of 1-3 bases: the tile sums of every scanned column go through three rounds of k_tile_tops
  depth     65 534 fragments that all reach over one position behind the first 1 024 tiles of the depth scan, k one-base fragments on it
  compact   the length columns of carry
  sort      keys of uvc_sort_by_pos_cls with mostly tied offsets"""
import os

import numpy as np

from prep_units_restatement import D, EQ, H, I, M, N, PAD, S, X

TILE = 2048                      # SC_TILE of uvc_prep.hip: elements per tile of its scans
ROUND = 1024 * TILE              # elements one round of k_tile_tops covers
EDGES = (8, 512, 2048, 4096)     # items of a thread, of a wave, of one and of two tiles
SENTINEL = -7                    # what the probe fills an output with that a scatter kernel may leave alone

SHAPES = [
    [(M, 50)], [(EQ, 20), (X, 1), (EQ, 29)], [(S, 5), (M, 45)], [(M, 45), (S, 5)], [(S, 3), (M, 44), (S, 3)], [(H, 5), (M, 50)],
    [(H, 2), (S, 3), (M, 40), (S, 4), (H, 1)], [(M, 20), (I, 2), (M, 28)], [(M, 20), (D, 3), (M, 30)],
    [(M, 10), (I, 1), (M, 10), (D, 2), (M, 10), (I, 3), (M, 16)], [(M, 20), (I, 2), (D, 2), (M, 28)], [(M, 20), (N, 100), (M, 30)],
    [(M, 20), (PAD, 1), (M, 30)], [(S, 3), (I, 2)], [(H, 5)], [(EQ, 50)], [(M, 1)],
]
INS_SHAPE, DEL_SHAPE = 7, 8


def soa(pos, shapes, flag, mapq, new_frag, new_fs, fam_of_unit, strand_of_unit, fam_dflag, qual=30):
    """The read columns from per-read positions and CIGAR shapes, the head marks and the family of each unit; reads back to back."""
    n = len(pos)
    n_cigar = np.array([len(s) for s in shapes], np.int32)
    cigars = np.array([(l << 4) | o for s in shapes for o, l in s], np.uint32)
    l_qseq = np.array([sum(l for o, l in s if o in (M, EQ, X, I, S)) for s in shapes], np.int32)
    unit = np.cumsum(new_fs) - 1
    return dict(n_reads=n, pos=np.asarray(pos, np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), nm=np.full(n, -1, np.int32),
                l_qseq=l_qseq, n_cigar=n_cigar, frag_id=(np.cumsum(new_frag) - 1).astype(np.int32), fam_id=np.asarray(fam_of_unit, np.int32)[unit],
                flag=np.asarray(flag, np.uint16), mapq=np.asarray(mapq, np.uint8), fam_strand=np.asarray(strand_of_unit, np.uint8)[unit],
                fam_dflag=np.asarray(fam_dflag, np.uint8), n_fams=len(fam_dflag), seq_off=np.concatenate([[0], np.cumsum(l_qseq[:-1], dtype=np.int64)]),
                cigar_off=np.concatenate([[0], np.cumsum(n_cigar[:-1], dtype=np.int64)]), cigars=cigars, quals=np.full(int(l_qseq.sum()), qual, np.uint8))


def families(n_units):
    """units in groups of 2, 1, 1: a family with both strands, then two families with one strand each -> (fam, strand) per unit, n_fams"""
    fam, strand, f = [], [], 0
    while len(fam) < n_units:
        for size in (2, 1, 1):
            for k in range(size):
                fam.append(f); strand.append(k if size == 2 else f % 2)
            f += 1
    return np.array(fam[:n_units]), np.array(strand[:n_units]), fam[n_units - 1] + 1


NESTING_ARMS = {
    "default": dict(rbeg=1_000_000),
    "low_begin": dict(rbeg=60_000),                                    # seg_eligible off: no kind 2, no InDel read on the work list
    "iontorrent": dict(rbeg=1_000_000, platform=2),
    "no_singleton": dict(rbeg=1_000_000, overrides=dict(fam_thres_dup1add=1)),   # every unit generic
}


def nesting(arm):
    a = NESTING_ARMS[arm]
    rbeg, n, npos = a["rbeg"], 3 * TILE + 57, 3000
    # heads by cycling patterns: alignments per fragment 1, 2, 3 ..., fragments per unit 1, 2, 5 ...
    new_frag, new_fs = np.zeros(n, bool), np.zeros(n, bool)
    i = k = 0
    while i < n:
        new_fs[i] = True
        for _ in range((1, 2, 5, 1, 2)[k % 5]):
            if i < n:
                new_frag[i] = True
            i += (1, 2, 3, 2, 1, 1, 3)[(k + i) % 7]
        k += 1
    for e in EDGES:          # a unit of one fragment of one alignment on either side of each edge and on it
        new_fs[e - 1:e + 3] = True; new_frag[e - 1:e + 3] = True
    new_frag[n - 2] = True; new_frag[n - 1] = False; new_fs[n - 1] = False   # the last fragment: two alignments, clamped by the region end
    new_frag |= new_fs
    shapes = [SHAPES[i % len(SHAPES)] for i in range(n)]
    for e in EDGES:          # an InDel read on either side: every scanned column carries a value across the edge
        shapes[e - 1] = SHAPES[INS_SHAPE]; shapes[e] = SHAPES[DEL_SHAPE]
    shapes[n - 2] = shapes[n - 1] = SHAPES[0]
    pos = rbeg + 10 + (np.arange(n) * 7) % 2500
    pos[n - 2:] = rbeg + npos - 1 - 50                                 # both end on the last position a read may cover
    n_units = int(new_fs.sum())
    fam, strand, n_fams = families(n_units)
    fam_dflag = np.array([0, 1, 2, 3, 4, 0, 2, 1])[np.arange(n_fams) % 8]   # UMI 0x1, duplex 0x2 (with and without a partner strand), amplicon 0x4
    reads = soa(pos, shapes, flag=np.array([0, 16, 99, 147, 83, 163, 161, 145, 177])[np.arange(n) % 9], mapq=np.array([60, 0, 255, 30, 60, 1, 44])[np.arange(n) % 7],
                new_frag=new_frag, new_fs=new_fs, fam_of_unit=fam, strand_of_unit=strand, fam_dflag=fam_dflag)
    zq = 300                                                           # a read in the middle of a tile: one quality byte of 0
    reads["quals"][reads["seq_off"][zq] + 1] = 0
    return dict(reads=reads, rbeg=rbeg, rend=rbeg + npos, npos=npos, platform=a.get("platform", 1), overrides=a.get("overrides", {}), zero_qual=None, zero_read=zq)


CARRY_N = 2 * ROUND + TILE + 1
CARRY_SHAPES = [[(M, 1)], [(M, 1), (I, 1), (M, 1)], [(M, 1), (D, 1), (M, 1)], [(S, 2), (M, 1)]]


def carry_lengths(n=CARRY_N):
    """l_qseq, n_cigar of carry (also the input of compact)"""
    k = np.arange(n) % 4
    return np.array([1, 3, 2, 3], np.int32)[k], np.array([1, 3, 3, 2], np.int32)[k]


def carry(n=CARRY_N):
    """every 3rd read starts a fragment, every 7th a unit; positions cycle over a 4 096-position region"""
    rbeg, npos = 1_000_000, 4096
    i = np.arange(n)
    l_qseq, n_cigar = carry_lengths(n)
    per_shape = [np.array([(l << 4) | o for o, l in s], np.uint32) for s in CARRY_SHAPES]
    block = np.concatenate(per_shape)                                  # the ops of four consecutive reads
    cigars = np.concatenate([np.tile(block, n // 4), np.concatenate(per_shape[:n % 4]) if n % 4 else np.zeros(0, np.uint32)])
    unit = i // 7
    n_units = int(unit[-1]) + 1
    n_fams = (n_units + 1) // 2
    reads = dict(n_reads=n, pos=(rbeg + i % 4093).astype(np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), nm=np.full(n, -1, np.int32),
                 l_qseq=l_qseq, n_cigar=n_cigar, frag_id=(np.cumsum((i % 3 == 0) | (i % 7 == 0)) - 1).astype(np.int32), fam_id=(unit // 2).astype(np.int32),
                 flag=np.array([0, 16, 161, 177], np.uint16)[(i // 3) % 4], mapq=np.full(n, 60, np.uint8), fam_strand=(unit % 2).astype(np.uint8),
                 fam_dflag=np.array([0, 2, 1, 3], np.uint8)[np.arange(n_fams) % 4], n_fams=n_fams, seq_off=np.cumsum(l_qseq, dtype=np.int64) - l_qseq,
                 cigar_off=np.cumsum(n_cigar, dtype=np.int64) - n_cigar, cigars=cigars, quals=np.full(int(l_qseq.sum(dtype=np.int64)), 30, np.uint8))
    return dict(reads=reads, rbeg=rbeg, rend=rbeg + npos, npos=npos, platform=1, overrides={}, zero_qual=0)


DEPTH_NPOS, DEPTH_PILE, DEPTH_THIN = 2_100_000, 2_099_000, 65_534
# arm -> (k one-base fragments on the pile position, short fragments behind every other one, the bound the preparation must report)
DEPTH_ARMS = {"count_65535": (1, 0, 65535), "depth_65535": (1, 2, 65535), "depth_65536": (2, 2, 65536), "depth_65537": (3, 2, 65537)}


def depth(arm):
    """DEPTH_THIN single-read fragments begin 31 positions apart inside the first 1 024 tiles of the depth scan and all end behind the pile
    position (1M <deletion> 1M), so each of them covers it; k fragments of one base lie on it; `extra` fragments of one base lie behind the
    end of all others (they only raise the fragment count to 65 536 and more, where the bound is the scanned depth and not the count)."""
    k, extra, _ = DEPTH_ARMS[arm]
    rbeg = 1_000_000
    start = np.arange(DEPTH_THIN) * 31
    assert start[-1] < ROUND < DEPTH_PILE
    shapes = [[(M, 1), (D, DEPTH_PILE + 500 - 2 - int(s)), (M, 1)] for s in start] + [[(M, 1)]] * (k + extra)
    pos = np.concatenate([rbeg + start, np.full(k, rbeg + DEPTH_PILE), np.full(extra, rbeg + DEPTH_PILE + 900)])
    n = len(pos)
    reads = soa(pos, shapes, flag=np.zeros(n), mapq=np.full(n, 60), new_frag=np.ones(n, bool), new_fs=np.ones(n, bool), fam_of_unit=np.arange(n), strand_of_unit=np.zeros(n),
                fam_dflag=np.zeros(n))
    return dict(reads=reads, rbeg=rbeg, rend=rbeg + DEPTH_NPOS, npos=DEPTH_NPOS, platform=1, overrides={}, zero_qual=0)


SORT_BITS = [(1, 0), (8, 0), (7, 1), (8, 1), (15, 1), (16, 1), (22, 2), (23, 2), (30, 2), (31, 1), (32, 0)]
SORT_N = [1, 255, 256, 257, 70_001]
SORT_BEG = 12_345


def sort_case(pos_bits, cls_bits, n):
    """Offsets from at most eight distinct values, 0 and 2^pos_bits - 1 among them, classes up to 2^cls_bits - 1 (both ends present where n
    allows); the two work lists of the gather: more entries than alignments (kind 0 with one entry, kind 2 with three) and fewer (kind 0
    with one entry, two of kind 1 without).  With n = 1 the first list has one alignment: an entry needs one."""
    rng = np.random.default_rng(1000 * pos_bits + 10 * cls_bits + n % 997)
    top = (1 << pos_bits) - 1
    values = np.unique(np.concatenate([[0, top], rng.integers(0, top + 1, 6)]))
    off = values[rng.integers(0, len(values), n)]
    cls = rng.integers(0, 1 << cls_bits, n)
    off[0] = top; cls[0] = (1 << cls_bits) - 1
    if n > 1:
        off[n - 1] = 0; cls[n - 1] = 0
    pos = ((SORT_BEG + off.astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)   # as an int32 column holds it
    lists = []
    for kinds, entries in (((0, 2), (1, 3)), ((0, 1, 1), (1, 0, 0))):
        kind, a0 = [], []
        while len(a0) < n or len(kind) % len(kinds):                   # (the last cycle of kinds is completed: alignments without an entry)
            j = len(kind) % len(kinds)
            a0 += [len(kind)] * min(entries[j], n - len(a0))
            kind.append(kinds[j])
        lists.append(dict(kind=np.array(kind, np.int32), a=[np.array(a0, np.int32)] + [rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32) for _ in range(3)]))
    return dict(pos=pos, cls=cls.astype(np.int32), beg=SORT_BEG, pos_bits=pos_bits, cls_bits=cls_bits, n=n, n_first=[0, n // 2, n], lists=lists)


# ---- the probe's files ----
def write_scalars(d, values):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "scalars.txt"), "w") as f:
        for k, v in values.items():
            f.write("%s %d\n" % (k, v))


def write_col(d, name, a, dtype):
    np.ascontiguousarray(a, dtype=dtype).tofile(os.path.join(d, "in_%s.bin" % name))


READ_COLUMNS = dict(pos=np.int32, mpos=np.int32, isize=np.int32, nm=np.int32, l_qseq=np.int32, n_cigar=np.int32, frag_id=np.int32, fam_id=np.int32, flag=np.uint16, mapq=np.uint8,
                    fam_strand=np.uint8, fam_dflag=np.uint8, seq_off=np.int64, cigar_off=np.int64, cigars=np.uint32, quals=np.uint8)


def write_prep(d, case):
    r = case["reads"]
    sc = dict(n_reads=r["n_reads"], n_bases=len(r["quals"]), n_cigar_ops=len(r["cigars"]), n_fams=r["n_fams"], rbeg=case["rbeg"], rend=case["rend"], npos=case["npos"],
              platform=case["platform"], zero_qual=-1 if case["zero_qual"] is None else case["zero_qual"])
    sc.update(case["overrides"])
    write_scalars(d, sc)
    for name, t in READ_COLUMNS.items():
        write_col(d, name, r[name], t)


def write_compact(d, l_qseq, n_cigar):
    write_scalars(d, dict(n_reads=len(l_qseq), n_bases=int(l_qseq.sum(dtype=np.int64)), n_b4=int(((l_qseq.astype(np.int64) + 1) // 2).sum())))
    write_col(d, "l_qseq", l_qseq, np.int32); write_col(d, "n_cigar", n_cigar, np.int32)


def write_sort(d, c):
    sc = dict(n=c["n"], beg=c["beg"], pos_bits=c["pos_bits"], cls_bits=c["cls_bits"], sentinel=SENTINEL, n_ranks=len(c["n_first"]), n_gathers=len(c["lists"]))
    sc.update({"n_first_%d" % k: v for k, v in enumerate(c["n_first"])})
    sc.update({"g%d_n_alns" % k: len(l["kind"]) for k, l in enumerate(c["lists"])})
    write_scalars(d, sc)
    write_col(d, "pos", c["pos"], np.int32); write_col(d, "cls", c["cls"], np.int32)
    for k, l in enumerate(c["lists"]):
        write_col(d, "g%d_kind" % k, l["kind"], np.int32)
        for j in range(4):
            write_col(d, "g%d_a%d" % (k, j), l["a"][j], np.int32)


def read_out(d, name, dtype):
    return np.fromfile(os.path.join(d, "out_%s.bin" % name), dtype=dtype)


def read_out_scalars(d):
    with open(os.path.join(d, "out_scalars.txt")) as f:
        return {k: int(v) for k, v in (line.split() for line in f)}


def handle_reads(case, seed=77):
    """The reads of a preparation case as a region handle takes them: bases that follow a random reference (0.5 % errors; inserted and
    clipped bases at random), tid / beg / end / refseq with the same [rbeg, rend) inside the handle."""
    rng = np.random.default_rng(seed)
    r = dict(case["reads"])
    n_ref = case["npos"] - 1
    ref = rng.integers(0, 4, n_ref + 1)
    bases = rng.integers(0, 4, len(r["quals"]))
    for i in range(r["n_reads"]):
        q, p = int(r["seq_off"][i]), int(r["pos"][i]) - case["rbeg"]
        for c in r["cigars"][r["cigar_off"][i]:r["cigar_off"][i] + r["n_cigar"][i]]:
            o, l = int(c) & 0xF, int(c) >> 4
            if o in (M, EQ, X):
                bases[q:q + l] = ref[p:p + l]
            q += l if o in (M, EQ, X, I, S) else 0
            p += l if o in (M, EQ, X, D, N) else 0
    bases = np.where(rng.random(len(bases)) < 0.005, rng.integers(0, 4, len(bases)), bases).astype(np.uint8)
    r.update(bases=bases, tid=1, beg=case["rbeg"], end=case["rbeg"] + n_ref, refseq="".join("ACGT"[b] for b in ref[:n_ref]))
    return r
