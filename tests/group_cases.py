"""Inputs of the family-assignment pass (uvc_amd/csrc/uvc_group.hip) at the places where its kernels can go wrong, written down as data:
block edges of the per-alignment kernels, the 1 024-bin rounds of k_g_scan, the clamp of the second-scan window, every filter reason,
mates on other references, two-strand families, colliding and extreme hash values, and the thresholds of k_g_center.

A case is a function of a sub-case label that returns (params_overrides, cols, fetch_tbeg, fetch_tend); SUBCASES lists the labels.
tests/test_group_shapes_cpu.py checks on the oracle that every case reaches what it is named for, tests/test_gpu_group_shapes.py runs
them through the kernels."""
import functools
import math

import numpy as np

from test_group import py_digest

TB = 100_000
U64 = (1 << 64) - 1
_HASH_COLS = ("umi_kind", "qname_hash31", "qname_hash17", "umi_hash31", "umi_hash17")
_digest = functools.lru_cache(maxsize=None)(py_digest)


def build(rows, overrides=None):
    """rows: (tid, pos, endpos, mtid, mpos, isize, flag, mapq, name) in file order.  overrides: {row index: {hash column: value}} replaces
    what the name's digest gives (umi_kind, qname_hash31, qname_hash17, umi_hash31, umi_hash17).  -> the UvcGroupInput columns."""
    out = {k: np.array([r[j] for r in rows], np.int64) for j, k in enumerate(("tid", "pos", "endpos", "mtid", "mpos", "isize", "flag", "mapq"))}
    d = [dict(zip(_HASH_COLS, _digest(r[8]))) for r in rows]
    for i, o in (overrides or {}).items():
        assert set(o) <= set(_HASH_COLS)
        d[i].update(o)
    out["umi_kind"] = np.array([x["umi_kind"] for x in d], np.uint8)
    for k in _HASH_COLS[1:]:
        out[k] = np.array([x[k] for x in d], np.uint64)
    for v in out.values():
        v.setflags(write=False)
    return out


def aln(cls, t_beg, t_end, name, rl=50, tid=0, mapq=60):
    """One properly paired alignment of the first-scan class `cls` (isrc * 2 + isr2) whose merged template begins at t_beg and ends at
    t_end (the tBeg / tEnd of fill_isrc_isr2_beg_end_with_aln).  Classes 0 and 3 are the two reads of a top-strand pair (t_beg < t_end),
    1 and 2 those of a bottom-strand pair (t_beg > t_end).  The mate is a row of its own, or absent."""
    l, r = min(t_beg, t_end), max(t_beg, t_end)
    assert (t_beg < t_end) == (cls in (0, 3)) and 0 < r - l + 1 < 2000
    flag = {0: 0x1 | 0x2 | 0x20 | 0x40, 3: 0x1 | 0x2 | 0x10 | 0x80, 1: 0x1 | 0x2 | 0x20 | 0x80, 2: 0x1 | 0x2 | 0x10 | 0x40}[cls]
    if flag & 0x10:
        return (tid, r - rl + 1, r + 1, tid, l, -(r - l + 1), flag, mapq, name)
    return (tid, l, l + rl, tid, r - rl + 1, r - l + 1, flag, mapq, name)


def strand_ends(cls, l, r):
    return (l, r) if cls in (0, 3) else (r, l)


def pair(l, r, name, top=True, **kw):
    """both reads of a pair"""
    return [aln(0 if top else 1, *strand_ends(0 if top else 1, l, r), name, **kw), aln(3 if top else 2, *strand_ends(3 if top else 2, l, r), name, **kw)]


def single(pos, rl, name, rev=False, mapq=60, tid=0):
    return (tid, pos, pos + rl, -1, -1, 0, 0x10 if rev else 0, mapq, name)


def random_rows(seed, n_pairs, lo, hi, umi=True):
    """a mixed bag in the style of test_group.make_alignments: pairs of both strands, lone mates, secondary, unmapped and single-end rows"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n_pairs):
        l = max(int(rng.integers(lo, hi)), 0)
        ins = int(rng.integers(120, 420)) if k % 17 else 1700
        name = "r%04d" % k
        if umi and k % 2:
            name += "#" + "ACGT"[k % 4] * 3 + ("+" if k % 3 else "") + "ACGT"[(k // 4) % 4] * 3
        two = pair(l, l + ins - 1, name, top=bool(rng.integers(0, 2)), rl=60, mapq=int(rng.integers(0, 61)))
        rows += two if k % 7 else two[:1]
        if k % 13 == 0:
            rows.append(two[0][:6] + (two[0][6] | 0x100,) + two[0][7:])
        if k % 19 == 0:
            rows.append((0, l, l + 1, -1, -1, 0, 0x4, 0, name))
        if k % 11 == 0:
            rows.append(single(l, 70, "s%04d" % k, rev=bool(k % 2)))
    rows.sort(key=lambda r: r[1])
    return rows


# ---- sizes: the 256-thread block of k_g_pre / k_g_key / k_g_flags / k_g_assign, and nothing or one alignment kept -------------------
def sizes(sub):
    tb, te = TB, TB + 500
    if isinstance(sub, int):
        return {}, build(random_rows(5, 200, tb - 300, te + 100)[:sub]), tb, te
    # the names are visited through alignments that the second scan then drops as outside its window (their own position is far to the
    # right, their template, taken from the mate's position, overlaps the region)
    rows = []
    for k in range(100):
        rows.append((0, te + 2100, te + 2160, 0, tb + 10 + k, 200, 0x1 | 0x2 | 0x20 | 0x40, 60, "v%03d" % k))      # 100
        rows.append((0, tb + 10 + k, tb + 70 + k, -1, -1, 0, 0x4, 0, "v%03d" % k))                                    # 1
        rows.append((0, tb + 10 + k, tb + 70 + k, 0, tb + 150, 200, 0x1 | 0x2 | 0x20 | 0x40 | (0x100 if k % 2 else 0x800), 60, "v%03d" % k))   # 2
    if sub == "one_kept":
        rows[151] = single(tb + 60, 80, "v050")
    else:
        assert sub == "none_kept"
    return {}, build(rows), tb, te


# ---- scan_rounds: the carry of k_g_scan between its rounds of 1 024 bins ---------------------------------------------------------------
PILE = 100            # = dedup_amplicon_border_weak_minDP: a border of 100 is weak-amplicon only while 100 >= tot * 0.05, tot <= 2 000


def _pile(rows, cls, lb, rb, tb, tot, tag):
    """PILE identical alignments of class `cls` between the bins lb < rb, and as many others inside the interval [iL, iR) of the border
    difference as make that difference `tot`.  Classes 0 / 3: [lb + 6, rb - 6), the pile's own ends lie outside; classes 1 / 2: [lb, rb),
    which holds the pile's PILE end counts at lb."""
    pos = lambda b: b - 2000 + tb
    for k in range(PILE):
        rows.append(aln(cls, *strand_ends(cls, pos(lb), pos(rb)), "%s_p%03d" % (tag, k)))
    own = 0 if cls in (0, 3) else PILE
    assert (tot - own) % 2 == 0
    span = rb - lb - 40 - 150
    assert span > 100
    for k in range((tot - own) // 2):
        l = lb + 20 + (k * 13) % span
        rows.append(aln(cls, *strand_ends(cls, pos(l), pos(l + 150)), "%s_n%04d" % (tag, k)))


def scan_rounds(sub):
    """sub = fetch_tend - fetch_tbeg.  One pile per class; its border interval crosses bin 1 024 (classes 0 and 2), 2 048 (class 1) and,
    in class 3, whichever of 2 048, 3 072 and 4 096 lie between the region's end and the last bin OUT_OF_RANGE admits.  tot is 2 002
    where a lost carry makes it smaller (the pile turns amplicon) and 1 998 in class 2 (an excess un-makes it)."""
    tb, te = TB, TB + sub
    rows = []
    _pile(rows, 0, 1000, 2050, tb, 2002, "a")
    _pile(rows, 1, 1500, 2500, tb, 2002, "b")
    _pile(rows, 3, sub + 1995, sub + 3988, tb, 2002, "c")        # oE = fetch_tend + 1988, the highest end that is not OUT_OF_RANGE
    _pile(rows, 2, 11, 1999, tb, 1998, "d")                      # oB = fetch_tbeg - 1989, the lowest
    rows.append(aln(3, tb - 200, tb, "edge"))                    # visited (class 3, below that pile's interval) ...
    rows.append(aln(0, tb - 1990, tb - 1700, "edge"))            # ... so that one bin below the lowest is OUT_OF_RANGE, not 101
    rows.append(aln(3, te + 1700, te + 1989, "edge"))            # and one above the highest
    rows.sort(key=lambda r: r[1])
    return {}, build(rows), tb, te


# ---- low_tbeg: the window of the second scan begins at max(fetch_tbeg - 2001, 0) -------------------------------------------------------
def low_tbeg(sub):
    tb, te = sub, sub + 300
    rows = random_rows(9, 150, 0, tb + 700)
    rows += [single(0, 90, "z0"), single(0, 90, "z0", rev=True), single(0, 2100 if tb > 1000 else 90, "z1")] + pair(0, 250, "z2") + pair(0, 1600, "z3", top=False)
    rows += [single(tb + 10, 90, "z0"), single(tb + 20, 90, "z1"), single(tb + 30, 90, "z2"), single(tb + 40, 90, "z3")]      # all four names visited
    rows.sort(key=lambda r: r[1])
    return {}, build(rows), tb, te


# ---- every_reason -------------------------------------------------------------------------------------------------------------------------
def every_reason(sub=None):
    tb, te = TB, TB + 50
    # the two thresholds act swapped (k_g_pre): kept_aln_min_aln_len bounds the mapping quality, kept_aln_min_mapqual the aligned length
    par = dict(kept_aln_min_aln_len=20, kept_aln_min_mapqual=50, kept_aln_min_isize=120, kept_aln_max_isize=900, kept_aln_is_zero_isize_discarded=1, end2end=1)
    rows = []
    paired = 0x1 | 0x2 | 0x20 | 0x40
    for k in range(60):
        name = "e%02d" % k
        rows += pair(tb - 40 - k % 5, te + 60 + k % 3, name, top=bool(k % 2), rl=60, mapq=20 + k % 30)                      # 0: spans the region
        l = tb - 30
        extra = [(0, l, l + 60, -1, -1, 0, 0x4 | 0x1, 0, name),                            # 1 unmapped
                 (0, l, l + 60, 0, l + 100, 160, paired | 0x800, 60, name),                # 2 supplementary
                 (0, l, l + 60, 0, l + 100, 160, paired, 19, name),                        # 3 quality 19 < 20
                 (0, l, l + 49, 0, l + 100, 160, paired, 60, name),                        # 4 length 49 < 50
                 (0, l, l + 60, 0, l + 59, 119, paired, 60, name),                         # 5 insert 119 < 120
                 (0, l, l + 60, 0, l + 841, 901, paired, 60, name),                        # 6 insert 901 > 900
                 (0, l, l + 60, 0, l + 2500, 2560, paired, 60, name),                      # 7 insert >= 2000 reads as 0
                 (0, tb - 2000, tb - 1940, 0, tb - 1800, 260, paired, 60, name),           # 8 lowest end 1 990 or more before the region
                 (0, tb + 5, tb + 65, 0, tb + 200, 255, paired, 60, name),                 # 9 begins inside the region
                 (0, tb - 2002, tb - 1942, 0, tb - 1800, 262, paired, 60, name)]           # 100 before the second-scan window
        rows.append(extra[k % len(extra)])
        if k % 6 == 0:
            rows += pair(te + 500, te + 800, "f%02d" % k, rl=60)                          # 101: no alignment of the name touches the region
    rows.sort(key=lambda r: r[1])
    return par, build(rows), tb, te


# ---- mates_elsewhere ----------------------------------------------------------------------------------------------------------------------
def mates_elsewhere(sub=None):
    tb, te = TB, TB + 1000
    rows = []
    far = 0x1 | 0x20 | 0x40
    for j in range(3):
        for mtid in (0, 3, 7):       # equal positions, different mate reference: three families; 0 sorts before, 7 after this reference
            rows.append((3, tb + 100, tb + 160, mtid, 5000, 0 if mtid != 3 else -95000, far, 60, "m%d_%d" % (mtid, j)))
            rows.append((3, tb + 300, tb + 360, mtid, tb + 300, 0, far, 60, "q%d_%d" % (mtid, j)))               # mpos == pos
        rows.append((3, tb + 100, tb + 160, -1, -1, 0, 0x1 | 0x8 | 0x40, 60, "u_%d" % j))                        # mate unmapped
        rows.append((3, tb + 100, tb + 160, 3, tb + 100, 0, 0x1 | 0x8 | 0x40, 60, "w_%d" % j))                   # ... placed at the read, as aligners write it
        rows.append((3, tb + 100, tb + 160, -1, 5000, 0, far, 60, "x_%d" % j))                                    # mate flagged mapped, no reference
        rows += pair(tb + 500, tb + 500 + 1499 + j, "i%d" % j, tid=3)                                             # |isize| 1 500 .. 1 502: borders preserved
        rows += pair(tb + 500, tb + 500 + 1498, "j%d" % j, tid=3)                                                 # 1 499: snapped ends
        rows += pair(tb + 520, tb + 520 + 1998, "k%d" % j, tid=3, top=False)                                      # 1 999, bottom strand
        rows.append((3, tb + 600, tb + 660, 3, tb + 2600 + j // 2, 2060 + j // 2, 0x1 | 0x2 | 0x20 | 0x40, 60, "l%d" % j))   # >= 2 000: reads as 0
        rows.append((3, tb + 2600 + j // 2, tb + 2660 + j // 2, 3, tb + 600, -2060 - j // 2, 0x1 | 0x2 | 0x10 | 0x80, 60, "l%d" % j))
        rows.append(single(tb + 100, 60, "s%d" % j, tid=3))
    rows.sort(key=lambda r: r[1])
    return {}, build(rows), tb, te


# ---- duplex_families ----------------------------------------------------------------------------------------------------------------------
def _two_strand(rows, l, r, umi, tag, n_top, n_bot, five=True):
    """top and bottom pairs with the same ends and UMI text, dealt out alternately; the first top name carries five alignments"""
    todo = []
    for j in range(max(n_top, n_bot)):
        if j < n_top:
            todo.append(pair(l, r, "%st%d#%s" % (tag, j, umi), top=True))
        if j < n_bot:
            todo.append(pair(l, r, "%sb%d#%s" % (tag, j, umi), top=False))
    if five:                     # three more alignments under the first top name, away from its first two in the file
        todo.insert(3, pair(l, r, "%st0#%s" % (tag, umi), top=True))
        todo.insert(6, pair(l, r, "%st0#%s" % (tag, umi), top=True)[:1])
    for which in (0, 1):
        rows += [p[which] for p in todo if len(p) > which]


def duplex_families(sub):
    tb = TB
    rows = []
    if sub == "big":             # one family of 5 000 alignments on both strands, over some twenty blocks of the sorted order
        te = tb + 2000
        for k in range(1300):
            rows += pair(tb + 100, tb + 420, "gt%04d#ACGT+TTGA" % k, top=True)
        for k in range(1200):
            rows += pair(tb + 100, tb + 420, "gb%04d#ACGT+TTGA" % k, top=False)
        _two_strand(rows, tb + 700, tb + 1000, "CCC+GGG", "h", 3, 4)
        for k in range(300):
            rows.append(single(tb + 1200 + 2 * k, 60 + k % 3, "o%03d#AC+GT" % k, rev=bool(k % 2)))
        rows.sort(key=lambda r: r[1])
        return {}, build(rows), tb, te
    assert sub == "mixed"
    te = tb + 9200
    _two_strand(rows, tb + 100, tb + 400, "ACGT+TTGA", "d", 4, 3)
    _two_strand(rows, tb + 100, tb + 400, "ACGT+TTGC", "e", 3, 3, five=False)        # the same ends, another UMI
    _two_strand(rows, tb + 120, tb + 430, "ACGT+TTGA", "f", 3, 5, five=False)        # the same UMI, other ends
    umis = ["AAC+GGT", "CCA+TTG", "GGA+CCT", "TTC+AAG", "ACA+GTG", "CAC+TGT", "AGA+CTC", "GAG+TCT"]
    for k in range(600):         # strong begin border, end border split in two: idflag 0x9 (begin + UMI)
        rows += pair(tb + 1000, tb + 1300 + 30 * (k % 2), "p%03d#%s" % (k, umis[k % 8 if k % 16 < 8 else (k + 1) % 8]))
    for k in range(600):         # the mirror: idflag 0xA (end + UMI)
        rows += pair(tb + 2000 + 30 * (k % 2), tb + 2400, "q%03d#%s" % (k, umis[k % 8 if k % 16 < 8 else (k + 1) % 8]))
    for k in range(2000):        # singleton families
        rows.append(single(tb + 3000 + 3 * k, 60 + 3 * (k % 5), "s%04d#%s" % (k, umis[k % 8])))
    rows.sort(key=lambda r: r[1])
    return {}, build(rows), tb, te


# ---- hash_edges ---------------------------------------------------------------------------------------------------------------------------
def hash_edges(sub=None):
    tb, te = TB, TB + 1000
    rows, ov = [], {}

    def add(row, **o):
        if o:
            ov[len(rows)] = o
        rows.append(row)
    one = lambda name: aln(0, tb + 100, tb + 400, name)
    out = lambda name: aln(0, te + 300, te + 600, name)          # inside the second-scan window, not touching the region
    X = 0x1234_5678_9ABC_DEF0
    # one family and strand; A and B share the base-17 hash: one fragment (the reference keys fragments by that hash alone), two visited names
    add(one("A"), qname_hash17=X, qname_hash31=11)
    add(out("C"), qname_hash17=X, qname_hash31=33)               # a third name under the same base-17 hash, never visited: 101
    add(one("B"), qname_hash17=X, qname_hash31=22)
    add(out("A"), qname_hash17=X, qname_hash31=11)               # kept only because the first row visited its name
    add(out("D"), qname_hash17=44, qname_hash31=11)              # A's base-31 hash under another base-17 hash: 101
    edge = [0, U64, 1 << 63, (1 << 63) - 1, 5, (1 << 63) | 5, U64 - 1, 1]
    for rep in range(2):         # fragments of the same family and strand; their order is that of the unsigned 64-bit hash
        for j, h in enumerate(edge):
            add(one("E%d" % j), qname_hash17=h, qname_hash31=edge[(j * 3 + 1) % len(edge)] if j else 0)
    add(aln(1, tb + 400, tb + 100, "E0b"), qname_hash17=0, qname_hash31=0)             # the all-zero name on the other strand as well
    add(aln(1, tb + 400, tb + 100, "E1b"), qname_hash17=U64, qname_hash31=U64)
    add(aln(1, tb + 400, tb + 100, "E0b"), qname_hash17=0, qname_hash31=0)
    two = lambda name: aln(0, tb + 600, tb + 900, name)
    add(two("N1"), umi_kind=1, umi_hash31=0, umi_hash17=0)       # a UMI whose hashes are both 0 ...
    add(two("N2"), umi_kind=0, umi_hash31=0, umi_hash17=0)       # ... is not the absence of a UMI
    add(two("N2b"), umi_kind=0, umi_hash31=7, umi_hash17=9)      # hashes without the UMI bit are not read: with N2
    for kind, u31, u17 in ((1, 7, 9), (1, 7, 10), (1, 8, 9), (3, 7, 9), (1, U64, 1 << 63), (1, U64, (1 << 63) - 1), (1, 7, 9)):
        add(two("N3"), umi_kind=kind, umi_hash31=u31, umi_hash17=u17)                  # one name under different UMI hashes: a family each
    return {}, build(rows, ov), tb, te


# ---- center_thresholds ----------------------------------------------------------------------------------------------------------------------
EXACT_MULTS = (1.5, 2.5, 1.25, 3.0)          # their powers up to the third are exact doubles


def _exact_groups(mult):
    """(locnt, hicnt, d, delta): hicnt + 1 == (locnt + 1) * mult ** d + delta with the smallest locnt that makes the product whole"""
    out = []
    for d in (1, 2, 3):
        p = mult ** d
        lo1 = next(k for k in range(2, 200) if (k * p) == int(k * p))
        for delta in (-1, 0, 1):
            out.append((lo1 - 1, int(lo1 * p) + delta - 1, d, delta))
    return out


def search_inexact(mult, max_lo=130):
    """Pairs on which a power of `mult` that is one ulp off decides differently: for d = 2, 3 and locnt + 1 = 2 .. max_lo, the hicnt + 1
    for which (hicnt + 1) > (locnt + 1) * p is not the same for p = the host's pow(mult, d), p one ulp down and p one ulp up.  These
    are the products that round to a whole number.  -> (locnt, hicnt, d), the first two for d = 2 and the first for d = 3."""
    found = []
    for d, keep in ((2, 2), (3, 1)):
        p = math.pow(mult, d)
        hits = []
        for lo1 in range(2, max_lo + 1):
            for hi1 in range(max(int(lo1 * p) - 1, lo1 + 1), int(lo1 * p) + 3):
                if len({hi1 > lo1 * q for q in (math.nextafter(p, 0.0), p, math.nextafter(p, math.inf))}) > 1:
                    hits.append((lo1 - 1, hi1 - 1, d))
        found += hits[:keep]
    return found


# What search_inexact(1.2) and search_inexact(1.4) find on an x86-64 host with glibc's pow (test_group_shapes_cpu.py runs the search again).
# 1.1 and 1.3 have no such pair below a count of 1 000: their squares need locnt + 1 = 100 * k and round away from the whole number.
INEXACT = {1.2: [(24, 35, 2), (49, 71, 2), (124, 215, 3)],
           1.4: [(24, 48, 2), (49, 97, 2), (124, 342, 3)]}


def rounded_cube(mult):
    """the correctly rounded double of mult ** 3"""
    from fractions import Fraction
    return float(Fraction(mult) ** 3)


def search_host_pow(lo1s, hi1s):
    """Multipliers on which the host's pow(mult, 3) is not the correctly rounded cube (glibc's is an ulp off for about one double in
    1 200) AND the two decide (hicnt + 1) > (locnt + 1) * p differently: for each locnt + 1 and hicnt + 1, the doubles within three ulps
    of the cube root of their quotient.  -> {mult: (locnt, hicnt, 3)}"""
    found = {}
    for lo1 in lo1s:
        for hi1 in hi1s:
            m = (hi1 / lo1) ** (1.0 / 3.0)
            for _ in range(3):
                m = math.nextafter(m, 0.0)
            for _ in range(7):
                a, b = math.pow(m, 3.0), rounded_cube(m)
                if a != b and (hi1 > lo1 * a) != (hi1 > lo1 * b):
                    found[m] = (lo1 - 1, hi1 - 1, 3)
                m = math.nextafter(m, math.inf)
    return found


# The two smallest finds of search_host_pow(range(2, 301), range(3, 901)) below a multiplier of 4, on an x86-64 host with glibc's pow: with
# the first the host's cube is an ulp low and snaps where the rounded cube does not, with the second it is an ulp high and does not snap where
# the rounded cube does.  They hold k_g_center to the power the reference takes, the host's, wherever that and the exact one part.
HOST_POW = {float.fromhex("0x1.b3d4ecb832bbbp+0"): [(60, 300, 3)],        # 1.702467722864397
            float.fromhex("0x1.c44fe6012fbe4p+1"): [(7, 352, 3)]}         # 3.5336883073609773


def center_thresholds(sub):
    """Isolated pairs of bins d apart in the begin and the end histogram of every class.  The reads of both bins share their other end,
    so where the low bin snaps to the high one their two families become one.  No pile may turn amplicon (the read name would enter the
    key and hide the merge): the two minimum depths are out of reach."""
    mult = sub
    tb, te = TB, TB + 1500
    par = dict(dedup_center_mult=mult, dedup_amplicon_border_weak_minDP=1e9, dedup_amplicon_border_strong_minDP=1e9)
    groups = _exact_groups(mult) if mult in EXACT_MULTS else [(lo, hi, d, None) for lo, hi, d in {**INEXACT, **HOST_POW}[mult]]
    rows = []
    for cls in range(4):
        sgn = 1 if cls in (0, 3) else -1
        g = 0
        for hist in ("beg", "end"):
            for locnt, hicnt, d, delta in groups:
                step = d if g % 2 == 0 else -d                                     # the high bin on either side
                base = tb + 20 * g + (0 if hist == "beg" else 1000)
                for cnt, at in ((locnt, base), (hicnt, base + step)):
                    for k in range(cnt):
                        name = "c%d%s%02d_%d_%03d" % (cls, hist[0], g, at - base, k)
                        rows.append(aln(cls, at, base + sgn * 300, name) if hist == "beg" else aln(cls, base - sgn * 300, at, name))
                g += 1
        assert g <= 18
    rows.sort(key=lambda r: r[1])
    return par, build(rows), tb, te


# ---- the registry -------------------------------------------------------------------------------------------------------------------------
CASES = dict(sizes=sizes, scan_rounds=scan_rounds, low_tbeg=low_tbeg, every_reason=every_reason, mates_elsewhere=mates_elsewhere,
             duplex_families=duplex_families, hash_edges=hash_edges, center_thresholds=center_thresholds)
SUBCASES = dict(sizes=[0, 1, 255, 256, 257, "none_kept", "one_kept"], scan_rounds=[76, 77, 1100, 1], low_tbeg=[0, 5, 2001, 2002], every_reason=[None],
                mates_elsewhere=[None], duplex_families=["mixed", "big"], hash_edges=[None], center_thresholds=list(EXACT_MULTS) + sorted(INEXACT) + sorted(HOST_POW))
ALL = [(c, s) for c in CASES for s in SUBCASES[c]]
IDS = ["%s-%s" % (c, s) if s is not None else c for c, s in ALL]


@functools.lru_cache(maxsize=None)
def case(name, sub):
    """built once per process; the columns are read-only"""
    return CASES[name](sub)


_reference = {}


def reference(oracle_lib, name, sub):
    """the oracle's result, computed once per process and shared; nobody writes to it"""
    if (name, sub) not in _reference:
        from uvc_amd import group
        _reference[name, sub] = group.group_families(oracle_lib, *params(oracle_lib, name, sub))
    return _reference[name, sub]


def params(lib, name, sub):
    from uvc_amd import group
    par, cols, tb, te = case(name, sub)
    P = group.default_params(lib, tb, te)
    for k, v in par.items():
        assert hasattr(P, k)
        setattr(P, k, v)
    return P, cols
