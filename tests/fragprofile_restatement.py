"""The definitions of uvcgpu_region_fragment_profile (include/uvcgpu.h) restated in numpy from the read columns alone (pos,
cigars, flag, mapq, fam_id, fam_strand, frag_id) and the reference text: the TARGET rows and the profile row of a range list, and the text
of the report (uvcio_fragprofile_write).  Loads no library: the checker of tests/test_gpu_fragprofile.py and tests/test_fragprofile_cpu.py."""
import numpy as np

# the layout, written out (tests/test_fragprofile_cpu.py holds it against include/uvc_fragprofile.def and the header's enums)
TARGET_ROW, NCOUNTER, NLEN, NMOTIF, LEN, FAMLEN, MOTIF, ROW = 8, 16, 1024, 256, 16, 1040, 2064, 2320
PAIRS, OTHERS, SINGLES, LEN_SUM, SHORT, LONG, FAMILIES, RESERVED, FAMILIES_BOTH, ENDS, ENDS_OFF, ENDS_NO_REF = range(12)
TARGET_NAMES = ["pairs", "others", "singles", "len_sum", "short", "long", "families"]
SUMMARY_NAMES = TARGET_NAMES + ["families_both_strands", "ends", "ends_off_region", "ends_no_ref"]
SUMMARY_WORDS = [PAIRS, OTHERS, SINGLES, LEN_SUM, SHORT, LONG, FAMILIES, FAMILIES_BOTH, ENDS, ENDS_OFF, ENDS_NO_REF]
CONTINUES = 1
REF_OPS = (0, 2, 3, 7, 8)   # M D N = X consume the reference
KIND_NONE, KIND_PAIR, KIND_OTHER, KIND_SINGLE = -1, 0, 1, 2
BIG = np.iinfo(np.int64).max


def ref_ends(reads):
    """pos + the reference length of the CIGAR per alignment, exclusive; a CIGAR without a reference-consuming op counts one position."""
    pos = np.asarray(reads["pos"], np.int64)
    cig = np.asarray(reads["cigars"], np.int64)
    n_cigar = np.asarray(reads["n_cigar"], np.int64)
    off = np.asarray(reads["cigar_off"], np.int64) if reads.get("cigar_off") is not None else np.concatenate(([0], np.cumsum(n_cigar)))[:len(pos)]
    ref_len = np.where(np.isin(cig & 0xF, REF_OPS), cig >> 4, 0)
    csum = np.concatenate(([0], np.cumsum(ref_len)))
    return pos + np.maximum(csum[off + n_cigar] - csum[off], 1)


def fragments(reads, min_mapq=0):
    """Per distinct (fam_id, fam_strand, frag_id): dict of int64 arrays fam, strand, nF, nR, loF, hiF, loR, hiR, lo, hi, L, kind."""
    pos, end = np.asarray(reads["pos"], np.int64), ref_ends(reads)
    flag, mapq = np.asarray(reads["flag"], np.int64), np.asarray(reads["mapq"], np.int64)
    fam, strand, frag = np.asarray(reads["fam_id"], np.int64), np.asarray(reads["fam_strand"], np.int64), np.asarray(reads["frag_id"], np.int64)
    counted = (mapq >= min_mapq) & ((flag & 0x904) == 0)
    fwd = (flag & 0x10) == 0
    key = (fam * 2 + strand) * (int(frag.max()) + 1 if len(frag) else 1) + frag
    ids, first, at = np.unique(key, return_index=True, return_inverse=True)
    at = at.reshape(-1)
    ng = len(ids)
    out = dict(fam=fam[first], strand=strand[first])
    for tag, sel in (("F", counted & fwd), ("R", counted & ~fwd)):
        lo, hi = np.full(ng, BIG), np.full(ng, -BIG)
        np.minimum.at(lo, at[sel], pos[sel])
        np.maximum.at(hi, at[sel], end[sel])
        out["n" + tag], out["lo" + tag], out["hi" + tag] = np.bincount(at[sel], minlength=ng).astype(np.int64), lo, hi
    nF, nR = out["nF"], out["nR"]
    out["lo"], out["hi"] = np.minimum(out["loF"], out["loR"]), np.maximum(out["hiF"], out["hiR"])
    some = (nF + nR) > 0
    out["L"] = np.where(some, out["hi"] - out["lo"], 0)
    both = (nF >= 1) & (nR >= 1)
    pair = both & (out["loF"] <= out["loR"]) & (out["hiF"] <= out["hiR"])
    out["kind"] = np.where(~some, KIND_NONE, np.where(pair, KIND_PAIR, np.where(both, KIND_OTHER, KIND_SINGLE)))
    return out


def families(frs):
    """Per sized fam_id (a family with at least one pair fragment): dict of int64 arrays fam, tlo, thi, TL and the bool array both (a pair
    fragment in each strand unit)."""
    pair = frs["kind"] == KIND_PAIR
    fam, strand, lo, hi = frs["fam"][pair], frs["strand"][pair], frs["lo"][pair], frs["hi"][pair]
    ids, at = np.unique(fam, return_inverse=True)
    at = at.reshape(-1)
    nf = len(ids)
    tlo, thi = np.full(nf, BIG), np.full(nf, -BIG)
    np.minimum.at(tlo, at, lo)
    np.maximum.at(thi, at, hi)
    s0, s1 = np.bincount(at[strand == 0], minlength=nf), np.bincount(at[strand != 0], minlength=nf)
    return dict(fam=ids, tlo=tlo, thi=thi, TL=thi - tlo, both=(s0 > 0) & (s1 > 0))


def _select(lo, hi, ranges):
    """(target[i] per range, first): the indices of the objects [lo, hi) under the TARGET rule of each range, and the mask of those under the
    FIRST rule of the call.  Every object is tested against every range by the definitions; so that a million objects and thousands of
    ranges stay affordable the objects are sorted by lo once and a range looks at those with lo in [pos_beg - the longest object, pos_end):
    no other object can overlap it."""
    order = np.argsort(lo, kind="stable")
    slo, shi = lo[order], hi[order]
    longest = int((shi - slo).max()) if len(order) else 0
    first = np.zeros(len(lo), bool)
    target = []
    for q in ranges:
        pos_beg, pos_end = int(q[0]), int(q[1])
        prev_end, flags = (int(q[2]) if len(q) > 2 else pos_beg), (int(q[3]) if len(q) > 3 else 0)
        a, b = np.searchsorted(slo, pos_beg - longest, "left"), np.searchsorted(slo, pos_end, "left")
        wlo, whi, widx = slo[a:b], shi[a:b], order[a:b]
        over = (wlo < pos_end) & (whi > pos_beg)
        target.append(widx[over & ((wlo >= pos_beg) if flags & CONTINUES else True)])
        first[widx[over & (prev_end <= wlo)]] = True
    return target, first


def motif_code(ch):
    return "ACGT".find(ch.upper())


def end_state(refseq, x, right):
    """An end at region offset x (left: its first base; right: one behind its last): ('off', None), ('no_ref', None) or ('ok', motif index)."""
    n = len(refseq)   # positions that hold a reference base
    if (x - 4 < 0 or x > n) if right else (x < 0 or x + 4 > n):
        return "off", None
    sym = [motif_code(refseq[x - 1 - k]) for k in range(4)] if right else [motif_code(refseq[x + k]) for k in range(4)]
    if min(sym) < 0:
        return "no_ref", None
    if right:
        sym = [3 - s for s in sym]
    return "ok", sym[0] * 64 + sym[1] * 16 + sym[2] * 4 + sym[3]


def _ends(prof, refseq, x, right):
    """end_state over an array of offsets, added to the profile"""
    n = len(refseq)
    code = np.array([motif_code(c) for c in refseq] + [-1], np.int64)
    usable = ((x - 4 >= 0) & (x <= n)) if right else ((x >= 0) & (x + 4 <= n))
    x = x[usable]
    sym = np.stack([code[x - 1 - k] if right else code[x + k] for k in range(4)]) if len(x) else np.zeros((4, 0), np.int64)
    acgt = (sym >= 0).all(0)
    sym = (3 - sym[:, acgt]) if right else sym[:, acgt]
    prof[ENDS_OFF] += int((~usable).sum())
    prof[ENDS_NO_REF] += int((~acgt).sum())
    prof[ENDS] += int(acgt.sum())
    np.add.at(prof, MOTIF + sym[0] * 64 + sym[1] * 16 + sym[2] * 4 + sym[3], 1)


def rows_and_profile(frs, fams, ranges, beg, refseq, short=(100, 150), long=(151, 220)):
    """(int64 [len(ranges), TARGET_ROW], int64 [ROW]) straight from the definitions: every fragment and family against every range."""
    rows, prof = np.zeros((len(ranges), TARGET_ROW), np.int64), np.zeros(ROW, np.int64)
    has = frs["kind"] != KIND_NONE
    kind, lo, hi, L = frs["kind"][has], frs["lo"][has], frs["hi"][has], frs["L"][has]
    is_short, is_long = (L >= short[0]) & (L <= short[1]), (L >= long[0]) & (L <= long[1])
    t_frag, f_frag = _select(lo, hi, ranges)
    t_fam, f_fam = _select(fams["tlo"], fams["thi"], ranges)

    def words(sel, n_fam):
        pair = sel[kind[sel] == KIND_PAIR]
        return [len(pair), (kind[sel] == KIND_OTHER).sum(), (kind[sel] == KIND_SINGLE).sum(), L[pair].sum(), is_short[pair].sum(), is_long[pair].sum(), n_fam, 0]
    for i in range(len(ranges)):
        rows[i] = words(t_frag[i], len(t_fam[i]))
    prof[:TARGET_ROW] = words(np.flatnonzero(f_frag), f_fam.sum())
    prof[FAMILIES_BOTH] = (f_fam & fams["both"]).sum()
    pair = f_frag & (kind == KIND_PAIR)
    np.add.at(prof, LEN + np.minimum(L[pair], NLEN - 1), 1)
    np.add.at(prof, FAMLEN + np.minimum(fams["TL"][f_fam], NLEN - 1), 1)
    _ends(prof, refseq, lo[pair] - beg, False)
    _ends(prof, refseq, hi[pair] - beg, True)
    return rows, prof


def header(min_mapq=0, short=(100, 150), long=(151, 220)):
    return ["##fragment_profile=1", "##fragment_profile_min_mapq=%d" % min_mapq, "##fragment_profile_short=%d-%d" % tuple(short), "##fragment_profile_long=%d-%d" % tuple(long),
            "##summary, lengths and end motifs: every fragment and family that overlaps a target, counted once; target lines: every fragment and family that overlaps the target"]


TARGET_HEADER = "#chrom\tbeg\tend\tname\t" + "\t".join(TARGET_NAMES)


def report_text(targets, target_rows, prof, min_mapq=0, short=(100, 150), long=(151, 220)):
    """The text uvcio_fragprofile_write writes: `targets` = (chrom, beg, end, name or None) in order, `target_rows` = per target its summed
    TARGET row (the first 7 values are read), `prof` = the summed profile rows of the run (ROW values)."""
    prof = np.asarray(prof, np.int64)
    t = header(min_mapq, short, long) + ["#summary"] + ["%s\t%d" % (n, prof[w]) for n, w in zip(SUMMARY_NAMES, SUMMARY_WORDS)]
    t.append("#length\tfragments\tfamilies")
    t += ["%d%s\t%d\t%d" % (k, "+" if k == NLEN - 1 else "", prof[LEN + k], prof[FAMLEN + k]) for k in range(NLEN)]
    t.append("#end_motif\tcount")
    t += ["%s\t%d" % ("".join("ACGT"[(m >> s) & 3] for s in (6, 4, 2, 0)), prof[MOTIF + m]) for m in range(NMOTIF)]
    t.append(TARGET_HEADER)
    for (chrom, beg, end, name), r in zip(targets, target_rows):
        t.append("%s\t%d\t%d\t%s\t" % (chrom, beg, end, name or ".") + "\t".join("%d" % int(v) for v in r[:7]))
    return "\n".join(t) + "\n"
