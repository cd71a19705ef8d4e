"""The definitions of uvcgpu_region_family_stats (include/uvcgpu.h) restated in numpy from the read columns alone (pos,
cigars, fam_id, fam_strand, frag_id, fam_dflag): the rows of a range list and the text of the report (uvcio_famstats_write).  Loads no
library: the checker of tests/test_gpu_famstats.py and tests/test_famstats_cli_cpu.py."""
import numpy as np

# the row layout, written out (tests/test_famstats_cli_cpu.py holds it against include/uvc_famstats.def and the header's enums)
TARGET, FIRST, FLAGS, SIZE, NSIZE, STRANDS, CAP, ROW = 0, 4, 8, 12, 64, 76, 16, 365
COUNTERS = ["families", "fragments", "alignments", "families_both_strands"]
FIRST_NAMES = COUNTERS + ["families_umi", "families_duplex_tag", "families_amplicon"]
CONTINUES = 1
REF_OPS = (0, 2, 3, 7, 8)   # M D N = X consume the reference


def ref_ends(reads):
    """pos + the reference length of the CIGAR per alignment, exclusive (a CIGAR without a reference-consuming op counts one position, as
    bam_endpos does)."""
    pos = np.asarray(reads["pos"], np.int64)
    cig = np.asarray(reads["cigars"], np.int64)
    n_cigar = np.asarray(reads["n_cigar"], np.int64)
    off = np.asarray(reads["cigar_off"], np.int64) if reads.get("cigar_off") is not None else np.concatenate(([0], np.cumsum(n_cigar)))[:len(pos)]
    ref_len = np.where(np.isin(cig & 0xF, REF_OPS), cig >> 4, 0)
    csum = np.concatenate(([0], np.cumsum(ref_len)))
    length = csum[off + n_cigar] - csum[off]
    return pos + np.maximum(length, 1)


def families(reads):
    """Per fam_id that has alignments: dict of int64 arrays a, b (fragments of the strand-0 / strand-1 unit), n (alignments), lo, hi, dflag."""
    pos, end = np.asarray(reads["pos"], np.int64), ref_ends(reads)
    fam, strand, frag = np.asarray(reads["fam_id"], np.int64), np.asarray(reads["fam_strand"], np.int64), np.asarray(reads["frag_id"], np.int64)
    ids = np.unique(fam)
    at = np.searchsorted(ids, fam)
    nf = len(ids)
    n = np.bincount(at, minlength=nf)
    lo, hi = np.full(nf, np.iinfo(np.int64).max), np.full(nf, np.iinfo(np.int64).min)
    np.minimum.at(lo, at, pos)
    np.maximum.at(hi, at, end)
    ab = []
    for s in (0, 1):
        pairs = np.unique(np.stack([at[strand == s], frag[strand == s]]), axis=1)   # distinct (family, frag_id) of the unit
        ab.append(np.bincount(pairs[0], minlength=nf))
    return dict(a=ab[0].astype(np.int64), b=ab[1].astype(np.int64), n=n.astype(np.int64), lo=lo, hi=hi, dflag=np.asarray(reads["fam_dflag"], np.int64)[ids])


def rows(fams, ranges):
    """int64 [len(ranges), ROW] for ranges of (pos_beg, pos_end, prev_end, flags), straight from the definitions: every family against every range."""
    out = np.zeros((len(ranges), ROW), np.int64)
    a, b, n, lo, hi, dflag = (fams[k] for k in ("a", "b", "n", "lo", "hi", "dflag"))
    size, both = a + b, (a >= 1) & (b >= 1)
    for i, q in enumerate(ranges):
        pos_beg, pos_end = int(q[0]), int(q[1])
        prev_end, flags = (int(q[2]) if len(q) > 2 else pos_beg), (int(q[3]) if len(q) > 3 else 0)
        over = (lo < pos_end) & (hi > pos_beg)
        t = over & ((lo >= pos_beg) if flags & CONTINUES else True)
        f = over & (prev_end <= lo)
        for base, sel in ((TARGET, t), (FIRST, f)):
            out[i, base:base + 4] = [sel.sum(), size[sel].sum(), n[sel].sum(), (sel & both).sum()]
        out[i, FLAGS:FLAGS + 3] = [(f & ((dflag & bit) != 0)).sum() for bit in (1, 2, 4)]
        np.add.at(out[i], SIZE + np.minimum(size[f], NSIZE) - 1, 1)
        np.add.at(out[i], STRANDS + np.minimum(a[f], CAP) * (CAP + 1) + np.minimum(b[f], CAP), 1)
    return out


def summary_lines(first):
    """name<TAB>value of the #summary section from a FIRST block (a row from word FIRST on, or a whole row)."""
    c = dict(zip(FIRST_NAMES, (int(v) for v in first[FIRST:FIRST + 7])))
    t = ["%s\t%d" % (k, c[k]) for k in FIRST_NAMES]
    t.append("duplication_permille\t%d" % (1000 * (c["fragments"] - c["families"]) // c["fragments"] if c["fragments"] else 0))
    t.append("mean_family_size_x1000\t%d" % (1000 * c["fragments"] // c["families"] if c["families"] else 0))
    t.append("both_strands_permille\t%d" % (1000 * c["families_both_strands"] // c["families"] if c["families"] else 0))
    return t


HEADER = ["##family_stats=1",
          "##summary and histograms: every family that overlaps a target, counted once; target lines: every family that overlaps the target"]
TARGET_HEADER = "#chrom\tbeg\tend\tname\t" + "\t".join(COUNTERS) + "\tmean_family_size_x1000\tboth_strands_permille"


def report_text(targets, target_rows, first):
    """The text uvcio_famstats_write writes: `targets` = (chrom, beg, end, name or None) in order, `target_rows` = per target its summed TARGET
    block (4 values), `first` = the summed rows of the run (ROW values; the FIRST block is read)."""
    first = np.asarray(first, np.int64)
    t = list(HEADER) + ["#summary"] + summary_lines(first) + ["#family_size\tfamilies"]
    t += ["%s\t%d" % (("%d" % (k + 1)) if k + 1 < NSIZE else "%d+" % NSIZE, first[SIZE + k]) for k in range(NSIZE)]
    t.append("#strand0_size\tstrand1_size\tfamilies")
    lab = lambda v: "%d+" % CAP if v == CAP else "%d" % v   # noqa: E731
    t += ["%s\t%s\t%d" % (lab(x), lab(y), first[STRANDS + x * (CAP + 1) + y]) for x in range(CAP + 1) for y in range(CAP + 1) if first[STRANDS + x * (CAP + 1) + y]]
    t.append(TARGET_HEADER)
    for (chrom, beg, end, name), r in zip(targets, target_rows):
        fam, frg, aln, both = (int(v) for v in r[:4])
        t.append("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (chrom, beg, end, name or ".", fam, frg, aln, both, 1000 * frg // fam if fam else 0, 1000 * both // fam if fam else 0))
    return "\n".join(t) + "\n"
