"""A numpy restatement of the microsatellite tally (uvcgpu_region_msi, uvcio_msi_*, uvc1-mi355x --msi-out), written from the definitions in
uvcgpu.h alone and fed by public calls only: the STR planes of Region.fetch("RTR"), the four depth measures summed from fetched planes, the
rows of Region.indel_alleles() and the reference text.  It loads no library.

Positions x are region-relative.  A locus head h inside some range: RTR_begpos[h] == h, 1 <= RTR_unitlen[h] <= max_unitlen,
RTR_tracklen[h] >= min_tracklen, RTR_tracklen[h] // RTR_unitlen[h] >= min_units.  EDGE: h == 0 or h + tracklen >= npos - 1; such a locus
keeps zeros.  depth = the minimum over the tract of bDP, cDP12, cDP2, dDP1.  An allele row (refpos, symbol, strand, len, seq, bAD1, cAD1,
c2AD, c2dAD) adds its four counters to one bin of one locus: a deletion at x to h = RTR_begpos[x], bin -len / unit iff len % unit == 0 and
x + len <= h + tracklen; an insertion at q = x to h = RTR_begpos[q] if that is a reported locus, else (q > 0) to h = RTR_begpos[q - 1] if
that is a reported locus whose tract ends at q, bin +len / unit iff len % unit == 0 and seq[i] == ref[h + (q - h + i) % unit] for all i;
anything else of a hit locus is OTHER; shifts beyond 6 units go to the -6 / +6 bins."""
import numpy as np

ROW, DEPTH, HIST, NLEVEL, NBIN, OTHER, MAXSHIFT, EDGE = 64, 5, 9, 4, 13, 12, 6, 1
LEVELS = ["b", "c", "c2", "d"]
DEL_SYMBOLS, INS_SYMBOLS = (7, 8, 9), (10, 11, 12)      # LINK_D3P D2 D1, LINK_I3P I2 I1


def bin_of(shift_units):
    """the histogram bin of a shift by whole units (negative: deletion)"""
    s = max(-MAXSHIFT, min(MAXSHIFT, shift_units))
    return s + MAXSHIFT if s < 0 else s + MAXSHIFT - 1


def ref_codes(refseq):
    """A C G T (either case) -> 0..3, anything else 4"""
    lut = np.full(256, 4, np.uint8)
    for k, ch in enumerate("ACGT"):
        lut[ord(ch)] = lut[ord(ch.lower())] = k
    return lut[np.frombuffer(refseq.encode() if isinstance(refseq, str) else bytes(refseq), np.uint8)]


def loci_of(rtr, beg, ranges, min_tracklen=10, min_units=5, max_unitlen=6):
    """rows [n][64] with the header words filled: the loci of `ranges` ((pos_beg, pos_end) pairs, sorted, disjoint) of STR planes
    rtr [>= 3][npos] whose column 0 is position `beg`"""
    begpos, tracklen, unitlen = (np.asarray(rtr[k], np.int64) for k in range(3))
    npos = len(begpos)
    is_head = (begpos == np.arange(npos)) & (unitlen >= 1) & (unitlen <= max_unitlen) & (tracklen >= min_tracklen) & (tracklen // np.maximum(unitlen, 1) >= min_units)
    rows = []
    for i, (a, b) in enumerate(ranges):
        h = (a - beg) + np.flatnonzero(is_head[a - beg:b - beg])
        part = np.zeros((len(h), ROW), np.int32)
        part[:, 0], part[:, 1], part[:, 2], part[:, 3] = i, beg + h, tracklen[h], unitlen[h]
        part[:, 4] = np.where((h == 0) | (h + tracklen[h] >= npos - 1), EDGE, 0)
        rows.append(part)
    return np.concatenate(rows) if rows else np.zeros((0, ROW), np.int32)


def tally(rtr, beg, ranges, measures4, alleles, refseq, min_tracklen=10, min_units=5, max_unitlen=6):
    """The rows of uvcgpu_region_msi.  measures4: int [4][npos] = bDP, cDP12, cDP2, dDP1 per position; alleles: the dicts of
    Region.indel_alleles(); refseq: the reference text of the region from `beg` on.  Returns (rows, classes): classes counts how many allele
    rows fell into each class of attribution, for the self-checks of the tests."""
    rows = loci_of(rtr, beg, ranges, min_tracklen, min_units, max_unitlen)
    begpos = np.asarray(rtr[0], np.int64)
    npos = len(begpos)
    ref = ref_codes(refseq)
    index = {int(r[1]) - beg: k for k, r in enumerate(rows)}
    for r in rows:
        if not r[4] & EDGE:
            h, tl = int(r[1]) - beg, int(r[2])
            r[DEPTH:DEPTH + NLEVEL] = np.asarray(measures4)[:, h:h + tl].min(1)
    classes = dict(no_locus=0, edge=0, unit_del=0, unit_ins=0, tail=0, del_past_end=0, non_multiple=0, wrong_bases=0, behind_last_unit=0)
    for al in alleles:
        x, ln = al["refpos"] - beg, al["len"]
        is_del, is_ins = al["symbol"] in DEL_SYMBOLS, al["symbol"] in INS_SYMBOLS
        counts = [al["bAD1"], al["cAD1"], al["c2AD"], al["c2dAD"]]
        if not (is_del or is_ins) or ln < 1 or x < 0 or x >= npos or not any(counts):
            continue
        k = index.get(int(begpos[x]))
        behind = False
        if is_ins and k is None and x > 0:
            k = index.get(int(begpos[x - 1]))
            if k is not None and int(rows[k][1]) - beg + int(rows[k][2]) != x:
                k = None
            behind = k is not None
        if k is None:
            classes["no_locus"] += 1
            continue
        r = rows[k]
        if r[4] & EDGE:
            classes["edge"] += 1
            continue
        h, tl, ul = int(r[1]) - beg, int(r[2]), int(r[3])
        if ln % ul != 0:
            b = OTHER
            classes["non_multiple"] += 1
        elif is_del and x + ln > h + tl:
            b = OTHER
            classes["del_past_end"] += 1
        elif is_ins and any("ACGTN".index(ch) != ref[h + (x - h + i) % ul] for i, ch in enumerate(al["seq"])):
            b = OTHER
            classes["wrong_bases"] += 1
        else:
            b = bin_of(-(ln // ul) if is_del else ln // ul)
            classes["unit_del" if is_del else "unit_ins"] += 1
            classes["tail"] += ln // ul > MAXSHIFT
            classes["behind_last_unit"] += behind
        for lv in range(NLEVEL):
            r[HIST + lv * NBIN + b] += counts[lv]
    return rows, classes


def report_text(targets, loci_per_target, min_tracklen=10, min_units=5, max_unitlen=6, min_depth=30, unstable_permille=200):
    """targets: (chrom, beg, end, name or None); loci_per_target: per target the (row, unit text) pairs of its loci, in any order"""
    text = ("##msi_loci=1\n"
            "## A tally for a downstream classifier that has a baseline, NOT an MSI call: per microsatellite of the caller's own repeat tracks the\n"
            "## smallest depth along the tract and the InDel alleles that change its length by whole units (shifted) or otherwise (other), per\n"
            "## evidence level: b fragments, c UMI families, c2 consensus families, d duplex families.  A heterozygous germline length allele counts\n"
            "## as shifted.  EDGE: the tract touches the end of the region it was seen in; nothing was counted.\n")
    text += "#min_tract\t%d\n#min_units\t%d\n#max_unit\t%d\n#min_depth\t%d\n#unstable_permille\t%d\n" % (min_tracklen, min_units, max_unitlen, min_depth, unstable_permille)
    shifts = ["m%d" % s for s in range(MAXSHIFT, 0, -1)] + ["p%d" % s for s in range(1, MAXSHIFT + 1)]
    text += "\t".join(["#chrom", "beg", "end", "unit", "unitlen", "units", "target", "flags"] + ["%s_%s" % (lv, c) for lv in LEVELS for c in ["depth", "shifted", "other"] + shifts]) + "\n"
    n, n_edge, assessable, unstable = 0, 0, [0] * NLEVEL, [0] * NLEVEL
    for (chrom, _, _, name), loci in zip(targets, loci_per_target):
        for row, unit in sorted(loci, key=lambda q: int(q[0][1])):
            row = [int(v) for v in row]
            edge = bool(row[4] & EDGE)
            cols = [chrom, row[1], row[1] + row[2], unit, row[3], row[2] // row[3], name or ".", "EDGE" if edge else "."]
            for lv in range(NLEVEL):
                h = row[HIST + lv * NBIN:HIST + (lv + 1) * NBIN]
                depth, shifted = row[DEPTH + lv], sum(h[:OTHER])
                cols += [depth, shifted, h[OTHER]] + h[:OTHER]
                if not edge and depth >= min_depth:
                    assessable[lv] += 1
                    unstable[lv] += 1000 * shifted >= unstable_permille * depth
            text += "\t".join(str(c) for c in cols) + "\n"
            n += 1
            n_edge += edge
    text += "#summary\tloci\t%d\n#summary\tloci_EDGE\t%d\n" % (n, n_edge)
    return text + "".join("#summary\t%s\tassessable\t%d\tunstable\t%d\n" % (LEVELS[lv], assessable[lv], unstable[lv]) for lv in range(NLEVEL))
