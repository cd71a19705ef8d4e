"""The definitions of uvcgpu_region_clip_mates (include/uvcgpu.h) restated in plain Python: one loop over alignments and
sites, Python sorting and dictionaries.  Loads no library; it is the checker of the HIP kernels and of the P and M lines of the clip-sites
report."""
import numpy as np

import clipsites_restatement as cs

SITE_ROW, ROW, NTOTAL = 8, 12, 8
SITE_WORDS = ["site", "facing", "concordant", "other_contig", "same_strand", "far", "clusters", "clusters_kept"]
CLUSTER_WORDS = ["site", "mtid", "mate_strand", "mpos_min", "mpos_max", "pairs", "other_contig", "same_strand", "far", "mapq_sum", "first", "reserved"]
SW = {n: i for i, n in enumerate(SITE_WORDS)}
CW = {n: i for i, n in enumerate(CLUSTER_WORDS)}
TOTALS = ["pair_reads", "facing", "concordant", "discordant", "clusters", "clusters_kept", "sites_kept"]
CLASSES = ["CONCORDANT", "OTHER_CONTIG", "SAME_STRAND", "FAR"]
CONCORDANT, OTHER_CONTIG, SAME_STRAND, FAR = range(4)
LEFT, RIGHT = cs.LEFT, cs.RIGHT


def endpos(pos, cigar):
    """bam_endpos: pos + the reference length of the CIGAR, pos + 1 without a reference-consuming op"""
    e = pos + sum(ln for op, ln in cigar if op in (cs.M, cs.EQ, cs.X, cs.D, cs.N))
    return e if e > pos else pos + 1


def alignments(reads):
    """per alignment of a reads dict: (pos, rend, mpos, flag, mapq, l_qseq)"""
    cig = np.asarray(reads["cigars"])
    out = []
    for a in range(int(reads["n_reads"])):
        pos, co, nc = (int(reads[k][a]) for k in ("pos", "cigar_off", "n_cigar"))
        cigar = [(int(c) & 0xF, int(c) >> 4) for c in cig[co:co + nc]]
        out.append((pos, endpos(pos, cigar), int(reads["mpos"][a]), int(reads["flag"][a]), int(reads["mapq"][a]), int(reads["l_qseq"][a])))
    return out


def faces(side, p, pos, rend, flag, window, overhang):
    if side == RIGHT:
        return not (flag & 0x10) and pos < p and p - window < rend <= p + overhang
    return bool(flag & 0x10) and rend > p and p - overhang <= pos < p + window


def klass_of(mt, tid, flag, mpos, pos, min_dist):
    if mt != tid:
        return OTHER_CONTIG
    if ((flag >> 5) & 1) == ((flag >> 4) & 1):
        return SAME_STRAND
    return FAR if abs(mpos - pos) >= min_dist else CONCORDANT


def run(reads, rows, mtid, tid, min_mapq=0, window=500, overhang=5, min_dist=1000, max_gap=500, min_pairs=2):
    """-> (totals [8], site rows [n_sites, 8], cluster rows [n_kept, 12], witness rows [n_witnesses, 4]: site, read, cluster, klass).
    rows: site rows of clip_sites (pos and side are read); mtid: per alignment, or None."""
    alns = alignments(reads) if int(reads["n_reads"]) else []
    sites = [(int(r[cs.W["pos"]]), int(r[cs.W["side"]])) for r in rows]
    totals = np.zeros(NTOTAL, np.int64)
    site_rows = np.zeros((len(sites), SITE_ROW), np.int64)
    site_rows[:, SW["site"]] = np.arange(len(sites))
    witnesses = []                      # (site, mt, mate strand, mpos, read, klass, mapq)
    if not sites:                       # a call without sites looks at no read: zero totals
        alns = []
    for a,(pos, rend, mpos, flag, mapq, L) in enumerate(alns):
        mt = tid if mtid is None else int(mtid[a])
        if mapq < min_mapq or (flag & 0x4) or L <= 0 or not (flag & 0x1) or (flag & 0x8) or (flag & 0x900) or mt < 0:
            continue
        totals[0] += 1
        for s, (p, side) in enumerate(sites):
            if not faces(side, p, pos, rend, flag, window, overhang):
                continue
            k = klass_of(mt, tid, flag, mpos, pos, min_dist)
            totals[1] += 1
            totals[2 if k == CONCORDANT else 3] += 1
            site_rows[s, SW["facing"]] += 1
            site_rows[s, SW["concordant"] + k] += 1
            if k != CONCORDANT:
                witnesses.append((s, mt, (flag >> 5) & 1, mpos, a, k, mapq))
    witnesses.sort(key=lambda w: w[:5])
    clusters = []                       # lists of witness indices
    for i, w in enumerate(witnesses):
        p = witnesses[i - 1] if i else None
        if p is None or p[0] != w[0] or p[1] != w[1] or p[2] != w[2] or w[3] - p[3] > max_gap:
            clusters.append([])
        clusters[-1].append(i)
    out, wit = [], np.full((len(witnesses), 4), -1, np.int64)
    for c in clusters:
        ws = [witnesses[i] for i in c]
        s = ws[0][0]
        site_rows[s, SW["clusters"]] += 1
        kept = len(ws) >= min_pairs
        if kept:
            site_rows[s, SW["clusters_kept"]] += 1
            out.append([s, ws[0][1], ws[0][2], min(w[3] for w in ws), max(w[3] for w in ws), len(ws), sum(w[5] == OTHER_CONTIG for w in ws), sum(w[5] == SAME_STRAND for w in ws),
                        sum(w[5] == FAR for w in ws), sum(w[6] for w in ws), c[0], 0])
        for i in c:
            wit[i] = (s, witnesses[i][4], len(out) - 1 if kept else -1, witnesses[i][5])
    totals[4], totals[5], totals[6] = len(clusters), len(out), int((site_rows[:, SW["clusters_kept"]] > 0).sum())
    return totals, site_rows, np.array(out, np.int64).reshape(-1, ROW), wit


P_COLUMNS = "#P\tcontig\tpos\tside\tfacing\tconcordant\tother_contig\tsame_strand\tfar\tclusters\tclusters_kept"
M_COLUMNS = "#M\tcontig\tpos\tside\tmate_contig\tmate_beg\tmate_end\tmate_strand\tpairs\tother_contig\tsame_strand\tfar\tmapq_sum\tfragments\tfamilies\tfamilies_both_strands"


def mate_header(window, overhang, min_dist, max_gap, min_pairs):
    return ["##clip_sites_mate_window=%d" % window, "##clip_sites_mate_overhang=%d" % overhang, "##clip_sites_mate_min_dist=%d" % min_dist, "##clip_sites_mate_max_gap=%d" % max_gap,
            "##clip_sites_mate_min_pairs=%d" % min_pairs]


def mate_lines(contig, contig_names, call, rows, site_rows, clusters, wit, rd, family_columns=True):
    """(tid-less) per site index of one call the P line and the M lines of uvcio_clipsites_write.  rd: the reads dict of the call; `call`
    makes the family ids unique among calls.  family_columns False: the three family columns left out."""
    out = {}
    for i, row in enumerate(rows):
        at = "\t%s\t%d\t%s" % (contig, int(row[cs.W["pos"]]) + 1, "LR"[int(row[cs.W["side"]])])
        lines = ["P" + at + "\t" + "\t".join(str(int(v)) for v in site_rows[i][1:])]
        for c, cl in enumerate(clusters):
            if int(cl[CW["site"]]) != i:
                continue
            ws = [int(w[1]) for w in wit if int(w[2]) == c]
            fams = {}
            for a in ws:
                fams.setdefault((call, int(rd["fam_id"][a])), set()).add(int(rd["fam_strand"][a]))
            frags = {(call, int(rd["fam_id"][a]), int(rd["fam_strand"][a]), int(rd["frag_id"][a])) for a in ws}
            fam_cols = [len(frags), len(fams), sum(1 for s in fams.values() if len(s) == 2)] if family_columns else []
            mt = int(cl[CW["mtid"]])
            name = contig_names[mt] if 0 <= mt < len(contig_names) else "."
            lines.append("M" + at + "\t%s\t%d\t%d\t%s\t" % (name, cl[CW["mpos_min"]] + 1, cl[CW["mpos_max"]] + 1, "+-"[int(cl[CW["mate_strand"]])])
                         + "\t".join(str(int(v)) for v in list(cl[CW["pairs"]:CW["mapq_sum"] + 1]) + fam_cols))
        out[i] = lines
    return out


def report_text(text, calls, contig_names, mates, request, family_columns=True):
    """The file of uvcio_clipsites_write with mates on.  text: the file without them (clipsites_restatement.report_text or
    clipjunctions_restatement.report_text); calls: as those take them; mates: per call (site rows, cluster rows, witness rows) of run();
    request: (window, overhang, min_dist, max_gap, min_pairs)."""
    at = {}
    for call, ((tid, contig, rows, reads, rd), (site_rows, clusters, wit)) in enumerate(zip(calls, mates)):
        for i, lines in mate_lines(contig, contig_names, call, rows, site_rows, clusters, wit, rd, family_columns).items():
            at[(contig, int(rows[i][cs.W["pos"]]) + 1, "LR"[int(rows[i][cs.W["side"]])])] = lines
    src, out = text.splitlines(), []
    for k, line in enumerate(src):
        nxt = src[k + 1] if k + 1 < len(src) else ""
        out.append(line)
        f = line.split("\t")
        if line.startswith("##") and not nxt.startswith("##"):
            out += mate_header(*request)
        elif line.startswith("#") and not line.startswith("##") and not nxt.startswith("#"):
            out += [P_COLUMNS, M_COLUMNS]
        elif (f[0] == "S" and not nxt.startswith("J\t")) or f[0] == "J":
            out += at.get((f[1], int(f[2]), f[3]), [])
    return "\n".join(out) + "\n"
