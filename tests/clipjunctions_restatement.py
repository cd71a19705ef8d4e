"""The definitions of uvcgpu_region_clip_junctions (include/uvcgpu.h) restated in plain numpy / Python: a brute-force loop
over t, strand and k.  Loads no library; it is the checker of the HIP kernels (both builds) and of the J lines of the clip-sites report."""
import numpy as np

import clipsites_restatement as cs

ROW, NTOTAL, NHIST = 24, 8, 8
SECTIONS = ["site", "query_len", "cmp_len", "status", "best_mm", "n_best", "second_mm", "partner", "strand", "klass", "len", "mate"]
W = {n: i for i, n in enumerate(SECTIONS)}
HIST = 12
TOTALS = ["sites", "searched", "placed", "unique", "mated"]
NOT_SEARCHED, NOT_PLACED, PLACED = 0, 1, 2
CLASSES = ["NONE", "DEL", "DUP", "INV", "ADJACENT"]
NONE, DEL, DUP, INV, ADJACENT = range(5)
LEFT, RIGHT = cs.LEFT, cs.RIGHT
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def ref_codes(refseq):
    """The reference as codes: 0..3 for A C G T (either case), 4 for everything else."""
    return [CODE.get(ch, 4) for ch in (refseq.decode() if isinstance(refseq, bytes) else refseq).upper()]


def query(row, min_votes):
    """(query_len, q): q[k] = the winner of k where k is compared, None elsewhere."""
    vote = np.asarray(row[cs.VOTE:cs.ROW]).reshape(cs.NCONS, cs.NCODE)
    qlen, q = 0, []
    for k in range(cs.NCONS):
        total, win = int(vote[k].sum()), int(np.argmax(vote[k]))     # the first of equal maxima: the smaller code
        if total >= 1:
            qlen = k + 1
        q.append(win if total >= min_votes and win <= 3 and int(vote[k, win]) * 3 >= total * 2 else None)
    return qlen, q


def partner_of(side, strand, t):
    """(partner plane index, the side of the mate)"""
    if strand == 0:
        return (t, LEFT) if side == RIGHT else (t + 1, RIGHT)
    return (t + 1, RIGHT) if side == RIGHT else (t, LEFT)


def run(refseq, beg, rows, min_votes=2, min_len=16, max_mismatch=1, max_dist=0, mate_slop=10):
    """-> (totals [8], junction rows [n_sites, 24]).  refseq: the n = npos - 1 reference characters of the region; rows: site rows."""
    ref = np.array(ref_codes(refseq), np.int64)
    n = len(ref)
    out = np.zeros((len(rows), ROW), np.int64)
    totals = np.zeros(NTOTAL, np.int64)
    totals[0] = len(rows)
    for s, row in enumerate(rows):
        pos, side = int(row[cs.W["pos"]]), int(row[cs.W["side"]])
        qlen, q = query(row, min_votes)
        cmp_len = sum(c is not None for c in q)
        o = out[s]
        o[:] = 0
        o[W["site"]], o[W["query_len"]], o[W["cmp_len"]] = s, qlen, cmp_len
        for name in ("best_mm", "second_mm", "partner", "strand", "len", "mate"):
            o[W[name]] = -1
        if cmp_len < min_len:
            continue
        totals[1] += 1
        o[W["status"]] = NOT_PLACED
        d = 1 if side == RIGHT else -1
        hist, best = [0] * NHIST, None
        for strand in (0, 1):
            e = d if strand == 0 else -d
            # every t whose query_len faced positions t + e k lie in [0, n); the loop over k runs over all of them at once
            ts = np.arange(n)
            ts = ts[(ts + e * (qlen - 1) >= 0) & (ts + e * (qlen - 1) < n)]
            mms = np.zeros(len(ts), np.int64)
            for k in range(qlen):
                if q[k] is None:
                    continue
                r = ref[ts + e * k]
                mms += (r > 3) | ((r if strand == 0 else 3 - r) != q[k])
            for t, mm in zip(ts[mms <= max_mismatch].tolist(), mms[mms <= max_mismatch].tolist()):
                px, _ = partner_of(side, strand, t)
                if max_dist > 0 and abs(px + beg - pos) > max_dist:
                    continue
                hist[mm] += 1
                if best is None or (mm, strand, t) < best:
                    best = (mm, strand, t)
        o[HIST:HIST + NHIST] = hist
        if best is None:
            continue
        mm, strand, t = best
        px, mate_side = partner_of(side, strand, t)
        partner = px + beg
        later = [m for m in range(mm + 1, NHIST) if hist[m]]
        o[W["status"]], o[W["best_mm"]], o[W["n_best"]], o[W["partner"]], o[W["strand"]], o[W["len"]] = PLACED, mm, hist[mm], partner, strand, abs(partner - pos)
        o[W["second_mm"]] = mm if hist[mm] >= 2 else later[0] if later else -1
        if strand == 1:
            o[W["klass"]] = INV
        elif partner == pos:
            o[W["klass"]] = ADJACENT
        else:
            o[W["klass"]] = DEL if (partner > pos) == (side == RIGHT) else DUP
        cands = sorted((abs(int(r2[cs.W["pos"]]) - partner), int(r2[cs.W["pos"]]), i) for i, r2 in enumerate(rows)
                       if int(r2[cs.W["side"]]) == mate_side and abs(int(r2[cs.W["pos"]]) - partner) <= mate_slop)
        o[W["mate"]] = cands[0][2] if cands else -1
        totals[2] += 1
        totals[3] += hist[mm] == 1
        totals[4] += bool(cands)
    return totals, out


J_COLUMNS = "#J\tcontig\tpos\tside\tquery_len\tcmp_len\tstatus\tbest_mm\tn_best\tsecond_mm\tpartner_pos\tstrand\tclass\tlen\tmate_pos\tmate_side"


def j_line(contig, row, jrow, rows):
    """The J line of one site: row its site row, jrow its junction row, rows the site rows of the same call (the mate indexes them)."""
    dot = lambda v: "." if v < 0 else str(int(v))                                     # noqa: E731
    placed = int(jrow[W["status"]]) == PLACED
    mate = int(jrow[W["mate"]])
    f = ["J", contig, str(int(row[cs.W["pos"]]) + 1), "LR"[int(row[cs.W["side"]])], str(int(jrow[W["query_len"]])), str(int(jrow[W["cmp_len"]])), str(int(jrow[W["status"]])),
         dot(jrow[W["best_mm"]]), str(int(jrow[W["n_best"]])), dot(jrow[W["second_mm"]]),
         str(int(jrow[W["partner"]]) + 1) if placed else ".", "+-"[int(jrow[W["strand"]])] if placed else ".", CLASSES[int(jrow[W["klass"]])], dot(jrow[W["len"]]),
         str(int(rows[mate][cs.W["pos"]]) + 1) if mate >= 0 else ".", "LR"[int(rows[mate][cs.W["side"]])] if mate >= 0 else "."]
    return "\t".join(f)


def report_text(calls, min_mapq, min_clip, min_reads, with_reads, junctions=None, request=None, family_columns=True):
    """The file of uvcio_clipsites_write.  calls: as clipsites_restatement.report_text takes them.  junctions: None (today's text) or one
    array of junction rows per call; request: (min_votes, min_len, max_mismatch, max_dist, mate_slop)."""
    text = cs.report_text(calls, min_mapq, min_clip, min_reads, with_reads, family_columns)
    if junctions is None:
        return text
    j = {}
    for (tid, contig, rows, reads, rd), jrows in zip(calls, junctions):
        for row, jrow in zip(rows, jrows):
            j[(contig, int(row[cs.W["pos"]]) + 1, "LR"[int(row[cs.W["side"]])])] = j_line(contig, row, jrow, rows)
    out = []
    for line in text.splitlines():
        out.append(line)
        f = line.split("\t")
        if line.startswith("##clip_sites_reads="):
            out += ["##clip_sites_junction_%s=%d" % (name, v) for name, v in zip(("min_votes", "min_len", "max_mismatch", "max_dist", "slop"), request)]
        elif line == cs.R_COLUMNS:
            out.append(J_COLUMNS)
        elif f[0] == "S":
            out.append(j[(f[1], int(f[2]), f[3])])
    return "\n".join(out) + "\n"
