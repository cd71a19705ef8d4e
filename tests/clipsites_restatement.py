"""The definitions of uvcgpu_region_clip_sites (include/uvcgpu.h) restated in plain numpy / Python: one per-alignment CIGAR
walk over a reads dict (the columns of UvcReadSoA) and dictionaries keyed by (p, side).  Loads no library; it is the checker of the HIP
kernels and of the report text.  The walk runs once per set of reads and lists every event of every alignment; gates and ranges are
applied to that list."""
import numpy as np

M, I, D, N, S, H, P, EQ, X = range(9)
NTOTAL, NCONS, NCODE, VOTE, ROW = 8, 32, 5, 16, 176
SECTIONS = ["range", "pos", "side", "reads", "reads_fwd", "reads_supp", "reads_secondary", "reads_hard", "len_sum", "len_max", "mapq_sum", "spanning"]
W = {n: i for i, n in enumerate(SECTIONS)}
TOTALS = ["alignments", "events_in_range", "events_off_range", "events_short", "events_at_sites"]
LEFT, RIGHT = 0, 1


def walk(pos, cigar, bases):
    """One alignment: (rend, events); cigar: (op, len) pairs; bases: its query base codes.  An event is (side, p, soft_len, hard_len, c), c
    the query base codes of its S ops in query order; events with len 0 are not listed."""
    aligned = [j for j, (op, ln) in enumerate(cigar) if op in (M, EQ, X)]
    q, p = 0, pos
    ev = {LEFT: [None, 0, 0, []], RIGHT: [None, 0, 0, []]}
    for j, (op, ln) in enumerate(cigar):
        if aligned:
            side = LEFT if j < aligned[0] else RIGHT if j > aligned[-1] else None
            if j == aligned[0]:
                ev[LEFT][0] = p                       # the walk's coordinate at the first aligned op
            if side is not None and op == S:
                ev[side][1] += ln
                ev[side][3] += [int(b) for b in bases[q:q + ln]]
            if side is not None and op == H:
                ev[side][2] += ln
        if op in (M, EQ, X, I, S):
            q += ln
        if op in (M, EQ, X, D, N):
            p += ln
        if aligned and j == aligned[-1]:
            ev[RIGHT][0] = p                          # ... and behind the last one
    return p, [(side, e[0], e[1], e[2], e[3]) for side, e in sorted(ev.items()) if e[1] + e[2] >= 1]


class Restatement:
    def __init__(self, reads):
        self.beg = int(reads["beg"])
        self.npos = int(reads["end"]) - self.beg + 1
        self.alns = []          # per alignment: pos, rend, flag, mapq, l_qseq, events
        cig, bases = np.asarray(reads["cigars"]), np.asarray(reads["bases"])
        for a in range(int(reads["n_reads"])):
            pos, so, co, nc, L = (int(reads[k][a]) for k in ("pos", "seq_off", "cigar_off", "n_cigar", "l_qseq"))
            cigar = [(int(c) & 0xF, int(c) >> 4) for c in cig[co:co + nc]]
            rend, events = walk(pos, cigar, bases[so:so + L])
            self.alns.append((pos, rend, int(reads["flag"][a]), int(reads["mapq"][a]), L, events))

    def run(self, ranges, min_mapq=0, min_clip=10, min_reads=3):
        """-> (totals [8], rows [n_sites, 176], reads [n_reads, 4]: site, read, soft_len, hard_len)"""
        totals = np.zeros(NTOTAL, np.int64)
        which = {}              # position -> index of the range that holds it
        for k, (b, e) in enumerate(ranges):
            for p in range(b, e):
                which[p] = k
        piles, span = {}, np.zeros(self.npos + 1, np.int64)
        for a, (pos, rend, flag, mapq, L, events) in enumerate(self.alns):
            if mapq < min_mapq or (flag & 0x4) or L <= 0:
                continue
            totals[0] += 1
            span[max(pos + 1 - self.beg, 0):max(min(rend - self.beg, self.npos), 0)] += 1     # pos < p < rend
            for side, p, soft, hard, c in events:
                if soft + hard < min_clip:
                    totals[3] += 1
                elif 0 <= p - self.beg < self.npos and p in which:
                    totals[1] += 1
                    piles.setdefault((p, side), []).append((a, soft, hard, c, flag, mapq))
                else:
                    totals[2] += 1
        keys = sorted(k for k, v in piles.items() if len(v) >= min_reads)
        rows, reads = np.zeros((len(keys), ROW), np.int64), []
        for i, (p, side) in enumerate(keys):
            r = rows[i]
            r[W["range"]], r[W["pos"]], r[W["side"]], r[W["spanning"]] = which[p], p, side, span[p - self.beg]
            for a, soft, hard, c, flag, mapq in piles[(p, side)]:
                ln = soft + hard
                r[W["reads"]] += 1
                r[W["reads_fwd"]] += not (flag & 0x10)
                r[W["reads_supp"]] += bool(flag & 0x800)
                r[W["reads_secondary"]] += bool(flag & 0x100)
                r[W["reads_hard"]] += hard > 0
                r[W["len_sum"]] += ln
                r[W["len_max"]] = max(r[W["len_max"]], ln)
                r[W["mapq_sum"]] += mapq
                for k in range(min(soft, NCONS)):
                    base = c[soft - 1 - k] if side == LEFT else c[k]
                    r[VOTE + k * NCODE + (base if 0 <= base <= 3 else 4)] += 1
                reads.append((a, side, i, soft, hard))
            totals[4] += len(piles[(p, side)])
        reads = np.array([(i, a, soft, hard) for a, side, i, soft, hard in sorted(reads)], np.int64).reshape(-1, 4)
        return totals, rows, reads


def consensus(row):
    """(cons_len, cons) of a row: per k the base with the most votes (ties to the smaller code, N for code 4), lower-case iff
    winner * 3 < total * 2; LEFT sites are printed in reference direction (k descending)."""
    vote = np.asarray(row[VOTE:ROW]).reshape(NCONS, NCODE)
    ks = [k for k in range(NCONS) if vote[k].sum() > 0]
    letters = []
    for k in ks:
        c = int(np.argmax(vote[k]))                  # the first of equal maxima
        ch = "ACGTN"[c]
        letters.append(ch.lower() if int(vote[k, c]) * 3 < int(vote[k].sum()) * 2 else ch)
    if int(row[W["side"]]) == LEFT:
        letters.reverse()
    return len(ks), "".join(letters) or "."


S_COLUMNS = "#S\tcontig\tpos\tside\treads\tfwd\tsupp\tsecondary\thard\tlen_sum\tlen_max\tmapq_sum\tspanning\tfragments\tfamilies\tfamilies_both_strands\tcons_len\tcons"
R_COLUMNS = "#R\tcontig\tpos\tside\tqname\tflag\tmapq\tsoft_len\thard_len\tfamily_rank\tstrand"


def report_text(calls, min_mapq, min_clip, min_reads, with_reads, family_columns=True):
    """The file of uvcio_clipsites_write.  calls: (contig id, contig, rows, reads, the reads dict of the call with "qnames") per call; ids of
    families and fragments are local to a call.  family_columns False: the three family columns left out (they depend on the tile cuts)."""
    t = ["##clip_sites_min_mapq=%d" % min_mapq, "##clip_sites_min_clip=%d" % min_clip, "##clip_sites_min_reads=%d" % min_reads, "##clip_sites_reads=%d" % with_reads, S_COLUMNS, R_COLUMNS]
    sites = {}
    for call, (tid, contig, rows, reads, rd) in enumerate(calls):
        for i, row in enumerate(rows):
            ev = [(str(rd["qnames"][a]), int(rd["flag"][a]), int(rd["mapq"][a]), int(soft), int(hard), (call, int(rd["fam_id"][a])), int(rd["fam_strand"][a]), int(rd["frag_id"][a]))
                  for s, a, soft, hard in reads if s == i]
            sites[(tid, int(row[W["pos"]]), int(row[W["side"]]))] = (contig, row, ev)
    for (tid, pos, side), (contig, row, ev) in sorted(sites.items()):
        fams = {}
        for e in ev:
            fams.setdefault(e[5], set()).add(e[6])
        frags = {(e[5], e[6], e[7]) for e in ev}
        n, cons = consensus(row)
        at = "\t%s\t%d\t%s" % (contig, pos + 1, "LR"[side])
        fam_cols = [len(frags), len(fams), sum(1 for s in fams.values() if len(s) == 2)] if family_columns else []
        t.append("S" + at + "\t" + "\t".join(str(int(v)) for v in list(row[W["reads"]:W["spanning"] + 1]) + fam_cols + [n]) + "\t" + cons)
        if with_reads:
            least = {}
            for e in ev:
                least[e[5]] = min(least.get(e[5], (e[0], e[1])), (e[0], e[1]))
            order = sorted(set(least.values()))
            rank = {f: order.index(k) + 1 for f, k in least.items()}
            for e in sorted(ev, key=lambda e: (rank[e[5]], e[0], e[1])):
                t.append("R" + at + "\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (e[0], e[1], e[2], e[3], e[4], rank[e[5]], e[6]))
    return "\n".join(t) + "\n"
