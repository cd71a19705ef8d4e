"""The definitions of uvcgpu_region_read_profile (include/uvcgpu.h) restated in plain numpy / Python: a per-read CIGAR walk
over a reads dict (the columns of UvcReadSoA) and the reference string.  Loads no library; it is the checker of the HIP kernels and of the
report text.  The walk runs once per set of reads and lists every aligned base and every unaligned event; gates and ranges are applied
to those lists."""
import numpy as np

NCLASS, NQUAL, NCYCLE, NKIND = 4, 64, 256, 5
Q_BINS, CYC_BINS, SUB_BINS, COUNTERS, ROW = 0, 512, 5632, 5696, 5712
COUNTER_NAMES = ["bases_low_mapq", "bases_no_ref", "bases_n", "bases_low_depth", "bases_high_alt", "bases_clean",
                 "positions_no_ref", "positions_low_depth", "positions_high_alt", "positions_clean"]
C = {n: COUNTERS + i for i, n in enumerate(COUNTER_NAMES)}
CLASSES = ["R1_fwd", "R1_rev", "R2_fwd", "R2_rev"]
KINDS = ["match", "mismatch", "ins", "del", "clip"]
NO_REF, LOW_DEPTH, HIGH_ALT, CLEAN = 0, 1, 2, 3
M, I, D, N, S, H, P, EQ, X = range(9)


def read_class(flag):
    return 2 * int((flag & 0x80) != 0) + int((flag & 0x10) != 0)


class Restatement:
    def __init__(self, reads, quals=None):
        self.beg = int(reads["beg"])
        self.npos = int(reads["end"]) - self.beg + 1                 # the region holds positions beg .. end; `end` has no reference base
        ref = np.full(self.npos, 4, np.int64)
        ref[:self.npos - 1] = [{"A": 0, "C": 1, "G": 2, "T": 3}.get(c, 4) for c in reads["refseq"].upper()]
        self.ref = ref
        quals = reads["quals"] if quals is None else quals
        al = [np.zeros((0, 6), np.int64)]    # aligned bases: class, cycle, quality, base, position, mapq
        ev = [np.zeros((0, 5), np.int64)]    # unaligned events: class, cycle, kind, anchor, mapq
        bases, quals = np.asarray(reads["bases"]).astype(np.int64), np.asarray(quals).astype(np.int64)
        for a in range(int(reads["n_reads"])):
            pos, flag, L, mapq = int(reads["pos"][a]), int(reads["flag"][a]), int(reads["l_qseq"][a]), int(reads["mapq"][a])
            if L == 0:
                continue
            so, co, nc = int(reads["seq_off"][a]), int(reads["cigar_off"][a]), int(reads["n_cigar"][a])
            cls, rev = read_class(flag), bool(flag & 0x10)
            cyc = lambda q: (L - 1 - q) if rev else q           # noqa: E731  (q: an index or an array of them)
            q, p = 0, pos
            for cg in reads["cigars"][co:co + nc]:
                op, ln = int(cg) & 0xF, int(cg) >> 4
                k = np.arange(ln)
                if op in (M, EQ, X):
                    al.append(np.stack([np.full(ln, cls), cyc(q + k), quals[so + q:so + q + ln], bases[so + q:so + q + ln], p + k, np.full(ln, mapq)], axis=1))
                    q += ln
                    p += ln
                elif op in (I, S):
                    ev.append(np.stack([np.full(ln, cls), cyc(q + k), np.full(ln, 2 if op == I else 4), np.full(ln, max(pos, p - 1)), np.full(ln, mapq)], axis=1))
                    q += ln
                elif op == D:
                    ev.append(np.array([[cls, cyc(max(0, q - 1)), 3, p, mapq]], np.int64))
                    p += ln
                elif op == N:
                    p += ln
        self.al = np.concatenate(al).astype(np.int64)
        self.ev = np.concatenate(ev).astype(np.int64)
        self._cache = {}

    def status(self, min_mapq, min_depth, max_alt_permille):
        """The status of every position of the region, and D and X."""
        a = self.al
        x = a[:, 4] - self.beg
        ok = (a[:, 5] >= min_mapq) & (x >= 0) & (x < self.npos) & (a[:, 3] <= 3)
        x = x[ok]
        Dp = np.bincount(x, minlength=self.npos)
        Xp = np.bincount(x[a[ok, 3] != self.ref[x]], minlength=self.npos)
        st = np.full(self.npos, CLEAN, np.int64)
        st[Xp * 1000 > max_alt_permille * Dp] = HIGH_ALT
        st[Dp < min_depth] = LOW_DEPTH
        st[self.ref > 3] = NO_REF
        return st, Dp, Xp

    def _gated(self, gate):
        """Per gate, once: the status of every position, and for every aligned base inside the region its position index, the counter it adds
        to wherever a range holds it (the tests in their order) and, where that is bases_clean, its Q, CYC and SUB words; for every event of
        a counted alignment with its anchor inside the region the anchor's index and its CYC word."""
        if gate in self._cache:
            return self._cache[gate]
        min_mapq = gate[0]
        st = self.status(*gate)[0]
        a = self.al
        x = a[:, 4] - self.beg
        keep = (x >= 0) & (x < self.npos)
        a, x = a[keep], x[keep]
        s = st[x]
        cat = np.full(len(a), 5)                            # bases_clean unless an earlier test holds; assigned in reverse order of the tests
        cat[s == HIGH_ALT] = 4
        cat[s == LOW_DEPTH] = 3
        cat[a[:, 3] > 3] = 2
        cat[s == NO_REF] = 1
        cat[a[:, 5] < min_mapq] = 0
        k = (a[:, 3] != self.ref[x]).astype(np.int64)
        qkey = Q_BINS + (a[:, 0] * NQUAL + np.minimum(a[:, 2], NQUAL - 1)) * 2 + k
        ckey = CYC_BINS + (a[:, 0] * NCYCLE + np.minimum(a[:, 1], NCYCLE - 1)) * NKIND + k
        skey = SUB_BINS + a[:, 0] * 16 + np.minimum(self.ref[x], 3) * 4 + np.minimum(a[:, 3], 3)
        e = self.ev
        ex = e[:, 3] - self.beg
        keep = (e[:, 4] >= min_mapq) & (ex >= 0) & (ex < self.npos)
        e, ex = e[keep], ex[keep]
        ekey = CYC_BINS + (e[:, 0] * NCYCLE + np.minimum(e[:, 1], NCYCLE - 1)) * NKIND + e[:, 2]
        self._cache[gate] = (st, x, cat, qkey, ckey, skey, ex, ekey)
        return self._cache[gate]

    def row(self, ranges, min_mapq=0, min_depth=20, max_alt_permille=50):
        st, x, cat, qkey, ckey, skey, ex, ekey = self._gated((min_mapq, min_depth, max_alt_permille))
        inr = np.zeros(self.npos, bool)
        for b, e in ranges:
            inr[b - self.beg:e - self.beg] = True
        row = np.zeros(ROW, np.int64)
        row[C["positions_no_ref"]:C["positions_no_ref"] + 4] = np.bincount(st[inr], minlength=4)    # NO_REF, LOW_DEPTH, HIGH_ALT, CLEAN
        m = inr[x]
        row[C["bases_low_mapq"]:C["bases_low_mapq"] + 6] = np.bincount(cat[m], minlength=6)
        m &= cat == 5
        for key in (qkey, ckey, skey):
            row += np.bincount(key[m], minlength=ROW)
        row += np.bincount(ekey[inr[ex]], minlength=ROW)
        return row


def sections(row):
    """Q [4, 64, 2], CYC [4, 256, 5], SUB [4, 4, 4] and the 16 counters of a row."""
    return (row[Q_BINS:CYC_BINS].reshape(NCLASS, NQUAL, 2), row[CYC_BINS:SUB_BINS].reshape(NCLASS, NCYCLE, NKIND),
            row[SUB_BINS:COUNTERS].reshape(NCLASS, 4, 4), row[COUNTERS:ROW])


def check_identities(row, n_positions):
    """What holds on every row: per class the Q, SUB and CYC match + mismatch sums agree, bases_clean is their total, the positions_*
    counters sum to the length of the ranges, the reserved words are 0."""
    q, cyc, sub, cnt = sections(np.asarray(row))
    for c in range(NCLASS):
        assert q[c].sum() == sub[c].sum() == cyc[c, :, 0:2].sum(), c
    assert row[C["bases_clean"]] == q.sum()
    assert sub[:, np.arange(4), np.arange(4)].sum() == q[:, :, 0].sum()
    assert cnt[6:10].sum() == n_positions
    assert not cnt[10:].any()


def report_text(row, min_mapq, min_depth, max_alt_permille):
    """The file of uvcio_readprofile_write for the summed row."""
    q, cyc, sub, cnt = sections(np.asarray(row))
    t = ["##read_profile_min_mapq=%d" % min_mapq, "##read_profile_min_depth=%d" % min_depth, "##read_profile_max_alt_permille=%d" % max_alt_permille,
         "##empirical_quality=-10*log10((mismatch+1)/(match+mismatch+2))", "#counter\tcount"]
    t += ["%s\t%d" % (n, cnt[i]) for i, n in enumerate(COUNTER_NAMES)]
    t.append("#class\tquality\tmatch\tmismatch")
    t += ["%s\t%d\t%d\t%d" % (CLASSES[c], b, q[c, b, 0], q[c, b, 1]) for c in range(NCLASS) for b in range(NQUAL) if q[c, b].any()]
    t.append("#class\tcycle\tmatch\tmismatch\tins\tdel\tclip")
    t += ["%s\t%d\t%s" % (CLASSES[c], b, "\t".join(str(int(v)) for v in cyc[c, b])) for c in range(NCLASS) for b in range(NCYCLE) if cyc[c, b].any()]
    t.append("#class\tref\tread\tcount")
    t += ["%s\t%s\t%s\t%d" % (CLASSES[c], "ACGT"[r], "ACGT"[b], sub[c, r, b]) for c in range(NCLASS) for r in range(4) for b in range(4) if sub[c, r, b]]
    return "\n".join(t) + "\n"
