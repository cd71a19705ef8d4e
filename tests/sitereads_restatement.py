"""The definitions of uvcgpu_region_site_reads (include/uvcgpu.h) restated in plain numpy / Python: a per-alignment CIGAR walk
over a reads dict (the columns of UvcReadSoA) and the reference string.  Loads no library; it is the checker of the HIP kernels.  The walk
runs once per set of reads and lists every observation an alignment has at any position, with the events anchored there; a site list, the
mapq gate and alt_only select from that list."""
import numpy as np

KINDS = ["A", "C", "G", "T", "N", "DEL"]
DEL = 5
NCOL, COL_INS, COL_DEL_AFTER = 8, 6, 7
FIELDS = ["site", "read", "q", "obs", "ins_q", "ins_len", "del_len", "reserved"]
ROW = np.dtype([(n, np.int32) for n in FIELDS])
M, I, D, N, S, H, P, EQ, X = range(9)


class Restatement:
    def __init__(self, reads, quals=None):
        self.beg = int(reads["beg"])
        self.npos = int(reads["end"]) - self.beg + 1                 # the region holds positions beg .. end; `end` has no reference base
        ref = np.full(self.npos, 4, np.int64)
        ref[:self.npos - 1] = [{"A": 0, "C": 1, "G": 2, "T": 3}.get(c, 4) for c in reads["refseq"].upper()]
        self.ref = ref
        quals = reads["quals"] if quals is None else quals
        bases, quals = np.asarray(reads["bases"]).astype(np.int64), np.asarray(quals).astype(np.int64)
        out = [np.zeros((0, 9), np.int64)]   # read, position, q, kind, quality, ins_q, ins_len, del_len, mapq
        for a in range(int(reads["n_reads"])):
            pos, L, mapq = int(reads["pos"][a]), int(reads["l_qseq"][a]), int(reads["mapq"][a])
            if L == 0:
                continue
            so, co, nc = int(reads["seq_off"][a]), int(reads["cigar_off"][a]), int(reads["n_cigar"][a])
            q, p = 0, pos
            obs, events = [], []                                     # events: (anchor, is insertion, length, query index)
            for cg in reads["cigars"][co:co + nc]:
                op, ln = int(cg) & 0xF, int(cg) >> 4
                k = np.arange(ln)
                if op in (M, EQ, X):
                    b = bases[so + q:so + q + ln]
                    obs.append(np.stack([p + k, q + k, np.where(b <= 3, b, 4), quals[so + q:so + q + ln]], axis=1))
                    q += ln
                    p += ln
                elif op == I:
                    events.append((p - 1, True, ln, q))
                    q += ln
                elif op == S:
                    q += ln
                elif op == D:
                    qe = max(0, q - 1)
                    obs.append(np.stack([p + k, np.full(ln, qe), np.full(ln, DEL), np.full(ln, quals[so + qe])], axis=1))
                    events.append((p - 1, False, ln, q))
                    p += ln
                elif op == N:
                    p += ln
            if not obs:
                continue
            o = np.concatenate(obs)
            t = np.zeros((len(o), 9), np.int64)
            t[:, 0], t[:, 1:5], t[:, 5], t[:, 8] = a, o, -1, mapq
            for anchor, ins, ln, qi in events:                       # an event attaches to the observation at its anchor, if there is one
                at = int(np.searchsorted(t[:, 1], anchor))
                if at < len(t) and t[at, 1] == anchor:
                    if ins:
                        if t[at, 6] == 0:
                            t[at, 5] = qi
                        t[at, 6] += ln
                    else:
                        t[at, 7] += ln
            out.append(t)
        self.obs = np.concatenate(out)

    def site_reads(self, sites, min_mapq=0, alt_only=0):
        """-> (rows, counts) as uvcgpu_region_site_reads returns them."""
        sites = np.asarray(sites, np.int64)
        assert len(sites) >= 1 and (np.diff(sites) > 0).all() and sites[0] >= self.beg and sites[-1] < self.beg + self.npos
        t = self.obs
        index_of = np.full(self.npos, -1, np.int64)                 # position -> its index in `sites`
        index_of[sites - self.beg] = np.arange(len(sites))
        x = t[:, 1] - self.beg
        at = np.where((x >= 0) & (x < self.npos), index_of[np.clip(x, 0, self.npos - 1)], -1)
        sel = (t[:, 8] >= min_mapq) & (at >= 0)
        t, at = t[sel], at[sel]
        counts = np.zeros((len(sites), NCOL), np.int64)
        np.add.at(counts, (at, t[:, 3]), 1)
        np.add.at(counts[:, COL_INS], at[t[:, 6] > 0], 1)
        np.add.at(counts[:, COL_DEL_AFTER], at[t[:, 7] > 0], 1)
        if alt_only:
            ref = self.ref[t[:, 1] - self.beg]
            keep = (t[:, 3] == DEL) | (t[:, 6] > 0) | (t[:, 7] > 0) | ((t[:, 3] <= 3) & (ref <= 3) & (ref != t[:, 3]))
            t, at = t[keep], at[keep]
        rows = np.zeros(len(t), ROW)
        rows["site"], rows["read"], rows["q"], rows["obs"] = at, t[:, 0], t[:, 2], t[:, 3] | (t[:, 4] << 8)
        rows["ins_q"], rows["ins_len"], rows["del_len"] = t[:, 5], t[:, 6], t[:, 7]
        return rows, counts.astype(np.int32)
