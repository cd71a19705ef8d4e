"""Inputs of the family-concordance tests, placed read by read on an empty region (no random background: every cell of a row is accounted
for).  A Builder lays families out the way set_reads wants them: the reads of a family together, its strand-0 fragments in front of its
strand-1 fragments, the alignments of a fragment together.  tests/test_famconcord_cpu.py computes the rows of the small cases by hand;
tests/test_gpu_famconcord.py compares the HIP path with tests/famconcord_restatement.py on the planted ones."""
import functools

import numpy as np

M, I, D, S = 0, 1, 2, 4
BEG = 1_000_000
_COLS = dict(pos=np.int32, mpos=np.int32, isize=np.int32, flag=np.uint16, mapq=np.uint8, nm=np.int32, l_qseq=np.int32, seq_off=np.int64, cigar_off=np.int64,
             n_cigar=np.int32, frag_id=np.int32, fam_id=np.int32, fam_strand=np.uint8)


class Builder:
    def __init__(self, ref_len, seed, beg=BEG, ref_at=None):
        """ref_at = {offset: base code}: reference bases the case needs at fixed places"""
        self.rng = np.random.default_rng(seed)
        self.ref = self.rng.integers(0, 4, ref_len)
        for off, b in (ref_at or {}).items():
            self.ref[off] = b
        self.beg, self.ref_len = beg, ref_len
        self.cols = {k: [] for k in _COLS}
        self.bases, self.quals, self.cigars, self.fam_dflag = [], [], [], []
        self.frag = -1
        self.ref_n = []

    def family(self, dflag=0):
        self.fam_dflag.append(dflag)
        self._last_strand = 0
        return len(self.fam_dflag) - 1

    def read(self, start, ops, strand=0, mate=False, qual=37, subst=None, quals=None, nm=-1):
        """One alignment of the current family at region offset `start`.  mate: a further alignment of the fragment before it.  subst = {read
        offset: shift}: the base there becomes (reference + shift) % 4 (the read offset counts inserted bases); quals = {read offset: quality}."""
        assert self.fam_dflag and strand >= self._last_strand, "strand-0 fragments come first"
        self._last_strand = strand
        if not mate:
            self.frag += 1
        q, rp = [], start
        for o, l in ops:
            if o == M: q += [int(b) for b in self.ref[rp:rp + l]]; rp += l
            elif o in (I, S): q += [int(b) for b in self.rng.integers(0, 4, l)]
            elif o == D: rp += l
        assert rp <= self.ref_len - 1, "a read ends at or before the region's end - 1"
        for off, sh in (subst or {}).items():
            q[off] = (q[off] + sh) % 4
        ql = [qual] * len(q)
        for off, v in (quals or {}).items():
            ql[off] = v
        app = dict(pos=self.beg + start, mpos=-1, isize=0, flag=(0x10 if strand else 0), mapq=60, nm=nm, l_qseq=len(q), seq_off=len(self.bases), cigar_off=len(self.cigars),
                   n_cigar=len(ops), frag_id=self.frag, fam_id=len(self.fam_dflag) - 1, fam_strand=strand)
        for k, v in app.items():
            self.cols[k].append(v)
        self.bases += q; self.quals += ql; self.cigars += [(l << 4) | o for o, l in ops]
        return len(self.cols["pos"]) - 1

    def reads(self):
        ref = ["ACGT"[b] for b in self.ref]
        for off in self.ref_n:                   # after the reads took their bases from the reference
            ref[off] = "N"
        r = {k: np.array(v, _COLS[k]) for k, v in self.cols.items()}
        r.update(n_reads=len(self.cols["pos"]), tid=3, beg=self.beg, end=self.beg + self.ref_len, refseq="".join(ref), n_fams=len(self.fam_dflag),
                 fam_dflag=np.array(self.fam_dflag, np.uint8), bases=np.array(self.bases, np.uint8), quals=np.array(self.quals, np.uint8), cigars=np.array(self.cigars, np.uint32))
        return r


# ---- the planted region of the GPU tests: every bin edge from both sides, every path of the vote evaluation ----
UNIT_SIZES = (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 33)
PLANTED_LEN = 600


@functools.lru_cache(maxsize=None)
def planted():
    """UMI families of UNIT_SIZES single-read fragments (dflag 0x1, alternating strands), read length 100, laid over a 600 bp region: the first
    starts at the region's first position, the last ends at its last.  In every family fragment 1 (where there is one) dissents at read
    offset 20 and has a quality-0 base at offset 30; families of 4 split 2:2 at offset 40; reference N at two places inside units.  Then a
    family of four with a one-base insertion in one fragment and a three-base deletion in another (InDel reads: the per-alignment path), a
    family of three plain pairs (two alignments per fragment: the register path) of which one mate pair disagrees in the overlap, a lone pair
    and lone single reads."""
    b = Builder(PLANTED_LEN, 71)
    L = 100
    last = PLANTED_LEN - 1 - L                    # a read may end at the region's end - 1
    starts = np.linspace(0, last, len(UNIT_SIZES)).astype(int)
    for n, s in zip(UNIT_SIZES, starts):
        b.family(0x1)
        strand = int(n % 2)
        for k in range(n):
            subst, quals = {}, {}
            if k == 1:
                subst[20] = 1; quals[30] = 0
            if n == 4 and k >= 2:
                subst[40] = 2
            b.read(int(s), [(M, L)], strand=strand, subst=subst, quals=quals)
    b.ref_n += [int(starts[3]) + 50, int(starts[8]) + 10]
    b.family(0x1)                                 # InDel reads in a family
    b.read(130, [(M, 100)]); b.read(130, [(M, 100)])
    b.read(130, [(M, 50), (I, 1), (M, 50)], nm=1); b.read(130, [(M, 40), (D, 3), (M, 57)], nm=3)
    b.family(0x1)                                 # plain pairs
    for k in range(3):
        b.read(300, [(M, 90)], strand=1)
        b.read(350, [(M, 90)], strand=1, mate=True, subst=({5: 1} if k == 2 else {}), quals=({5: 30} if k == 2 else {}))
    b.family(0)
    b.read(420, [(M, 80)]); b.read(470, [(M, 80)], mate=True)
    for s in (5, 64, 127, 256):
        b.family(0)
        b.read(s, [(M, 70)], strand=int(s % 2))
    return b.reads()


@functools.lru_cache(maxsize=None)
def duplex_planted():
    """Duplex families (dflag 0x3, both strands) on a 400 bp region: agreeing strands; a BASE conflict (strand 1 reads another base at offset
    25); a LINK conflict (strand 1 carries a two-base deletion); strands that overlap only partly; a strand without a vote (its two fragments
    tie 1:1 at offset 30); and a family with both strands whose dflag lacks bit 1, which the duplex tallies must not see."""
    b = Builder(400, 72, ref_at={10 + 25: 1})     # a C under the BASE conflict
    L = 80
    b.family(0x3)
    for st in (0, 1):
        b.read(10, [(M, L)], strand=st); b.read(10, [(M, L)], strand=st)
    b.family(0x3)                                 # C on strand 0, T on strand 1
    b.read(10, [(M, L)], strand=0); b.read(10, [(M, L)], strand=0)
    b.read(10, [(M, L)], strand=1, subst={25: 2}); b.read(10, [(M, L)], strand=1, subst={25: 2})
    b.family(0x3)                                 # a deletion on strand 1
    b.read(120, [(M, L)], strand=0); b.read(120, [(M, L)], strand=0)
    b.read(120, [(M, 40), (D, 2), (M, 38)], strand=1, nm=2); b.read(120, [(M, 40), (D, 2), (M, 38)], strand=1, nm=2)
    b.family(0x3)                                 # partial overlap
    b.read(200, [(M, L)], strand=0); b.read(250, [(M, L)], strand=1)
    b.family(0x3)                                 # strand 0 ties 1:1 at offset 30: no vote there
    b.read(300, [(M, L)], strand=0); b.read(300, [(M, L)], strand=0, subst={30: 1})
    b.read(300, [(M, L)], strand=1)
    b.family(0x1)                                 # both strands, no duplex tag
    b.read(150, [(M, L)], strand=0); b.read(150, [(M, L)], strand=1, subst={12: 1})
    return b.reads()
