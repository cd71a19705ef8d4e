"""The input of the microsatellite tests: a 6 kb reference with planted repeats and reads with explicit CIGARs that carry, per planted locus,
every class of InDel the tally distinguishes.  Two arms: `plain` (about 60x, every read its own fragment and family) and `duplex` (UMI
families of 3-5 fragments on both strands, so that the consensus and duplex levels count as well)."""
import numpy as np

N, L, BEG = 6000, 150, 2_000_000
# (region-relative start, unit, copies).  Tracts: at region position 0 and ending on the last base (EDGE); straddling positions 1 024 and
# 2 048 (block seams of a whole-region range); (CA)4 below the default min_units; two tracts back to back; one across a border of RANGES_150.
PLANTS = [(0, "CA", 8), (300, "A", 20), (600, "CA", 12), (900, "AAG", 8), (1012, "CA", 12), (1300, "GATA", 6), (1600, "CA", 4), (1900, "AC", 8), (1916, "TG", 8),
          (2038, "A", 20), (3140, "CA", 12), (N - 16, "CA", 8)]
WITH_EVENTS = [300, 600, 900, 1012, 1300, 1900, 1916, 2038, 3140]


def ranges_150(beg=BEG):
    """40 ranges of 150 bp, one behind the other: range 20 = [3000, 3150) ends inside the (CA)12 planted at 3140"""
    return [(beg + 150 * k, beg + 150 * k + 150) for k in range(40)]


def reference(rng):
    ref = rng.integers(0, 4, N)
    for at, unit, copies in PLANTS:
        u = ["ACGT".index(c) for c in unit]
        ref[at:at + len(u) * copies] = u * copies
        guard = next(b for b in range(4) if b not in (u[0], u[-1]))       # neither side continues the period
        if at > 0 and not any(a + len(w) * c == at for a, w, c in PLANTS):
            ref[at - 1] = guard
        if at + len(u) * copies < N and not any(a == at + len(u) * copies for a, _, _ in PLANTS):
            ref[at + len(u) * copies] = guard
    return ref


def events(ref):
    """(kind, position, length or inserted codes) per planted event: kind 'D' at its first deleted base, 'I' at the base right of the inserted ones"""
    ev = []
    for at, unit, copies in PLANTS:
        if at not in WITH_EVENTS:
            continue
        u, tl = len(unit), len(unit) * copies
        code = ["ACGT".index(c) for c in unit]
        ev += [("D", at + 2 * u, u), ("D", at + u, 2 * u), ("I", at + 3 * u, code),                 # -1, -2, +1 units
               ("D", at + tl - u, 2 * u),                                                          # runs past the end of the tract
               ("I", at + 4 * u, [(c + 1) % 4 for c in code]),                                     # the right length, the wrong bases
               ("I", at + tl, code)]                                                               # behind the last unit
        if u > 1:
            ev.append(("D", at + 3 * u, u + 1))                                                    # no whole number of units
        if at == 300:
            ev.append(("D", at + 5, 7))                                                            # seven units: the tail bin
    ev += [("D", 450, 2), ("I", 470, [2, 3])]                                                      # in plain sequence
    return ev


def build(arm, seed=7):
    """The reads dict of uvc_amd (the UvcReadSoA arrays, refseq, tid, beg, end) of arm 'plain' or 'duplex'"""
    rng = np.random.default_rng(seed)
    ref = reference(rng)
    duplex = (arm == "duplex")
    n_mol = int((30 if duplex else 60) * N / L)
    start = np.sort(rng.integers(0, N - L - 16, n_mol))
    carried = {}                                                          # molecule -> event
    per_event = 2 if duplex else 4
    for e in events(ref):
        kind, p, arg = e
        ln = arg if kind == "D" else len(arg)
        fit = [m for m in np.flatnonzero((start + 14 <= p) & (p + ln + 14 <= start + L)) if m not in carried]
        for m in rng.choice(fit, min(per_event, len(fit)), replace=False):
            carried[int(m)] = e
    pos, flag, nm, frag, fam, strand, cig_rows, bases = [], [], [], [], [], [], [], []
    n_frag = 0
    for m in range(n_mol):
        s = int(start[m])
        if m in carried:
            kind, p, arg = carried[m]
            k = p - s
            if kind == "D":
                b = np.concatenate([ref[s:p], ref[p + arg:p + arg + L - k]])
                cig, mism = [(0, k), (2, arg), (0, L - k)], arg
            else:
                b = np.concatenate([ref[s:p], np.array(arg), ref[p:p + L - k - len(arg)]])
                cig, mism = [(0, k), (1, len(arg)), (0, L - k - len(arg))], len(arg)
        else:
            b, cig, mism = ref[s:s + L], [(0, L)], 0
        assert len(b) == L
        sizes = [int(rng.integers(3, 6)), int(rng.integers(3, 6))] if duplex else ([1, 0] if m % 2 == 0 else [0, 1])
        for sd in range(2):
            for _ in range(sizes[sd]):
                pos.append(BEG + s); flag.append(16 if sd else 0); nm.append(mism); frag.append(n_frag); fam.append(m); strand.append(sd)
                cig_rows.append(cig); bases.append(b)
                n_frag += 1
    n = len(pos)
    n_cigar = np.array([len(c) for c in cig_rows], np.int32)
    cigar_off = np.zeros(n, np.int64)
    cigar_off[1:] = np.cumsum(n_cigar[:-1])
    cigars = np.array([(ln << 4) | op for c in cig_rows for op, ln in c], np.uint32)
    return dict(tid=3, beg=BEG, end=BEG + N, refseq="".join("ACGT"[b] for b in ref), n_reads=n,
                pos=np.array(pos, np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), flag=np.array(flag, np.uint16), mapq=np.full(n, 60, np.uint8),
                nm=np.array(nm, np.int32), l_qseq=np.full(n, L, np.int32), seq_off=np.arange(n, dtype=np.int64) * L, cigar_off=cigar_off, n_cigar=n_cigar,
                frag_id=np.array(frag, np.int32), fam_id=np.array(fam, np.int32), fam_strand=np.array(strand, np.uint8), n_fams=n_mol,
                fam_dflag=np.full(n_mol, 3 if duplex else 0, np.uint8), bases=np.concatenate(bases).astype(np.uint8), quals=np.full(n * L, 36, np.uint8), cigars=cigars)
