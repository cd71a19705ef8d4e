"""Inputs of tests/test_gpu_misq.py and tests/test_misq_cpu.py, and a numpy restatement of the mismatch queue of the accumulate.

The queue (RegionDev::mis, read by k_p2_mism) holds one item per base of a work-list entry that differs from the reference.  An entry is a
simple alignment or an M run of an InDel read whose InDels are all high-quality (edge_reads.classify: kinds 0 and 2; a read of kind 1 goes
through the per-read kernels and is not on the list).  In the plain form of P2 an item is (rank of the alignment, position, symbol | (quality +
bq_phred_added_misma) << 8).  `items` below lists them from the read columns alone; `m_bases` lists every M-op base of every read, which is
what the oracle's per-symbol depths count.

A region [beg, end) has npos = end - beg + 1 plane positions, the last one without a reference base, and no read may reach position end - 1
(set_reads refuses it, uvc_prep.hip): the last plane index a read covers, and so the last one a mismatch can be planted
on, is npos - 3.  The cases name that index `last` and use it where the list of edges says npos - 1."""
import functools

import numpy as np

from edge_reads import classify, is_simple
from test_gpu_worklist import D, I, M, S, unpaired

PSCAN_TILE = 1024   # k_prep_scan: positions per block
PSCAN_QCAP = 512    # its LDS queue
PSCAN_ROUND = 512   # entries between two looks at the queue
REGION_LENGTHS = (1023, 1024, 1025, 2049)   # plane positions (npos)
QUALITY_BYTES = (0, 93, 128, 255)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def ops_of(reads, k):
    cg = reads["cigars"][int(reads["cigar_off"][k]):int(reads["cigar_off"][k]) + int(reads["n_cigar"][k])]
    return [(int(c & 0xF), int(c >> 4)) for c in cg]


def m_bases(reads, k):
    """(query offsets in the read's bases, plane indices) of the bases under the read's M ops, and the M run each belongs to."""
    qi, xi, run = [], [], []
    q, r, n_run = 0, int(reads["pos"][k]) - reads["beg"], 0
    for op, ln in ops_of(reads, k):
        if op in (M, 7, 8):
            qi.append(np.arange(q, q + ln)); xi.append(np.arange(r, r + ln)); run.append(np.full(ln, n_run)); q += ln; r += ln; n_run += 1
        elif op in (I, S):
            q += ln
        elif op in (D, 3):
            r += ln
    if not qi:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(qi), np.concatenate(xi), np.concatenate(run)


def ref_codes(reads):
    """The reference's symbols per plane index; -1 on the last one, which has none."""
    return np.array([CODE[c] for c in reads["refseq"]] + [-1], np.int64)


def mismatches(reads, k, ref):
    """The mismatching M-op bases of read k: plane index, symbol, quality, M run."""
    qi, xi, run = m_bases(reads, k)
    off = int(reads["seq_off"][k])
    b, q = reads["bases"][off + qi].astype(np.int64), reads["quals"][off + qi].astype(np.int64)
    sel = b != ref[xi]
    return xi[sel], b[sel], q[sel], run[sel]


def kinds(reads, platform=1):
    return np.array([classify(ops_of(reads, k), reads["quals"][int(reads["seq_off"][k]):int(reads["seq_off"][k]) + int(reads["l_qseq"][k])], reads["beg"], platform)
                     for k in range(reads["n_reads"])])


def items(reads, added_misma=0, platform=1):
    """The queue as rows (rank, epos, symval), sorted; and per (read, M run) entry the plane indices of its items."""
    ref, kd = ref_codes(reads), kinds(reads, platform)
    rows, per_entry = [], {}
    for k in range(reads["n_reads"]):
        if kd[k] == 1:
            continue
        xi, b, q, run = mismatches(reads, k, ref)
        for r in (np.unique(m_bases(reads, k)[2])):
            per_entry[(k, int(r))] = xi[run == r]
        rows += [(k, reads["beg"] + int(x), int(s) | ((int(v) + added_misma) << 8)) for x, s, v in zip(xi, b, q)]
    return sorted(rows), per_entry


def demoted_mismatches(reads, platform=1):
    """The mismatching M-op bases of the InDel reads that are off the work list only because of a low quality at an InDel.  set_reads sizes
    the queue (RegionDev::mis_total) before it looks at the qualities -- uvcgpu_region_correct_bq can bring such a read back without a new
    allocation -- so the count it made is the number of items plus this."""
    ref, kd, n = ref_codes(reads), kinds(reads, platform), 0
    # k_aln_prelude counts a read into mis_total when it is a simple alignment or k_read_facts gave it kind 2 (`rk >= 0 || W.kind[id] == 2`), and
    # only then demotes a kind-2 read to kind 1 by has_lowbq_indel.  classify() is k_read_facts' rule followed by that one test of the qualities,
    # and has_lowbq_indel is true only where a quality is at or below the threshold of 21: with every quality at 60 it cannot fire, so the second
    # call returns the kind k_read_facts gave, and "kind 1 now, kind 2 then" picks exactly the reads that were counted and then demoted.
    for k in np.nonzero(kd == 1)[0]:
        if classify(ops_of(reads, k), np.full(int(reads["l_qseq"][k]), 60, np.uint8), reads["beg"], platform) == 2:
            n += len(mismatches(reads, k, ref)[0])
    return n


def pileup(reads):
    """[5][npos]: how many M-op bases of every read show symbol s on position x."""
    out = np.zeros((5, reads["end"] - reads["beg"] + 1), np.int64)
    for k in range(reads["n_reads"]):
        qi, xi, _ = m_bases(reads, k)
        np.add.at(out, (reads["bases"][int(reads["seq_off"][k]) + qi].astype(np.int64), xi), 1)
    return out


# ---- the inputs ----
def follow_reference(reads):
    """Every M-op base becomes the reference's: no item is left."""
    ref = ref_codes(reads)
    bases = reads["bases"].copy()
    for k in range(reads["n_reads"]):
        qi, xi, _ = m_bases(reads, k)
        bases[int(reads["seq_off"][k]) + qi] = ref[xi]
    return dict(reads, bases=bases)


def plant(reads, k, x, sym=None, qual=None):
    """Read k shows `sym` (default: the reference's base + 1) with quality `qual` on plane index x."""
    qi, xi, _ = m_bases(reads, k)
    hit = np.nonzero(xi == x)[0]
    assert len(hit) == 1, (k, x)
    at = int(reads["seq_off"][k]) + int(qi[hit[0]])
    reads["bases"][at] = (CODE[reads["refseq"][x]] + 1) % 4 if sym is None else sym
    if qual is not None:
        reads["quals"][at] = qual


def covering(reads, x, simple=True):
    """The reads with an M-op base on plane index x (simple alignments only, or InDel reads only)."""
    out = []
    for k in range(reads["n_reads"]):
        if is_simple(ops_of(reads, k)) == simple and x in m_bases(reads, k)[1]:
            out.append(k)
    return out


INDEL_SHAPES = [[(M, 30), (D, 2), (M, 30)], [(M, 30), (I, 2), (M, 28)], [(S, 5), (M, 20), (D, 1), (M, 35)], [(M, 10), (I, 1), (M, 20), (D, 3), (M, 29)]]


@functools.lru_cache(maxsize=None)
def boundary(npos, noise=0.01, seed=50):
    """A region of npos plane positions under 70-base reads every 5 positions (both strands, some clipped), one read on the region's first
    position, one that ends on its last read position, one across every PSCAN_TILE boundary, InDel reads every 90 positions (every other one
    with high qualities throughout: kind 2).  The bases follow the reference but for `noise` random errors and the planted mismatches:
    plane indices 0, 63, 64, 1023, 1024 and `last` as far as they exist, on either side of every tile boundary in one read, next to and far
    from an InDel in an InDel read."""
    n_ref = npos - 1
    last = n_ref - 2
    specs = [(0, 0, [(M, 100)]), (n_ref - 1 - 80, 16, [(S, 3), (M, 80)])]
    for k, st in enumerate(range(0, n_ref - 1 - 70, 5)):
        specs.append((st, 16 * (k % 2), [(S, 4)] * (k % 7 == 3) + [(M, 70)] + [(S, 6)] * (k % 11 == 5)))
    tiles = [t for t in range(PSCAN_TILE, n_ref, PSCAN_TILE) if t + 35 <= n_ref - 1]   # the boundaries a read can lie across
    n_tiled = len(range(0, n_ref - 1 - 70, 5))
    for t in tiles:
        specs.append((t - 35, 0, [(M, 70)]))
    n_simple = len(specs)
    for k, st in enumerate(range(20, n_ref - 1 - 70, 90)):
        specs.append((st, 16 * (k % 2), INDEL_SHAPES[k % 4]))
    order = sorted(range(len(specs)), key=lambda i: specs[i][0])
    reads = unpaired([specs[i] for i in order], n_ref=n_ref, seed=seed)
    where = {i: j for j, i in enumerate(order)}
    reads = follow_reference(reads)
    reads["bases"] = reads["bases"].copy(); reads["quals"] = reads["quals"].copy()
    rng = np.random.default_rng(seed + 1)
    ref = ref_codes(reads)
    for k in range(reads["n_reads"]):   # the noise: any other base
        qi, xi, _ = m_bases(reads, k)
        hit = rng.random(len(qi)) < noise
        reads["bases"][int(reads["seq_off"][k]) + qi[hit]] = (ref[xi[hit]] + rng.integers(1, 4, int(hit.sum()))) % 4
    indel_reads = [where[i] for i in range(n_simple, len(specs))]
    for n, k in enumerate(indel_reads):   # every other InDel read: qualities of 30 throughout, so that its M runs are on the work list
        if n % 2 == 0:
            reads["quals"][int(reads["seq_off"][k]):int(reads["seq_off"][k]) + int(reads["l_qseq"][k])] = 30
        xi, run = m_bases(reads, k)[1], m_bases(reads, k)[2]
        first_end = int(xi[run == 0][-1])
        plant(reads, k, first_end, qual=30)                   # next to the InDel
        plant(reads, k, int(xi[run == run.max()][-1]) - 3, qual=30)   # far from it
    planted = sorted({x for x in (0, 63, 64, 1023, 1024, last) if x <= last})
    for x in planted:
        plant(reads, covering(reads, x)[0], x, qual=37)
    plant(reads, where[0], 0, qual=37); plant(reads, where[1], last, qual=37)
    for n, t in enumerate(tiles):
        k = where[2 + n_tiled + n]
        plant(reads, k, t - 1, qual=37); plant(reads, k, t, qual=37); plant(reads, k, t - 30, qual=37); plant(reads, k, t + 30, qual=37)
    return dict(reads=reads, planted=planted, first_read=where[0], last_read=where[1], indel_reads=indel_reads,
                spanning=[where[2 + n_tiled + n] for n in range(len(tiles))], last=last)


def mc_npos_overflow():
    return PSCAN_TILE


@functools.lru_cache(maxsize=None)
def overflow():
    """1 024 plane positions (one tile) under 640 reads of 100 bases, every one of them with at least two mismatches inside the first tile: whichever 512
    entries a round of k_prep_scan takes, they hold more than PSCAN_QCAP mismatches, and the rest of the round takes the inline path."""
    rng = np.random.default_rng(60)
    starts = np.sort(rng.integers(0, 900, 640))
    reads = follow_reference(unpaired([(int(s), 16 * (k % 2), [(M, 100)]) for k, s in enumerate(starts)], n_ref=mc_npos_overflow() - 1, seed=61))
    reads["bases"] = reads["bases"].copy(); reads["quals"] = reads["quals"].copy()
    for k in range(reads["n_reads"]):
        xi = m_bases(reads, k)[1]
        for x in rng.choice(xi, 2 + k % 4, replace=False):
            plant(reads, k, int(x), qual=int(rng.choice([12, 30, 37])))
    return reads


@functools.lru_cache(maxsize=None)
def empty():
    """The boundary reads of 1 025 plane positions with every base the reference's: no item at all."""
    return follow_reference(boundary(1025)["reads"])


@functools.lru_cache(maxsize=None)
def with_n():
    """N in reads over a base of the reference, and N in the reference under N and under other bases of the reads."""
    case = boundary(1025)
    reads = dict(case["reads"])
    reads["bases"] = reads["bases"].copy(); reads["quals"] = reads["quals"].copy()
    ref = list(reads["refseq"])
    for x in (200, 201, 640):
        ref[x] = "N"
    reads["refseq"] = "".join(ref)
    read_n, ref_n_read_n, ref_n_read_base = [], [], []
    for x in (100, 101, 500):
        for k in covering(reads, x)[:3]:
            plant(reads, k, x, sym=4, qual=30); read_n.append((k, x))
    for x in (200, 201, 640):
        ks = covering(reads, x)
        for k in ks[:2]:
            plant(reads, k, x, sym=4, qual=30); ref_n_read_n.append((k, x))
        ref_n_read_base += [(k, x) for k in ks[2:]]
    return dict(reads=reads, read_n=read_n, ref_n_read_n=ref_n_read_n, ref_n_read_base=ref_n_read_base)


@functools.lru_cache(maxsize=None)
def quality_bytes():
    """Mismatching and matching bases of quality 0, 93, 128 and 255, in simple alignments and in M runs of InDel reads."""
    case = boundary(1024)
    reads = dict(case["reads"])
    reads["bases"] = reads["bases"].copy(); reads["quals"] = reads["quals"].copy()
    planted = []
    for n, x in enumerate(range(150, 950, 50)):
        qv = QUALITY_BYTES[n % 4]
        ks = covering(reads, x)
        plant(reads, ks[0], x, qual=qv); planted.append((ks[0], x, qv))
        qi, xi, _ = m_bases(reads, ks[1])
        reads["quals"][int(reads["seq_off"][ks[1]]) + int(qi[list(xi).index(x)])] = qv   # a matching base of that quality
    for n, k in enumerate(case["indel_reads"][::2]):   # (the InDel reads with high qualities: the byte goes far from the InDel)
        xi = m_bases(reads, k)[1]
        x, qv = int(xi[-3]), QUALITY_BYTES[1 + n % 3]   # (0 would be a low quality next to nothing: kept off the InDel reads)
        plant(reads, k, x, qual=qv); planted.append((k, x, qv))
    return dict(reads=reads, planted=planted)


def scan_rounds(reads, platform=1):
    """How many mismatches inside tile 0 each work-list entry has that reaches the tile (every entry here lies in it)."""
    _, per_entry = items(reads, platform=platform)
    return np.array([int(((x >= 0) & (x < PSCAN_TILE)).sum()) for x in per_entry.values()])
