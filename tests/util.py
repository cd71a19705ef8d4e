import ctypes as C

import numpy as np

from uvc_amd import _ffi, region, synth

INT_GROUPS = ["PREP32", "PREP64", "THRES", "SEG32", "SEG64", "BQSUM", "FRAG", "FAM", "FAMINFO32", "FAMINFO64", "DUPLEX", "RTR", "BAQ", "VQ"]


def run_region(lib, reads, params=None, platform=1):
    p = params if params is not None else region.default_params(lib, platform=platform)
    R = region.Region(lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    R.accumulate()
    return R


def amplicon_stack():
    """A 70 000-read amplicon stack: every read covers positions 152..209 of a 400 bp region, more than 65 535 fragments on one position."""
    rng = np.random.default_rng(8)
    n, L, ref_len, beg = 70000, 60, 400, 7_000_000
    ref = rng.integers(0, 4, ref_len)
    start = 150 + rng.integers(0, 3, n)
    bases = ref[start[:, None] + np.arange(L)[None, :]]
    err = rng.random((n, L)) < 0.004
    bases = np.where(err, rng.integers(0, 4, (n, L)), bases).astype(np.uint8)
    return dict(n_reads=n, pos=(beg + start).astype(np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), flag=np.where(np.arange(n) % 2, 16, 0).astype(np.uint16),
                mapq=np.full(n, 60, np.uint8), nm=np.full(n, -1, np.int32), l_qseq=np.full(n, L, np.int32), seq_off=(np.arange(n, dtype=np.int64) * L), cigar_off=np.arange(n, dtype=np.int64),
                n_cigar=np.ones(n, np.int32), frag_id=np.arange(n, dtype=np.int32), fam_id=np.arange(n, dtype=np.int32), fam_strand=(np.arange(n) % 2).astype(np.uint8), n_fams=n,
                fam_dflag=np.zeros(n, np.uint8), bases=bases.reshape(-1), quals=rng.choice([20, 30, 37], n * L).astype(np.uint8), cigars=np.full(n, (L << 4) | 0, np.uint32),
                tid=1, beg=beg, end=beg + ref_len, refseq="".join("ACGT"[b] for b in ref))


def exact_stack(n):
    """n single-read fragments, all the same 60 bases (the reference's) with one quality on one strand, over positions 150..209 of a 400 bp
    region: with n = 65 535 one 16-bit bucket counter of k_frag reaches 0xFFFF, with 65 536 the fragment depth is the first that needs 32 bits."""
    rng = np.random.default_rng(9)
    L, ref_len, beg = 60, 400, 7_000_000
    ref = rng.integers(0, 4, ref_len)
    return dict(n_reads=n, pos=np.full(n, beg + 150, np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), flag=np.zeros(n, np.uint16),
                mapq=np.full(n, 60, np.uint8), nm=np.full(n, -1, np.int32), l_qseq=np.full(n, L, np.int32), seq_off=(np.arange(n, dtype=np.int64) * L), cigar_off=np.arange(n, dtype=np.int64),
                n_cigar=np.ones(n, np.int32), frag_id=np.arange(n, dtype=np.int32), fam_id=np.arange(n, dtype=np.int32), fam_strand=np.zeros(n, np.uint8), n_fams=n,
                fam_dflag=np.zeros(n, np.uint8), bases=np.tile(ref[150:150 + L], n).astype(np.uint8), quals=np.full(n * L, 30, np.uint8), cigars=np.full(n, (L << 4) | 0, np.uint32),
                tid=1, beg=beg, end=beg + ref_len, refseq="".join("ACGT"[b] for b in ref))


def diff_groups(Ra, Rb, groups=INT_GROUPS):
    """Returns {group: (n_mismatching_cells, first few mismatches)} for groups that differ."""
    bad = {}
    for g in groups:
        a, b = Ra.fetch(g), Rb.fetch(g)
        if not np.array_equal(a, b):
            idx = np.argwhere(a != b)
            bad[g] = (len(idx), [(tuple(int(v) for v in i), int(a[tuple(i)]), int(b[tuple(i)])) for i in idx[:8]])
    return bad


def kept_groups(full):
    """What UvcScoreRequest::kept_only returns, made from the records `full` of the same call without it: the (position, symbol type) groups
    with a written record (keep and out) or a GERMLINE line (germ_emit), whole and in order, with germ_ref / germ_alt1 / germ_alt2 re-based
    to the record indices of the reduced list.  -> (indices of the kept records in `full`, the expected kept records)."""
    n = len(full["refpos"])
    if n == 0:
        return np.zeros(0, np.int64), {f: v[:0] for f, v in full.items()}
    is_base = full["symbol"] <= 5
    head = np.ones(n, bool)
    head[1:] = (full["refpos"][1:] != full["refpos"][:-1]) | (is_base[1:] != is_base[:-1])
    gid = np.cumsum(head) - 1
    written = ((full["keep"] == 1) & (full["out"] == 1)) | (full["germ_emit"] == 1)
    group_kept = np.zeros(gid.max() + 1, bool)
    group_kept[gid[written]] = True
    sel = np.nonzero(group_kept[gid])[0]
    new_index = -np.ones(n, np.int64)
    new_index[sel] = np.arange(len(sel))
    out = {}
    for f in full:
        want = full[f][sel]
        if f in ("germ_ref", "germ_alt1", "germ_alt2"):
            want = np.where(want >= 0, new_index[np.maximum(want, 0)], -1)
            assert (want[full[f][sel] >= 0] >= 0).all(), f          # a genotype's records belong to its own group
        out[f] = want
    return sel, out


def presence_violations(R):
    """uvcgpu_region_check_presence on the planes the GPU handle R holds (what region.py runs after every accumulate when
    UVCGPU_CHECK_PRESENCE is set): the number of (position, symbol) cells that contradict the presence statement."""
    fn = R.lib.dll.uvcgpu_region_check_presence
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64(-1)
    R._check(fn(R.h, C.byref(n)))
    return int(n.value)
