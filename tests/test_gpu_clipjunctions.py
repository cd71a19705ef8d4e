"""The clip-site junctions of the HIP library (uvcgpu_region_clip_junctions, Region.clip_junctions) and the J lines built from them
(uvc1-mi355x --clip-sites-junctions 1).  Every number is an integer and is compared for equality with the restatement of the definitions
(tests/clipjunctions_restatement.py), for the library and for the test library tests/native/libuvcgpu_clipjunc_naive.so: the same sources
with the naive form of the search (one byte per base, straight from refsym), whose bytes must equal the packed form's.
  * site rows are crafted directly (the call reads pos, side and VOTE of a row and the reference of the region, nothing else): reference
    lengths around the word (32), wave (64), block (256) and grid-stride edges, query lengths 1..32, compare masks with holes, placements
    that touch both ends of the reference and the same query one further, N / I / - in the reference, the plane index without a base, ties,
    hist at every max_mismatch, second_mm, max_dist, the mate rule, 0..257 sites;
  * assertions on the restatement's own output that an unwired branch could not meet;
  * every refusal by its message, with nothing written; the legality window; two calls return the same bytes;
  * one chain of synthetic reads with a planted deletion, tandem duplication and inversion through clip_sites and clip_junctions;
  * the report of the command line against the Python chain and the restatement text, VCF, S and R lines unchanged by the option."""
import ctypes as C
import os

import numpy as np
import pytest

import bamwriter
import clipjunctions_restatement as cj
import clipsites_restatement as cr
from test_bq_correction import make_reads
from test_gpu_coverage import run_cli
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
NAIVE = os.path.join(_ffi.ROOT, "tests", "native", "libuvcgpu_clipjunc_naive.so")
EINVAL = _ffi.ENUMS["UVCGPU_EINVAL"]
BEG = 70_000
LEFT, RIGHT = cj.LEFT, cj.RIGHT
COMP = {0: 3, 1: 2, 2: 1, 3: 0}


@pytest.fixture(scope="module")
def libs(gpu_lib):
    """(name, library): the product library and the naive build of the kernel file."""
    assert os.path.exists(NAIVE), "build it: make -C uvc_amd/csrc"
    naive = _ffi.Lib(NAIVE, "uvcgpu_")
    assert naive.dll.uvcgpu_init(0) == 0, naive.last_error()
    assert gpu_lib.dll.uvc_clipjunc_naive() == 0 and naive.dll.uvc_clipjunc_naive() == 1
    return [("packed", gpu_lib), ("naive", naive)]


def random_ref(n, seed, letters="ACGT"):
    return "".join(letters[i] for i in np.random.default_rng(seed).integers(0, len(letters), n))


def codes(s):
    return [cj.CODE[c] for c in s]


def planted(ref, side, strand, t, L):
    """The query (codes, k = 0 .. L - 1) whose placement on `strand` at t has no mismatch; ref may be longer than the region's."""
    d = 1 if side == RIGHT else -1
    if strand == 0:
        return [cj.CODE[ref[t + d * k]] for k in range(L)]
    return [COMP[cj.CODE[ref[t - d * k]]] for k in range(L)]


def site_row(x, side, votes):
    """A site row with pos = BEG + x; votes: per k a code (three votes for it), a tuple of five counts, or None."""
    row = np.zeros(cr.ROW, np.int64)
    row[cr.W["pos"]], row[cr.W["side"]], row[cr.W["reads"]] = BEG + x, side, 3
    for k, v in enumerate(votes):
        if v is None:
            continue
        cell = row[cr.VOTE + k * cr.NCODE:cr.VOTE + (k + 1) * cr.NCODE]
        if isinstance(v, tuple):
            cell[:] = v
        else:
            cell[v] = 3
    return row


def rows_of(sites):
    """sites: (x, side, votes), in any order -> rows ascending by (pos, side), and for every given site its row's index"""
    order = sorted(range(len(sites)), key=lambda i: (sites[i][0], sites[i][1]))
    rows = np.stack([site_row(*sites[i]) for i in order]) if sites else np.zeros((0, cr.ROW), np.int64)
    index = {i: k for k, i in enumerate(order)}
    return rows, [index[i] for i in range(len(sites))]


def open_ref(lib, ref):
    return region.Region(lib, region.default_params(lib), 0, BEG, BEG + len(ref), ref)


def check(libs, ref, rows, regions=None, **req):
    """Both builds against the restatement -> (totals, junction rows) of the restatement.  regions: one open Region per library."""
    wt, wj = cj.run(ref, BEG, rows, **req)
    for k, (name, lib) in enumerate(libs):
        R = regions[k] if regions else open_ref(lib, ref)
        totals, got = R.clip_junctions(rows, **req)
        if not regions:
            R.close()
        assert got.dtype == np.int64 and got.shape == wj.shape, (name, got.shape, wj.shape)
        assert np.array_equal(got, wj), (name, req, [(int(i), int(j), int(got[i, j]), int(wj[i, j])) for i, j in np.argwhere(got != wj)[:8]])
        assert totals.tolist() == wt.tolist(), (name, totals.tolist(), wt.tolist())
    return wt, wj


def col(j, name):
    return j[:, cj.W[name]].tolist()


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65, 255, 256, 257, 4099])
def test_reference_lengths_and_both_ends_of_the_reference(n, libs):
    """Per side and strand a 16-base query whose placement touches x = 0, one that touches x = n - 1, and the same two one position further
    out, planted on a reference one base longer at either end: those must not count."""
    L = 16
    ext = random_ref(n + 2, n)            # the region's reference is ext[1 : n + 1]: x = index in ext - 1
    ref = ext[1:n + 1]
    sites, want = [], []
    x = 0
    for side in (LEFT, RIGHT):
        d = 1 if side == RIGHT else -1
        for strand in (0, 1):
            e = d if strand == 0 else -d
            for lo in (-1, 0, n - L, n - L + 1):                       # the lowest faced x of the placement
                t = lo if e > 0 else lo + L - 1
                sites.append((x, side, planted(ext, side, strand, t + 1, L)))
                want.append((strand, t) if 0 <= lo <= n - L else None)
                x += 1 + (n - 17) // 16
    rows, at = rows_of(sites)
    wt, wj = check(libs, ref, rows, min_len=16, max_mismatch=1)
    for i, w in zip(at, want):
        if w is None:
            assert wj[i, cj.W["status"]] == cj.NOT_PLACED and wj[i, cj.HIST:].sum() == 0, (n, i, wj[i].tolist())
        else:
            side = int(rows[i, cr.W["side"]])
            assert wj[i, cj.W["status"]] == cj.PLACED and wj[i, cj.W["best_mm"]] == 0 and wj[i, cj.W["strand"]] == w[0], (n, i, wj[i].tolist())
            assert wj[i, cj.W["partner"]] == BEG + cj.partner_of(side, w[0], w[1])[0]
    assert wt.tolist()[:3] == [16, 16, 8]


def test_a_reference_shorter_than_the_query(libs):
    ref = random_ref(20, 1)
    rows, _ = rows_of([(3, RIGHT, codes(random_ref(32, 2))), (5, LEFT, codes(ref[::-1]) + [0] * 12), (20, LEFT, codes(ref[:8]))])
    wt, wj = check(libs, ref, rows, min_len=8, max_mismatch=7)
    assert col(wj, "query_len") == [32, 32, 8] and col(wj, "status")[:2] == [cj.NOT_PLACED, cj.NOT_PLACED] and wj[:2, cj.HIST:].sum() == 0


@pytest.mark.parametrize("L", [1, 15, 16, 17, 31, 32])
def test_query_lengths(L, libs):
    ref = random_ref(257, 5)
    sites = [(10 * i, side, planted(ref, side, strand, t, L)) for i, (side, strand, t) in enumerate([(RIGHT, 0, 100), (LEFT, 0, 140), (RIGHT, 1, 180), (LEFT, 1, 60), (RIGHT, 0, 257 - L), (LEFT, 0, L - 1)])]
    rows, at = rows_of(sites)
    wt, wj = check(libs, ref, rows, min_len=1, max_mismatch=0)
    assert col(wj, "query_len") == [L] * 6 and col(wj, "cmp_len") == [L] * 6 and col(wj, "status") == [cj.PLACED] * 6
    if L >= 15:
        assert col(wj, "n_best") == [1] * 6 and [wj[at[0], cj.W["partner"]], wj[at[1], cj.W["partner"]]] == [BEG + 100, BEG + 141]
    else:
        assert min(col(wj, "n_best")) > 20                                  # a single base lies everywhere
    check(libs, ref, rows, min_len=min(L + 1, 32), max_mismatch=0)          # one more than there is: not searched (L = 32: searched)


def test_compare_masks_with_holes(libs):
    """A low-majority k, a code-4 winner and a total below min_votes are not compared: a wrong base there is no mismatch; votes that begin
    at k = 5 make a query whose first five indices face the reference uncompared."""
    ref = random_ref(300, 8)
    q = planted(ref, RIGHT, 0, 120, 24)
    wrong = lambda c: (c + 1) % 4                                                            # noqa: E731
    holes = list(q)
    holes[3] = tuple(3 if c == wrong(q[3]) else 2 if c == q[3] else 0 for c in range(5))     # 3 of 5 for a wrong base: 9 < 10
    holes[7] = (0, 0, 0, 0, 5)                                                               # the winner is code 4
    holes[11] = tuple(1 if c == wrong(q[11]) else 0 for c in range(5))                       # one vote, min_votes 2
    strict = list(q)
    strict[3] = tuple(4 if c == wrong(q[3]) else 2 if c == q[3] else 0 for c in range(5))    # 4 of 6: 12 >= 12, compared, a mismatch
    late = [None] * 5 + planted(ref, LEFT, 0, 200, 26)[5:]
    tie = list(planted(ref, LEFT, 1, 40, 20))
    tie[2] = tuple(2 if c in (tie[2], 3) else 0 for c in range(5)) if tie[2] != 3 else (2, 0, 0, 2, 0)   # 2 of 4: 6 < 8, not compared
    rows, at = rows_of([(10, RIGHT, holes), (20, RIGHT, strict), (30, LEFT, late), (40, LEFT, tie)])
    wt, wj = check(libs, ref, rows, min_votes=2, min_len=16, max_mismatch=0)
    assert col(wj, "query_len") == [24, 24, 26, 20] and col(wj, "cmp_len") == [21, 24, 21, 19]
    assert col(wj, "status") == [cj.PLACED, cj.NOT_PLACED, cj.PLACED, cj.PLACED] and wj[at[2], cj.W["partner"]] == BEG + 201
    wt, wj = check(libs, ref, rows, min_votes=1, min_len=16, max_mismatch=1)                 # min_votes 1: k = 11 is compared and differs
    assert col(wj, "cmp_len") == [22, 24, 21, 19] and col(wj, "best_mm")[:2] == [1, 1]
    check(libs, ref, rows, min_votes=3, min_len=22, max_mismatch=0)                          # the votes of three: only the full query is searched


def test_reference_characters_that_are_no_base(libs):
    """N, I and - under a placement mismatch everything, lower case is a base; under an index that is not compared they cost nothing."""
    base = random_ref(200, 13)
    q = planted(base, RIGHT, 0, 50, 24)
    ref = list(base)
    ref[52], ref[60], ref[70] = "N", "I", "-"
    ref[55] = ref[55].lower()
    ref = "".join(ref)
    free = list(q)
    free[2] = free[10] = None                                                                # x = 52 and x = 60 are not compared
    free[23] = q[23]
    rc = planted(base, LEFT, 1, 50, 24)                                                      # faces x = 50 .. 73 as well, complemented
    rows, at = rows_of([(5, RIGHT, q), (6, RIGHT, free), (7, LEFT, rc)])
    for mm in (2, 3):
        wt, wj = check(libs, ref, rows, min_len=16, max_mismatch=mm)
        assert col(wj, "status") == [cj.PLACED if mm == 3 else cj.NOT_PLACED, cj.PLACED, cj.PLACED if mm == 3 else cj.NOT_PLACED]
        assert col(wj, "best_mm")[1] == 1 and (mm < 3 or col(wj, "best_mm") == [3, 1, 3])


def test_the_last_plane_index_has_no_base(libs):
    """refsym[npos - 1] is 0, the code of A: sixteen A never lie over it."""
    ref = random_ref(84, 3, "CGT") + "A" * 15
    n = len(ref)
    rows, at = rows_of([(10, RIGHT, [0] * 16), (n, LEFT, [0] * 16), (20, LEFT, [3] * 16), (30, RIGHT, [0] * 15)])
    wt, wj = check(libs, ref, rows, min_len=15, max_mismatch=0)
    assert [wj[i, cj.W["status"]] for i in at] == [cj.NOT_PLACED, cj.NOT_PLACED, cj.NOT_PLACED, cj.PLACED] and wj[at[3], cj.W["partner"]] == BEG + n - 15
    wt, wj = check(libs, ref, rows, min_len=15, max_mismatch=1)                              # with one mismatch the G in front is taken in
    assert [wj[i, cj.W["status"]] for i in at] == [cj.PLACED] * 4 and [wj[i, cj.W["best_mm"]] for i in at] == [1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ ties and counts
def test_three_copies_a_palindrome_hist_and_second_mm(libs):
    motif = "ACGGTCATTGCAGGCTAAGCTTAGCCTG"[:20]
    pal = "ACGTTGCAAGCTTGCAACGT"                                                            # its own reverse complement
    assert [COMP[c] for c in codes(pal)][::-1] == codes(pal)
    other = lambda s, at: "".join({"A": "C", "C": "A", "G": "T", "T": "G"}[c] if i in at else c for i, c in enumerate(s))   # noqa: E731
    near, far = other(motif, (7,)), other(motif, (3, 9, 15))                                 # one and three mismatches from the motif
    assert sum(a != b for a, b in zip(near, motif)) == 1 and sum(a != b for a, b in zip(far, motif)) == 3
    pad = lambda k: random_ref(37, 100 + k, "CT")                                            # noqa: E731
    ref = pad(0) + motif + pad(1) + motif + pad(2) + near + pad(3) + motif + pad(4) + far + pad(5) + pal + pad(6)
    first, at_pal = len(pad(0)), ref.index(pal)
    only = "TTGACCGATAGGCATCAGTA"                                                            # a query that lies once, with no mismatch, and nowhere near
    ref += only + pad(7)
    rows, at = rows_of([(5, RIGHT, codes(motif)), (9, RIGHT, codes(pal)), (400, LEFT, codes(pal)[::-1]), (12, RIGHT, codes(only)), (14, RIGHT, codes(near))])
    for mm in range(8):
        wt, wj = check(libs, ref, rows, min_len=16, max_mismatch=mm)
        h = wj[at[0], cj.HIST:].tolist()
        assert h[0] == 3 and h[1] == (1 if mm >= 1 else 0) and h[3] == (1 if mm >= 3 else 0) and not any(h[mm + 1:]), (mm, h)
        assert wj[at[0], cj.W["n_best"]] == 3 and wj[at[0], cj.W["partner"]] == BEG + first and wj[at[0], cj.W["second_mm"]] == 0      # the smallest t of three
        assert wj[at[1], cj.W["strand"]] == 0 and wj[at[1], cj.W["partner"]] == BEG + at_pal and wj[at[1], cj.W["n_best"]] == 2         # forward wins the tie
        assert wj[at[2], cj.W["strand"]] == 0 and wj[at[2], cj.W["n_best"]] == 2
        # second_mm: best_mm with two best; the next non-empty bin with one; -1 with nothing behind the best
        assert wj[at[3], cj.W["n_best"]] == 1 and wj[at[3], cj.W["second_mm"]] == -1 or mm >= 5
        assert wj[at[4], cj.W["best_mm"]] == 0 and wj[at[4], cj.W["second_mm"]] == (1 if mm >= 1 else -1)
    assert wt.tolist()[:4] == [5, 5, 5, 2]


def test_max_dist_at_the_boundary(libs):
    ref = random_ref(600, 21)
    q = planted(ref, RIGHT, 0, 400, 20)
    rows, _ = rows_of([(100, RIGHT, q), (101, RIGHT, q), (520, LEFT, planted(ref, LEFT, 1, 300, 20))])
    for dist, want in [(0, [2, 2, 2]), (300, [2, 2, 2]), (299, [1, 2, 2]), (219, [1, 1, 1]), (220, [1, 1, 2])]:
        wt, wj = check(libs, ref, rows, min_len=16, max_mismatch=1, max_dist=dist)
        assert col(wj, "status") == want, (dist, col(wj, "status"), col(wj, "len"))


def test_the_mate_rule(libs):
    """The slop at the exact distance, two candidates at one distance (the smaller pos), a site of the wrong side ignored, the site itself
    allowed."""
    ref = random_ref(800, 34)
    q = planted(ref, RIGHT, 0, 500, 20)                    # partner x = 500, the mate is a LEFT site
    inv = planted(ref, RIGHT, 1, 299, 20)                  # reverse at t = 299: partner x = 300, the mate is a RIGHT site
    sites = [(100, RIGHT, q), (495, LEFT, [1] * 3), (500, RIGHT, [1] * 3), (505, LEFT, [1] * 3), (300, RIGHT, inv), (650, LEFT, planted(ref, LEFT, 0, 539, 20))]      # partner x = 540, the mate is a RIGHT site
    rows, at = rows_of(sites)
    for slop, mates in [(5, [at[1], at[4], -1]), (4, [-1, at[4], -1]), (50, [at[1], at[4], at[2]]), (40, [at[1], at[4], at[2]]), (39, [at[1], at[4], -1]), (0, [-1, at[4], -1])]:
        wt, wj = check(libs, ref, rows, min_len=16, max_mismatch=0, mate_slop=slop)
        assert [int(wj[at[i], cj.W["mate"]]) for i in (0, 4, 5)] == mates, (slop, col(wj, "mate"), col(wj, "partner"))
    rows2, at2 = rows_of([sites[0], (497, LEFT, [1] * 3), (502, LEFT, [1] * 3), (500, RIGHT, [1] * 3)])   # 3 below, 2 above: the nearer one
    wt, wj = check(libs, ref, rows2, min_len=16, max_mismatch=0, mate_slop=3)
    assert wj[at2[0], cj.W["mate"]] == at2[2] and wt[4] == 1


@pytest.mark.parametrize("n_sites", [0, 1, 63, 64, 65, 257])
def test_site_counts(n_sites, libs):
    n = 4099
    ref = random_ref(n, 77)
    rng = np.random.default_rng(n_sites)
    sites = []
    for i in range(n_sites):
        side, strand, L = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(14, 33))
        t = int(rng.integers(32, n - 32))
        q = planted(ref, side, strand, t, L)
        if i % 5 == 0:
            q[int(rng.integers(0, L))] ^= 1                                      # one mismatch
        if i % 7 == 0:
            q = codes(random_ref(L, 1000 + i))                                   # lies nowhere
        sites.append((16 * i + (i % 3), side, q))
    rows, _ = rows_of(sites)
    wt, wj = check(libs, ref, rows, min_len=16, max_mismatch=1, mate_slop=40)
    assert wt[0] == n_sites
    if n_sites >= 63:
        assert set(col(wj, "status")) == {0, 1, 2} and set(col(wj, "strand")) == {-1, 0, 1} and {cj.DEL, cj.DUP, cj.INV} <= set(col(wj, "klass")) and wt[4] > 0 and set(col(wj, "best_mm")) == {-1, 0, 1}


# ------------------------------------------------------------------------------------------------ the ABI
SENTINEL = -123456789


def raw_call(lib, R, rows, req=(2, 16, 1, 0, 10), n=None, null=()):
    fn = lib.dll.uvcgpu_region_clip_junctions
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    rq = _ffi.UvcClipJunctionsRequest(*req)
    out = np.full((max(len(rows), 1), cj.ROW), SENTINEL, np.int64)
    totals = np.full(cj.NTOTAL, SENTINEL, np.int64)
    p = lambda name, v: None if name in null else v                                           # noqa: E731
    rc = fn(p("r", R.h), p("sites", rows.ctypes.data), len(rows) if n is None else n, p("req", C.byref(rq)), p("junctions", out.ctypes.data), p("totals", totals.ctypes.data))
    return rc, out, totals, lib.last_error()


def test_refusals_write_nothing(libs):
    name, lib = libs[0]
    ref = random_ref(500, 4)
    R = open_ref(lib, ref)
    good, _ = rows_of([(10, LEFT, planted(ref, LEFT, 0, 300, 20)), (10, RIGHT, planted(ref, RIGHT, 0, 100, 20)), (500, RIGHT, [0] * 20)])

    def moved(i, word, v):
        r = good.copy()
        r[i, cr.W[word]] = v
        return r

    for what, word, kw in [
        ("NULL region", "null region", dict(rows=good, null=("r",))), ("NULL sites", "NULL", dict(rows=good, null=("sites",))), ("NULL req", "NULL", dict(rows=good, null=("req",))),
        ("NULL junctions", "NULL", dict(rows=good, null=("junctions",))), ("NULL totals", "NULL", dict(rows=good, null=("totals",))), ("a negative count", "n_sites", dict(rows=good, n=-1)),
        ("min_votes 0", "min_votes", dict(rows=good, req=(0, 16, 1, 0, 10))), ("min_len 0", "min_len", dict(rows=good, req=(2, 0, 1, 0, 10))), ("min_len 33", "min_len", dict(rows=good, req=(2, 33, 1, 0, 10))),
        ("max_mismatch -1", "max_mismatch", dict(rows=good, req=(2, 16, -1, 0, 10))), ("max_mismatch 8", "max_mismatch", dict(rows=good, req=(2, 16, 8, 0, 10))),
        ("max_dist -1", "max_dist", dict(rows=good, req=(2, 16, 1, -1, 10))), ("mate_slop -1", "mate_slop", dict(rows=good, req=(2, 16, 1, 0, -1))),
        ("pos in front of the region", "row 0", dict(rows=moved(0, "pos", BEG - 1))), ("pos behind the region", "row 2", dict(rows=moved(2, "pos", BEG + 501))),
        ("side 2", "side", dict(rows=moved(1, "side", 2))), ("side -1", "side", dict(rows=moved(0, "side", -1))),
        ("equal rows", "row 1", dict(rows=moved(1, "side", 0))), ("descending pos", "row 2", dict(rows=moved(2, "pos", BEG + 9))), ("descending side", "row 1", dict(rows=good[[1, 0, 2]])),
    ]:
        rc, out, totals, msg = raw_call(lib, R, **kw)
        assert rc == EINVAL and word in msg and "clip_junctions" in msg, (what, rc, msg)
        assert (out == SENTINEL).all() and (totals == SENTINEL).all(), what
    rc, out, totals, msg = raw_call(lib, R, good)                              # the handle is as usable as before
    assert rc == 0 and np.array_equal(out, cj.run(ref, BEG, good)[1]) and (out != SENTINEL).all()
    rc, out, totals, msg = raw_call(lib, R, good[:0], null=("sites", "junctions"))   # no site: zero totals
    assert rc == 0 and not totals.any() and (out == SENTINEL).all()
    dll = lib.dll
    dll.uvcgpu_clip_junction_section_name.restype, dll.uvcgpu_clip_class_name.restype = C.c_char_p, C.c_char_p
    assert [dll.uvcgpu_clip_class_name(C.c_int32(i)).decode() for i in range(5)] == cj.CLASSES
    R.close()


def test_the_legal_window_and_equal_bytes(libs):
    reads = synth.generate_region(seed=12, region_len=3000, depth=40, clip_frac=0.2)
    ref = reads["refseq"] if isinstance(reads["refseq"], str) else reads["refseq"].decode()
    beg = int(reads["beg"])
    q = planted(ref, RIGHT, 0, 2000, 24)
    rows, _ = rows_of([(150, RIGHT, q), (2000, LEFT, planted(ref, LEFT, 0, 149, 24)), (2500, RIGHT, planted(ref, RIGHT, 1, 700, 24))])
    rows[:, cr.W["pos"]] += beg - BEG
    want = cj.run(ref, beg, rows)
    assert want[0].tolist()[:5] == [3, 3, 3, 3, 2] and col(want[1], "klass") == [cj.DEL, cj.DEL, cj.INV] and col(want[1], "mate")[:2] == [1, 0]
    for name, lib in libs:
        R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])

        def same(when):
            t, j = R.clip_junctions(rows)
            assert np.array_equal(j, want[1]) and t.tolist() == want[0].tolist(), (name, when)
            return t, j

        a, b = same("right after create"), same("a second call")
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        R.set_reads(reads)
        same("after set_reads")
        R.accumulate()
        same("after accumulate")
        R.score(release_state=True)
        same("after a releasing score")
        R.accumulate()
        gen = R.score_stream(4096)
        next(gen)
        same("while a score stream is open")
        gen.close()
        R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        same("after a reset")
        R.close()


# ------------------------------------------------------------------------------------------------ reads -> sites -> junctions
M, S = 0, 4
EVENTS = dict(dele=(400, 700), dup=(1200, 1260), inv=(1800, 2300))       # a 300 bp deletion, a 60 bp tandem duplication, a 500 bp inversion


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def event_reads(ref, beg, per_end=12, read_len=100):
    """Reads over the junctions of the sample, aligned as an aligner leaves them: the longer part matched, the rest soft-clipped.  Per junction
    end `per_end` reads, 60 matched and 40 clipped bases."""
    (d0, d1), (u0, u1), (i0, i1) = EVENTS["dele"], EVENTS["dup"], EVENTS["inv"]
    specs = []                                                            # (x of the first matched base, cigar, sequence)

    def right_clipped(x_end, tail):                                       # matched up to x_end (exclusive), then `tail`
        for j in range(per_end):
            m = 60 - j
            specs.append((x_end - m, [(M, m), (S, 40)], ref[x_end - m:x_end] + tail[:40]))

    def left_clipped(x_beg, head):                                        # `head`, then matched from x_beg
        for j in range(per_end):
            m = 60 - j
            specs.append((x_beg, [(S, 40), (M, m)], head[-40:] + ref[x_beg:x_beg + m]))

    right_clipped(d0, ref[d1:d1 + 40]);            left_clipped(d1, ref[d0 - 40:d0])                      # the deletion
    right_clipped(u1, ref[u0:u0 + 40]);            left_clipped(u0, ref[u1 - 40:u1])                      # the duplication's junction: u1 | u0
    right_clipped(i0, revcomp(ref[i1 - 40:i1]));   left_clipped(i1, revcomp(ref[i0:i0 + 40]))             # the inversion's outer ends
    left_clipped(i0, revcomp(ref[i1:i1 + 40]));    right_clipped(i1, revcomp(ref[i0 - 40:i0]))            # ... and the same reads as the inverted segment aligns them
    full = [(x, 0x10 if k % 2 else 0, cg, codes(seq), [30] * len(seq)) for k, (x, cg, seq) in enumerate(specs)]
    reads = make_reads(full, beg=beg, ref_len=len(ref))
    reads["refseq"] = ref
    return reads


def expected_events():
    """(x, side) -> (class, len, the mate's (x, side)) for the eight junction ends"""
    (d0, d1), (u0, u1), (i0, i1) = EVENTS["dele"], EVENTS["dup"], EVENTS["inv"]
    return {(d0, RIGHT): (cj.DEL, 300, (d1, LEFT)), (d1, LEFT): (cj.DEL, 300, (d0, RIGHT)), (u1, RIGHT): (cj.DUP, 60, (u0, LEFT)), (u0, LEFT): (cj.DUP, 60, (u1, RIGHT)),
            (i0, RIGHT): (cj.INV, 500, (i1, RIGHT)), (i1, RIGHT): (cj.INV, 500, (i0, RIGHT)), (i0, LEFT): (cj.INV, 500, (i1, LEFT)), (i1, LEFT): (cj.INV, 500, (i0, LEFT))}


def placed_events(rows, j, beg):
    """(x, side) -> (class, len, the mate's (x, side) or None) of the placed rows"""
    at = lambda i: (int(rows[i, cr.W["pos"]]) - beg, int(rows[i, cr.W["side"]]))             # noqa: E731
    return {at(i): (int(r[cj.W["klass"]]), int(r[cj.W["len"]]), at(int(r[cj.W["mate"]])) if r[cj.W["mate"]] >= 0 else None) for i, r in enumerate(j) if r[cj.W["status"]] == cj.PLACED}


def test_reads_to_sites_to_junctions(libs):
    ref = random_ref(3000, 2024)
    reads = event_reads(ref, BEG)
    rs = cr.Restatement(reads)
    whole = [(BEG, BEG + 3001)]
    wt, wrows, _ = rs.run(whole, 0, 10, 3)
    want = cj.run(ref, BEG, wrows)
    assert len(wrows) == 8 and placed_events(wrows, want[1], BEG) == expected_events() and want[0].tolist()[:5] == [8, 8, 8, 8, 8]
    for name, lib in libs:
        R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        R.set_reads(reads)
        totals, rows, _ = R.clip_sites(whole, 0, 10, 3)
        assert np.array_equal(rows, wrows), name
        t, j = R.clip_junctions(rows)
        assert np.array_equal(j, want[1]) and t.tolist() == want[0].tolist(), name
        R.close()


# ------------------------------------------------------------------------------------------------ command line
GATE = (0, 10, 3)
REQ = (2, 16, 1, 0, 10)
JOPTS = ["--clip-sites-junctions", "1"]


def event_panel(d):
    """A contig that holds the 3 kb region of the chain test from 20 000 on, with its reads and 30x of plain reads over it, and a BED line
    over the region: the events lie 400 bases and more inside it."""
    ref = random_ref(3000, 2024)
    off = 20_000
    rng = np.random.default_rng(5)
    flank = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))                        # noqa: E731
    chrom = flank(off) + ref + flank(4000)
    reads = event_reads(ref, off)
    recs = bamwriter.records_from_reads(reads, tid=0, qname_fmt="ev%d")
    bam, fa, bed = os.path.join(d, "e.bam"), os.path.join(d, "e.fa"), os.path.join(d, "e.bed")
    bamwriter.write_bam(bam, [("chrE", len(chrom))], recs)
    bamwriter.write_fasta(fa, [("chrE", chrom)])
    lines = [("chrE", off + 100, off + 2900)]
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % l for l in lines))
    return bam, fa, bed, lines, ref, off


def chain(gpu_lib, hb, hf, lines, path, junctions):
    """The report of the Python chain: every BED line its own region, Region.clip_sites over the positions it owns, Region.clip_junctions
    on those rows, io.ClipSites; and the same text from the two restatements' report_text on the chain's rows."""
    calls, jrows = [], []
    with uio.ClipSites(*GATE, 1) as st:
        if junctions:
            st.set_junctions(*REQ)
        for chrom, b, e in lines:
            res = pipeline.call_region(gpu_lib, hb, hf, chrom, b, e, keep_handle=True)
            a, z = res["score_range"][0], min(res["score_range"][1], e)
            R = res["region"]
            totals, rows, ev = R.clip_sites([(a, z)], *GATE, want_reads=True)
            t, j = R.clip_junctions(rows, *REQ)
            refseq = hf.fetch(chrom, R.beg, R.beg + R.npos - 1)
            assert np.array_equal(j, cj.run(refseq, R.beg, rows, *REQ)[1])
            qn = [res["qnames"][int(i)] for i in res["order"]]
            st.add(hb.tid(chrom), chrom, rows, ev, res["reads"], qn, junctions=j if junctions else None)
            evs = np.stack([ev[k] for k in region.CLIP_READ.names], axis=1).astype(np.int64).reshape(-1, 4)
            calls.append((hb.tid(chrom), chrom, rows, evs, dict(res["reads"], qnames=qn)))
            jrows.append(j)
            R.close()
        st.write(path)
    text = open(path).read()
    assert text == cj.report_text(calls, *GATE, 1, junctions=jrows if junctions else None, request=REQ)
    return text, jrows


def test_cli_junction_lines(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, ref, off = event_panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    want, jrows = chain(gpu_lib, hb, hf, lines, o("chain.tsv"), True)
    plain, _ = chain(gpu_lib, hb, hf, lines, o("chain0.tsv"), False)
    jl = [l.split("\t") for l in want.splitlines() if l.startswith("J\t")]
    assert len(jl) == 8 and {f[12] for f in jl} == {"DEL", "DUP", "INV"} and all(f[6] == "2" and f[14] != "." for f in jl), jl        # the expected J lines are not trivial
    assert {(int(f[2]) - 1 - off, f[3]): (f[12], int(f[13])) for f in jl} == {(x, "LR"[s]): (cj.CLASSES[k], n) for (x, s), (k, n, m) in expected_events().items()}
    vcf_without = run_cli(bam, fa, o("p.vcf.gz"), "-R", bed, "-t", "2", "--clip-sites-out", o("p.tsv"), "--clip-sites-reads", "1")
    vcf_with = run_cli(bam, fa, o("j.vcf.gz"), "-R", bed, "-t", "2", "--clip-sites-out", o("j.tsv"), "--clip-sites-reads", "1", *JOPTS)
    got, got_plain = open(o("j.tsv")).read(), open(o("p.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert got_plain == plain and vcf_with == vcf_without and len(vcf_with) > 100
    assert [l for l in got.splitlines() if not l.startswith(("J\t", "#J\t", "##clip_sites_junction_"))] == got_plain.splitlines()      # S, R and the other lines are those without the option
