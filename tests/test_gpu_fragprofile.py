"""Fragment lengths and reference end motifs of ranges from the device fragments and family units (uvcgpu_region_fragment_profile,
Region.fragment_profile) and the report built from them (uvc1-mi355x --fragment-profile-out).  Every number is an integer and is compared
for equality with tests/fragprofile_restatement.py, which restates the definitions from the read columns and the reference text alone:
  * hand-built reads that hold every case the definitions distinguish (fragments of 1, 2, 3 and 130 counted alignments, every kind, the
    flags and mapping qualities that take an alignment out, lengths around every bound and bin cap, a pile of 3000 equal pairs, the family
    shapes, ends on and off every edge of the region), against ranges placed on the edges of the overlap, CONTINUES and prev_end rules;
  * the suite's synthetic inputs against the ten range lists of test_gpu_coverage, from host and from device columns;
  * the refusals of the ABI, which launch nothing, leave the outputs alone and leave the handle usable, and the states the call is legal in;
  * the report of the command line against the Python chain (uvc_amd.pipeline regions + Region.fragment_profile + the restatement's text)."""
import ctypes as C
import os

import numpy as np
import pytest

import fragprofile_restatement as fp
from test_gpu_coverage import panel, range_lists, run_cli
from test_gpu_device_reads import DeviceColumns
from test_gpu_famstats import SITUATIONS
from test_gpu_parity import CASES
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
E = _ffi.ENUMS
TROW, ROW, EINVAL = E["UVC_FRAGPROF_TARGET_ROW"], E["UVC_FRAGPROF_ROW"], E["UVCGPU_EINVAL"]
B, LEN = 5_000_000, 3000   # the hand-built region: [B, B + LEN); SITUATIONS of the family test lie in [B + 50, B + 600)
MINQ = 20                  # the hand-built input is profiled with min_mapq 20
LIT_AT, LIT = 630, "ACGTTGCAAGGC"   # literal reference text, and the one pair [630, 638) on it
N_AT = 670                 # a reference base that is not A/C/G/T
M_OP, N_OP = 0, 3


# ------------------------------------------------------------------------------------------------ hand-built reads
def fw(x, n=30, mapq=60, extra=0):
    return (x, [(n, M_OP)], extra, mapq)


def rv(x, n=30, mapq=60, extra=0):
    return (x, [(n, M_OP)], 0x10 | extra, mapq)


def pr(x, L, n=30):
    """an FR pair over [x, x + L): a forward read at its left end, a reverse read at its right end"""
    return [fw(x, n), rv(x + L - n, n)]


def hand_built():
    """-> (reads, named): reads in the dict form of synth.generate_region; named[label] = frag_id of a fragment (the index of the fragment in
    fp.fragments: families, strands and fragments are numbered in the order they are made) or, for a family label, its fam_id."""
    rng = np.random.default_rng(43)
    fams, named = [], {}   # a family: (fragments of strand 0, fragments of strand 1); a fragment: a list of alignments (x, cigar, flag, mapq)

    def fam(s0, s1=(), label=None, frags=()):
        if label:
            named[label] = len(fams)
        n_before = sum(len(a) + len(b) for a, b in fams)
        for k, lab in enumerate(frags):
            named[lab] = n_before + k
        fams.append((list(s0), list(s1)))
    fam([[fw(1610)]])   # one alignment in front: the pairs behind it lie on odd alignment indices and straddle the lane and thread borders
    # the range situations of the family test, as pairs of the same spans
    fam([pr(200, 40)], frags=["lo_is_pos_end"])
    fam([pr(60, 40)], frags=["hi_is_pos_beg"])
    fam([pr(50, 60)], frags=["before_prev_end"])
    fam([pr(320, 40), pr(320, 40)], frags=["straddles_joint"])
    fam([pr(350, 40)], [pr(350, 40)], frags=["inside_continuing"])
    fam([pr(420, 40)], frags=["between"])
    fam([pr(495, 60)], frags=["spans_three"])
    # ends at the edges of the region (n = LEN positions hold a reference base), on the literal text and on the N.  set_reads refuses a read
    # that is not inside the region, so no fragment begins in front of it or ends behind its last position: the ends go off it through
    # fragments shorter than a motif
    fam([pr(0, 40)], frags=["lo_at_0"])
    fam([[fw(0, 3), rv(0, 4)]], frags=["y_is_4"])
    fam([[fw(0, 2), rv(0, 3)]], frags=["y_is_3"])
    fam([pr(LIT_AT, 8, 6)], frags=["literal"])
    fam([pr(N_AT - 2, 40)], frags=["n_in_left_motif"])
    fam([[fw(N_AT - 25, 20), rv(N_AT - 20, 22)]], frags=["n_in_right_motif"])
    fam([[fw(LEN - 4, 3), rv(LEN - 4, 4)]], frags=["x_plus_4_is_n"])
    fam([[fw(LEN - 3, 2), rv(LEN - 3, 3)]], frags=["x_plus_4_is_npos"])
    fam([[fw(2950, 30), rv(2970, 30)]], frags=["y_is_n"])
    # lengths around the bounds of short (100-150) and long (151-220) and around the last LEN bin; the longest that fits the region behind the
    # range situations, through a skip in the CIGAR
    for k, L in enumerate((99, 100, 150, 151, 220, 221, 1022, 1023, 1024)):
        fam([pr(700 + 10 * k, L)], frags=["L%d" % L])
    fam([[fw(700), (2000, [(30, M_OP), (930, N_OP), (30, M_OP)], 0x10, 60)]], frags=["L2290"])
    # kinds
    fam([[rv(800), fw(900)]], frags=["everted"])
    fam([[fw(1000), rv(990, 100)]], frags=["reverse_reaches_left"])
    fam([[fw(1000, 100), rv(1010)]], frags=["forward_reaches_right"])
    fam([[fw(1100)]], frags=["forward_only"])
    fam([[rv(1100)]], frags=["reverse_only"])
    fam([[fw(1200), fw(1250)]], frags=["two_forward"])
    fam([[fw(1300), rv(1400), rv(1420)]], frags=["three_alignments"])
    fam([[(fw if k % 2 == 0 else rv)(1500 + 100 * (k % 2) + k // 2) for k in range(130)]], frags=["run_of_130"])
    # what takes an alignment out: each placed so that counting it would change the span or the kind
    fam([[fw(1700, mapq=MINQ), rv(1800, mapq=MINQ), rv(1900, mapq=MINQ - 1)]], frags=["mapq_edge"])
    fam([[fw(2000), rv(2100), fw(1950, extra=0x100)]], frags=["secondary"])
    fam([[fw(2000), rv(2100), rv(2200, extra=0x800)]], frags=["supplementary"])
    fam([[fw(2300), rv(2400, extra=0x4)]], frags=["unmapped_mate"])
    fam([[fw(2500, mapq=0), rv(2600, mapq=MINQ - 1)]], frags=["all_uncounted"])
    # families
    fam([pr(1000, 160)], [pr(1005, 170)], label="pairs_in_both_units")      # template [1000, 1175): wider than either fragment
    fam([pr(1200, 200)], [[fw(1210)]], label="pairs_in_one_unit")
    fam([[fw(1300)]], [[rv(1300)]], label="not_sized")
    fam([pr(1400, 100), pr(1450, 100)], label="wide_in_one_unit")           # template [1400, 1550)
    fam([pr(1500, 167) for _ in range(3000)], label="pile")
    fam([[fw(1600)]])   # one alignment between the pile and the bulk: one of the two lies on odd alignment indices
    for _ in range(2000):
        mk = lambda: pr(int(rng.integers(700, 2500)), int(rng.integers(80, 400)))   # noqa: E731
        fam([mk() for _ in range(int(rng.integers(1, 4)))], [mk() for _ in range(int(rng.integers(0, 3)))])
    ref = rng.integers(0, 4, LEN)
    ref[LIT_AT:LIT_AT + len(LIT)] = ["ACGT".index(c) for c in LIT]
    refseq = "".join("ACGT"[b] for b in ref)
    refseq = refseq[:N_AT] + "N" + refseq[N_AT + 1:]
    cols = dict(pos=[], l_qseq=[], n_cigar=[], frag_id=[], fam_id=[], fam_strand=[], flag=[], mapq=[])
    cigars, bases, g = [], [], 0
    for f, units in enumerate(fams):
        for strand, frags in enumerate(units):
            for fr_ in frags:
                for x, cig, flag, mapq in fr_:
                    lq = sum(n for n, op in cig if op == M_OP)
                    cols["pos"].append(B + x); cols["l_qseq"].append(lq); cols["n_cigar"].append(len(cig)); cols["frag_id"].append(g); cols["fam_id"].append(f)
                    cols["fam_strand"].append(strand); cols["flag"].append(flag); cols["mapq"].append(mapq)
                    cigars += [(n << 4) | op for n, op in cig]
                    at = x
                    for n, op in cig:
                        if op == M_OP:
                            bases.append(ref[np.clip(np.arange(at, at + n), 0, LEN - 1)])
                        at += n
                g += 1
    n = len(cols["pos"])
    lq, nc = np.asarray(cols["l_qseq"], np.int32), np.asarray(cols["n_cigar"], np.int32)
    reads = dict(n_reads=n, pos=np.asarray(cols["pos"], np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), flag=np.asarray(cols["flag"], np.uint16),
                 mapq=np.asarray(cols["mapq"], np.uint8), nm=np.zeros(n, np.int32), l_qseq=lq, seq_off=np.concatenate(([0], np.cumsum(lq)))[:n].astype(np.int64),
                 cigar_off=np.concatenate(([0], np.cumsum(nc)))[:n].astype(np.int64), n_cigar=nc, frag_id=np.asarray(cols["frag_id"], np.int32), fam_id=np.asarray(cols["fam_id"], np.int32),
                 fam_strand=np.asarray(cols["fam_strand"], np.uint8), n_fams=len(fams), fam_dflag=np.ones(len(fams), np.uint8), bases=np.concatenate(bases).astype(np.uint8),
                 quals=np.full(int(lq.sum()), 30, np.uint8), cigars=np.asarray(cigars, np.uint32), tid=2, beg=B, end=B + LEN, refseq=refseq)
    return reads, named


WHOLE = [(B, B + LEN + 1, 0, 0)]
LISTS = {"the situations": SITUATIONS,
         "the whole region": WHOLE,
         "seventeen ranges": [(B + 600 + 140 * k, B + 600 + 140 * k + 100, B + 600 + 140 * k - (40 if k else 0), 0) for k in range(17)],
         "600 ranges of 5 bp (more than a block's window), every third continuing": [(B + 5 * k, B + 5 * k + 5, B + 5 * k if k else 0, int(k % 3 == 1)) for k in range(600)],
         "the literal text": [(B + LIT_AT, B + LIT_AT + 8, B + LIT_AT - 10, 0)]}


@pytest.fixture(scope="module")
def hand(gpu_lib):
    reads, named = hand_built()
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    frs = fp.fragments(reads, MINQ)
    yield reads, named, frs, fp.families(frs), R
    R.close()


def assert_rows(got, want, what):
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert got.shape == want.shape and got.dtype == np.int64, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:8]])


def assert_both(got, want, what):
    assert_rows(got[0], want[0], (what, "TARGET rows"))
    assert_rows(got[1], want[1], (what, "profile"))


def test_the_hand_built_input_holds_what_it_is_for(hand):
    reads, named, frs, fams, R = hand
    n = reads["n_reads"]
    assert reads["end"] - reads["beg"] <= 3000 and 15000 <= n <= 25000 and len(reads["refseq"]) == R.npos - 1 == LEN
    kind, L, lo, hi = frs["kind"], frs["L"], frs["lo"] - B, frs["hi"] - B
    g = lambda label: named[label]   # noqa: E731
    counted = (frs["nF"] + frs["nR"])
    # alignments per fragment, and fragments over the lane and thread borders
    assert {1, 2, 3, 130} <= set(counted.tolist()) and counted[g("run_of_130")] == 130 and kind[g("run_of_130")] == fp.KIND_PAIR
    first = np.flatnonzero(np.diff(reads["frag_id"], prepend=-1))          # the first alignment of every fragment
    size = np.diff(np.append(first, n))
    for border in (64, 256):
        over = [(a, s) for a, s in zip(first.tolist(), size.tolist()) if s >= 2 and a // border != (a + s - 1) // border]
        assert len(over) >= 5 and any(s == 2 for _, s in over), border
    a130 = first[g("run_of_130")]
    assert a130 // 64 != (a130 + 129) // 64
    # kinds
    assert [kind[g(k)] for k in ("spans_three", "everted", "reverse_reaches_left", "forward_reaches_right")] == [fp.KIND_PAIR] + [fp.KIND_OTHER] * 3
    assert [kind[g(k)] for k in ("forward_only", "reverse_only", "two_forward", "unmapped_mate")] == [fp.KIND_SINGLE] * 4
    assert kind[g("three_alignments")] == fp.KIND_PAIR and L[g("three_alignments")] == 150 and counted[g("three_alignments")] == 3
    # what takes an alignment out, against the same fragments with everything counted
    every = fp.fragments(dict(reads, flag=reads["flag"] & 0x10), 0)
    assert kind[g("all_uncounted")] == fp.KIND_NONE and every["kind"][g("all_uncounted")] == fp.KIND_PAIR
    assert set(reads["mapq"][reads["frag_id"] == g("mapq_edge")].tolist()) == {MINQ - 1, MINQ}
    assert L[g("mapq_edge")] == 130 and every["L"][g("mapq_edge")] == 230 and counted[g("mapq_edge")] == 2
    assert lo[g("secondary")] == 2000 and every["lo"][g("secondary")] - B == 1950
    assert hi[g("supplementary")] == 2130 and every["hi"][g("supplementary")] - B == 2230
    assert every["kind"][g("unmapped_mate")] == fp.KIND_PAIR
    for bit, label in ((0x100, "secondary"), (0x800, "supplementary"), (0x4, "unmapped_mate")):
        assert (reads["flag"][reads["frag_id"] == g(label)] & bit).any()
    # lengths
    for want in (99, 100, 150, 151, 220, 221, 1022, 1023, 1024, 2290):
        assert L[g("L%d" % want)] == want and kind[g("L%d" % want)] == fp.KIND_PAIR, want
    pile = (frs["fam"] == named["pile"])
    assert pile.sum() == 3000 and (L[pile] == 167).all() and (kind[pile] == fp.KIND_PAIR).all()
    # families
    at = {int(f): k for k, f in enumerate(fams["fam"].tolist())}
    assert fams["both"][at[named["pairs_in_both_units"]]] and fams["TL"][at[named["pairs_in_both_units"]]] == 175 > L[frs["fam"] == named["pairs_in_both_units"]].max()
    assert not fams["both"][at[named["pairs_in_one_unit"]]] and set(frs["strand"][frs["fam"] == named["pairs_in_one_unit"]].tolist()) == {0, 1}
    assert named["not_sized"] not in at and (frs["fam"] == named["not_sized"]).sum() == 2
    assert fams["TL"][at[named["wide_in_one_unit"]]] == 150 and not fams["both"][at[named["wide_in_one_unit"]]]
    # ends
    n_ref = LEN
    assert lo[g("lo_at_0")] == 0 and lo[kind >= 0].min() == 0 and hi[g("y_is_4")] == 4 and hi[g("y_is_3")] == 3
    assert lo[g("x_plus_4_is_n")] + 4 == n_ref and lo[g("x_plus_4_is_npos")] + 4 == n_ref + 1 and hi[g("y_is_n")] == n_ref == hi[g("x_plus_4_is_n")] == hi[kind >= 0].max()
    assert all(kind[g(k)] == fp.KIND_PAIR for k in ("lo_at_0", "y_is_4", "y_is_3", "x_plus_4_is_n", "x_plus_4_is_npos", "y_is_n"))
    ref = reads["refseq"]
    st = lambda label, right: fp.end_state(ref, int(hi[g(label)] if right else lo[g(label)]), right)[0]   # noqa: E731
    assert [st("lo_at_0", False), st("x_plus_4_is_n", False), st("x_plus_4_is_npos", False)] == ["ok", "ok", "off"]
    assert [st("y_is_4", True), st("y_is_3", True), st("y_is_n", True), st("x_plus_4_is_npos", True)] == ["ok", "off", "ok", "ok"]
    assert fp.end_state(ref, -1, False)[0] == "off" and fp.end_state(ref, n_ref + 1, True)[0] == "off"   # (what no read of a region can reach)
    assert ref[N_AT] == "N" and st("n_in_left_motif", False) == "no_ref" and st("n_in_right_motif", True) == "no_ref" and st("n_in_right_motif", False) == "ok"
    # one motif by hand: the pair [630, 638) on ACGTTGCA: left end ACGT = 0*64 + 1*16 + 2*4 + 3, right end the reverse complement of TGCA = TGCA = 3*64 + 2*16 + 1*4 + 0
    assert ref[LIT_AT:LIT_AT + 12] == "ACGTTGCAAGGC" and (lo[g("literal")], hi[g("literal")]) == (LIT_AT, LIT_AT + 8)
    assert fp.end_state(ref, LIT_AT, False) == ("ok", 27) and fp.end_state(ref, LIT_AT + 8, True) == ("ok", 228)
    # ... and the restatement's own rows show the range situations: literal pair and family counts of the six ranges
    rows, prof = fp.rows_and_profile(frs, fams, SITUATIONS, B, ref)
    assert rows[:, fp.PAIRS].tolist() == [1, 2, 2, 1, 1, 1] and rows[:, fp.FAMILIES].tolist() == [1, 1, 1, 1, 1, 1]
    assert prof[fp.PAIRS] == 5 and prof[fp.FAMILIES] == 3 and prof[fp.FAMILIES_BOTH] == 1
    whole, wprof = fp.rows_and_profile(frs, fams, WHOLE, B, ref)
    assert (whole[0, :7] > 0).all() and np.array_equal(whole[0], wprof[:TROW]) and whole[0, fp.FAMILIES] == len(fams["fam"])
    assert (wprof[[fp.FAMILIES_BOTH, fp.ENDS, fp.ENDS_OFF, fp.ENDS_NO_REF]] > 0).all() and wprof[fp.ENDS_NO_REF] >= 2 and wprof[fp.ENDS_OFF] == 2
    assert wprof[fp.LEN + 1022] == 1 and wprof[fp.LEN + 1023] == 3 and wprof[fp.LEN + 167] >= 3000 and wprof[fp.SHORT] >= 2 and wprof[fp.LONG] >= 3002


def test_hand_built_rows_equal_the_restatement(hand):
    reads, named, frs, fams, R = hand
    for what, ranges in LISTS.items():
        got = R.fragment_profile(ranges, min_mapq=MINQ)
        assert_both(got, fp.rows_and_profile(frs, fams, ranges, B, reads["refseq"]), what)
        assert got[0].any() and got[1].any(), what
        again = R.fragment_profile(ranges, min_mapq=MINQ)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes(), (what, "two calls, the same bytes")
    # the motif worked out by hand, from the device
    rows, prof = R.fragment_profile(LISTS["the literal text"], min_mapq=MINQ)
    assert rows[0].tolist() == [1, 0, 0, 8, 0, 0, 1, 0] and prof[fp.ENDS] == 2 and prof[fp.MOTIF + 27] == 1 and prof[fp.MOTIF + 228] == 1 and prof[fp.MOTIF:].sum() == 2
    assert prof[fp.LEN + 8] == 1 and prof[fp.FAMLEN + 8] == 1


def test_hand_built_requests_equal_the_restatement(hand):
    """other gates and bounds than the defaults: every alignment counted, and bounds that cut the pile in and out"""
    reads, named, _, _, R = hand
    for min_mapq, short, long in ((0, (100, 150), (151, 220)), (MINQ - 1, (0, 166), (167, 167)), (255, (0, 0), (0, 2000000000)), (60, (168, 1023), (1024, 5000))):
        frs = fp.fragments(reads, min_mapq)
        fams = fp.families(frs)
        for what in ("the whole region", "seventeen ranges"):
            got = R.fragment_profile(LISTS[what], min_mapq=min_mapq, short=short, long=long)
            assert_both(got, fp.rows_and_profile(frs, fams, LISTS[what], B, reads["refseq"], short, long), (what, min_mapq, short, long))


# ------------------------------------------------------------------------------------------------ synthetic inputs
@pytest.mark.parametrize("name", ["umi_duplex_2kb_400x", "config4shape_1kb_2000x_duplex", "config2shape_5kb_300x"])
def test_synthetic_rows_equal_the_restatement(name, gpu_lib):
    reads = synth.generate_region(**CASES[name])
    frs = fp.fragments(reads, 0)
    fams = fp.families(frs)
    p = region.default_params(gpu_lib)
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    cols = DeviceColumns(reads)
    Rd = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Rd.set_reads_device((cols.soa, cols))
    rng = np.random.default_rng(17)
    n_lists = 0
    for what, pairs in range_lists(rng, R.beg, R.npos):
        ranges = [(a, b, pairs[k - 1][1] if k else 0, 0) for k, (a, b) in enumerate(pairs)]
        got = R.fragment_profile(ranges)
        assert_both(got, fp.rows_and_profile(frs, fams, ranges, R.beg, reads["refseq"]), (name, what))
        for other, why in ((R.fragment_profile(ranges), "two calls, the same bits"), (Rd.fragment_profile(ranges), "device columns")):
            assert np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1]), (name, what, why)
        n_lists += 1
    assert n_lists == 10
    beg, end = R.beg, R.beg + R.npos
    rows, whole = R.fragment_profile([(beg, end, 0, 0)])
    print(name, dict(zip(fp.SUMMARY_NAMES, whole[fp.SUMMARY_WORDS].tolist())))
    assert whole[:3].sum() > 0 and np.array_equal(rows[0], whole[:TROW])
    assert whole[fp.LEN:fp.LEN + fp.NLEN].sum() == whole[fp.PAIRS] and whole[fp.FAMLEN:fp.FAMLEN + fp.NLEN].sum() == whole[fp.FAMILIES]
    assert whole[[fp.ENDS, fp.ENDS_OFF, fp.ENDS_NO_REF]].sum() == 2 * whole[fp.PAIRS] and whole[fp.MOTIF:].sum() == whole[fp.ENDS]
    cuts = [beg, beg + 70, beg + 71, beg + 200, beg + R.npos // 2, end - 5, end]
    _, part = R.fragment_profile([(a, b, a if k else 0, 0) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))])
    assert np.array_equal(part, whole), "the profile over a partition is the profile of the whole: every object once"
    Rd.close(); cols.free(); R.close()


# ------------------------------------------------------------------------------------------------ argument checks and states
def test_refusals_and_legal_states(gpu_lib):
    reads = synth.generate_region(**CASES["umi_duplex_2kb_400x"])
    frs = fp.fragments(reads, 0)
    fams = fp.families(frs)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, end = R.beg, R.beg + R.npos
    fn = gpu_lib.dll.uvcgpu_region_fragment_profile
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    sentinel = -0x5151515151515151

    def call(ranges, n=None, null=(), req=(0, 100, 150, 151, 220)):
        arr = (_ffi.UvcFamilyRange * len(ranges))(*[_ffi.UvcFamilyRange(*q) for q in ranges])
        rq = _ffi.UvcFragmentProfileRequest(*req)
        rows, prof = np.full((len(ranges), TROW), sentinel, np.int64), np.full(ROW, sentinel, np.int64)
        rc = fn(R.h, None if "ranges" in null else arr, len(ranges) if n is None else n, None if "req" in null else C.byref(rq),
                None if "out_ranges" in null else rows.ctypes.data, None if "out_profile" in null else prof.ctypes.data)
        return rc, rows, prof, gpu_lib.last_error()

    ok = [(beg + 5, beg + 100, beg + 5, 0), (beg + 100, beg + 101, beg + 100, 1), (beg + 300, end, beg + 150, 0)]
    rc, rows, prof, msg = call(ok)
    assert rc == EINVAL and "set_reads" in msg and "fragment_profile" in msg and (rows == sentinel).all() and (prof == sentinel).all()
    R.set_reads(reads)
    want = fp.rows_and_profile(frs, fams, ok, R.beg, reads["refseq"])
    assert want[0].any() and want[1].any()
    assert_both(R.fragment_profile(ok), want, "after set_reads, before accumulate")
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250, beg, 0), (beg + 10, beg + 50, beg, 0)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50, beg, 0), (beg + 49, beg + 60, beg + 49, 0)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50, beg, 0), (beg + 60, beg + 60, beg + 50, 0)]), "range 1"),
        ("reversed", dict(ranges=[(beg + 50, beg + 10, beg, 0)]), "range 0"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10, beg - 1, 0)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20, beg, 0), (end - 3, end + 1, beg + 20, 0)]), "range 1"),
        ("prev_end behind the begin", dict(ranges=[(beg + 10, beg + 20, beg + 11, 0)]), "range 0"),
        ("a decreasing prev_end", dict(ranges=[(beg + 10, beg + 20, beg + 10, 0), (beg + 40, beg + 50, beg + 9, 0)]), "range 1"),
        ("prev_end below the previous end", dict(ranges=[(beg + 10, beg + 20, beg + 5, 0), (beg + 40, beg + 50, beg + 19, 0)]), "range 1"),
        ("unknown flag bits", dict(ranges=[(beg + 10, beg + 20, beg, 0), (beg + 20, beg + 30, beg + 20, 2)]), "range 1"),
        ("a negative flag word", dict(ranges=[(beg + 10, beg + 20, beg, -1)]), "range 0"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("a negative count", dict(ranges=ok, n=-3), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null=("ranges",)), "NULL"),
        ("NULL req", dict(ranges=ok, null=("req",)), "NULL"),
        ("NULL out_ranges", dict(ranges=ok, null=("out_ranges",)), "NULL"),
        ("NULL out_profile", dict(ranges=ok, null=("out_profile",)), "NULL"),
        ("min_mapq below 0", dict(ranges=ok, req=(-1, 100, 150, 151, 220)), "min_mapq"),
        ("min_mapq above 255", dict(ranges=ok, req=(256, 100, 150, 151, 220)), "min_mapq"),
        ("short_lo below 0", dict(ranges=ok, req=(0, -1, 150, 151, 220)), "negative"),
        ("short_hi below 0", dict(ranges=ok, req=(0, 0, -150, 151, 220)), "negative"),
        ("long_lo below 0", dict(ranges=ok, req=(0, 100, 150, -151, 220)), "negative"),
        ("long_hi below 0", dict(ranges=ok, req=(0, 100, 150, 0, -1)), "negative"),
        ("short_lo above short_hi", dict(ranges=ok, req=(0, 151, 150, 151, 220)), "short_lo"),
        ("long_lo above long_hi", dict(ranges=ok, req=(0, 100, 150, 221, 220)), "long_lo"),
    ]
    for what, kw, word in bad_calls:
        rc, rows, prof, msg = call(**kw)
        assert rc == EINVAL and word in msg and "fragment_profile" in msg, (what, rc, msg)
        assert (rows == sentinel).all() and (prof == sentinel).all(), what
        assert_both(R.fragment_profile(ok), want, "a valid call after: " + what)
    # accumulate and scores neither are needed nor get in the way: the fragments belong to the reads, a releasing score gives up the planes only
    R.accumulate()
    assert_both(R.fragment_profile(ok), want, "after accumulate")
    R.score()
    assert_both(R.fragment_profile(ok), want, "after a plain score")
    R.score(release_state=True)
    assert_both(R.fragment_profile(ok), want, "after a releasing score")
    R.accumulate()
    gen = R.score_stream(4096)
    first = next(gen)
    assert_both(R.fragment_profile(ok), want, "while a score stream is open")
    assert len(first[0]["refpos"]) > 0
    for _ in gen:
        pass
    assert_both(R.fragment_profile(ok), want, "after the stream")
    # a region with zero reads gives zeros; a reset takes the fragments away
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and k != "fam_dflag" else v) for k, v in reads.items()}
    empty["n_reads"] = 0
    R.set_reads(empty)
    rc, rows, prof, msg = call(ok)
    assert rc == 0 and not rows.any() and not prof.any()
    R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    rc, rows, prof, msg = call(ok)
    assert rc == EINVAL and "set_reads" in msg and (rows == sentinel).all() and (prof == sentinel).all()
    R.close()


def test_a_library_without_the_symbol_says_so(oracle_lib):
    reads = synth.generate_region(**CASES["tiny_600bp_5x"])
    R = region.Region(oracle_lib, region.default_params(oracle_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    with pytest.raises(region.UvcError, match="region_fragment_profile"):
        R.fragment_profile([(R.beg, R.beg + 10)])
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def chain_report(gpu_lib, hb, hf, lines, clen, **req):
    """The report from the Python chain: one region per BED line (uvc_amd.pipeline.call_region), Region.fragment_profile with the line as the
    one piece and prev_end = the largest end of the lines before it on the contig (at most the line's begin; 0 for the first), the
    restatement's text.  -> (text, the summed profile of the run)."""
    total, per_target, targets, reach = np.zeros(ROW, np.int64), [], [], {}
    for chrom, b, e, name in lines:
        cb, ce = max(0, b), min(e, clen[chrom])
        row = np.zeros(TROW, np.int64)
        res = pipeline.call_region(gpu_lib, hb, hf, chrom, cb, ce, keep_handle=True) if ce > cb else None
        if res is not None:
            rows, prof = res["region"].fragment_profile([(cb, ce, min(cb, reach.get(chrom, 0)), 0)], **req)
            res["region"].close()
            row = rows[0]
            total += prof
        if ce > cb:
            reach[chrom] = max(reach.get(chrom, 0), ce)
        per_target.append(row)
        targets.append((chrom, b, e, name))
    return fp.report_text(targets, per_target, total, req.get("min_mapq", 0), req.get("short", (100, 150)), req.get("long", (151, 220))), total


def sections_of(text):
    """-> (summary dict, [(label, fragments, families)], target lines as lists)"""
    summary = {l.split("\t")[0]: int(l.split("\t")[1]) for l in text.split("#summary\n")[1].split("#length")[0].splitlines()}
    length = [l.split("\t") for l in text.split("#length\tfragments\tfamilies\n")[1].split("#end_motif")[0].splitlines()]
    targets = [l.split("\t") for l in text.split(fp.TARGET_HEADER + "\n")[1].splitlines()]
    return summary, length, targets


def test_cli_fragment_profile_report(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    want, total = chain_report(gpu_lib, hb, hf, lines, clen)
    assert total[:3].sum() > 100 and total[fp.MOTIF:].sum() == total[fp.ENDS]
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2")
    vcf_with = run_cli(bam, fa, o("f.vcf.gz"), "-R", bed, "-t", "2", "--fragment-profile-out", o("f.tsv"))
    got = open(o("f.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100
    # the sub-options reach the device call and the header
    req = dict(min_mapq=30, short=(50, 120), long=(121, 400))
    want_req, _ = chain_report(gpu_lib, hb, hf, lines, clen, **req)
    assert run_cli(bam, fa, o("q.vcf.gz"), "-R", bed, "-t", "4", "--fragment-profile-out", o("q.tsv"), "--fragment-profile-min-mapq", "30", "--fragment-profile-short", "50-120",
                   "--fragment-profile-long=121-400") == vcf_without
    assert open(o("q.tsv")).read() == want_req
    # all seven reports together: this one has the bytes of the run that writes it alone
    vcf_all = run_cli(bam, fa, o("a.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("c7.tsv"), "--error-profile-out", o("e7.tsv"), "--family-stats-out", o("s7.tsv"), "--callable-out", o("k7.bed"),
                      "--msi-out", o("m7.tsv"), "--read-profile-out", o("r7.tsv"), "--fragment-profile-out", o("f7.tsv"))
    assert vcf_all == vcf_without and open(o("f7.tsv")).read() == got
    assert all(os.path.getsize(o(n)) > 0 for n in ("c7.tsv", "e7.tsv", "s7.tsv", "k7.bed", "m7.tsv", "r7.tsv"))
    # --tile cuts the long line: a fragment next to a cut is the fragment of the tile's own fetch, so only the VCF and the
    # report's own consistency are promised
    vcf_tile0 = run_cli(bam, fa, o("k0.vcf.gz"), "-R", bed, "-t", "2", "--tile", "1000")
    assert run_cli(bam, fa, o("k.vcf.gz"), "-R", bed, "-t", "2", "--tile", "1000", "--fragment-profile-out", o("k.tsv")) == vcf_tile0
    s, length, targets = sections_of(open(o("k.tsv")).read())
    assert s["pairs"] == sum(int(l[1]) for l in length) and s["families"] == sum(int(l[2]) for l in length) and s["pairs"] + s["others"] + s["singles"] > 100
    assert [t[:4] for t in targets] == [[c, str(b), str(e), n or "."] for c, b, e, n in lines]
    # fixed windows without a BED file
    vcf_w0 = run_cli(bam, fa, o("w0.vcf.gz"), "-t", "2", "--tile", "1000000")
    assert run_cli(bam, fa, o("w.vcf.gz"), "-t", "2", "--tile", "1000000", "--fragment-profile-window", "5000", "--fragment-profile-out", o("w.tsv")) == vcf_w0
    s, length, targets = sections_of(open(o("w.tsv")).read())
    assert [(r[0], int(r[1]), int(r[2])) for r in targets] == [(c, q * 5000, min((q + 1) * 5000, clen[c])) for c in ("chrA", "chrB", "chrC") for q in range(-(-clen[c] // 5000))]
    kinds = s["pairs"] + s["others"] + s["singles"]
    # every window is a target of its own: a fragment over a window border counts in both, so the target lines sum to at least the summary
    assert kinds > 100 and sum(int(r[4]) + int(r[5]) + int(r[6]) for r in targets) >= kinds and all(r[4:] == ["0"] * 7 for r in targets if r[0] == "chrC")
    # ... and the same windows cut by --tile: every object still once in the summary's own terms
    vcf_wt0 = run_cli(bam, fa, o("x0.vcf.gz"), "-t", "2", "--tile", "2000")
    assert run_cli(bam, fa, o("x.vcf.gz"), "-t", "2", "--tile", "2000", "--fragment-profile-window", "5000", "--fragment-profile-out", o("x.tsv")) == vcf_wt0
    s2, length2, targets2 = sections_of(open(o("x.tsv")).read())
    assert [t[:4] for t in targets2] == [t[:4] for t in targets] and s2["pairs"] == sum(int(l[1]) for l in length2) and s2["ends"] + s2["ends_off_region"] + s2["ends_no_ref"] == 2 * s2["pairs"]
