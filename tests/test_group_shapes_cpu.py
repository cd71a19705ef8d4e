"""The reference side of tests/test_gpu_group_shapes.py, checked without a GPU: on every case of tests/group_cases.py the oracle equals the
pure-Python restatement of test_group.py (reasons, counters, the family / fragment structure with its flags and its inner order), every
case reaches what it is named for, and the scan_rounds and center_thresholds inputs tell a lost scan carry and a power one ulp off.
The last two are why a kernel with such a fault cannot pass the GPU file."""
import numpy as np
import pytest

import group_cases as gc
from test_group import py_group, py_structure, structure


def oracle_side(res):
    return res["filter_reason"].tolist(), int(res["n_amplicon"]), int(res["n_visited_qnames"]), structure(res)


def python_side(P, cols, **switch):
    reason, fams, n_amp, n_vis = py_group(P, cols, **switch)
    return reason.tolist(), n_amp, n_vis, py_structure(fams)


def features(res):
    """what a case is named for, read from the oracle's output alone"""
    fams, frags = structure(res)
    f = dict(reasons={int(r): int(c) for r, c in zip(*np.unique(res["filter_reason"], return_counts=True))}, n_kept=int(res["n_kept"]), n_fams=len(fams),
             idflags=sorted({x[2] for x in fams}), dflags=sorted({x[1] for x in fams}), largest_family=max([len(x[0]) for x in fams], default=0),
             largest_fragment=max([len(x) for x in frags], default=0), two_strand=0, frags_per_strand=0)
    frag_of = {i: k for k, fr in enumerate(frags) for i in fr}
    for seq, _, _ in fams:
        per = [len({frag_of[i] for s, i in seq if s == strand}) for strand in (0, 1)]
        if min(per) > 0:
            f["two_strand"] += 1
            f["frags_per_strand"] = max(f["frags_per_strand"], min(per))
    return f


@pytest.mark.parametrize("name,sub", gc.ALL, ids=gc.IDS)
def test_oracle_against_python(oracle_lib, name, sub):
    P, cols = gc.params(oracle_lib, name, sub)
    res = gc.reference(oracle_lib, name, sub)
    got, exp = oracle_side(res), python_side(P, cols)
    for k, what in enumerate(("filter_reason", "n_amplicon", "n_visited_qnames", "structure")):
        assert got[k] == exp[k], what
    assert len(cols["pos"]) <= 6000
    print("\n%s-%s: n=%d %s" % (name, sub, len(cols["pos"]), features(res)))


def test_sizes(oracle_lib):
    for n in (0, 1, 255, 256, 257):
        assert len(gc.case("sizes", n)[1]["pos"]) == n
    f = {s: features(gc.reference(oracle_lib, "sizes", s)) for s in gc.SUBCASES["sizes"]}
    assert f[0]["n_kept"] == 0 and f[1]["n_kept"] == 1 and all(f[n]["n_kept"] > 100 and f[n]["two_strand"] > 0 for n in (255, 256, 257))
    assert f["none_kept"]["n_kept"] == 0 and f["one_kept"]["n_kept"] == 1
    assert f["none_kept"]["reasons"] == {1: 100, 2: 100, 100: 100} and f["one_kept"]["reasons"] == {0: 1, 1: 99, 2: 100, 100: 100}
    assert gc.reference(oracle_lib, "sizes", "none_kept")["n_visited_qnames"] == 100


@pytest.mark.parametrize("sub", gc.SUBCASES["scan_rounds"])
def test_scan_rounds(oracle_lib, sub):
    P, cols = gc.params(oracle_lib, "scan_rounds", sub)
    res = gc.reference(oracle_lib, "scan_rounds", sub)
    assert P.fetch_tend - P.fetch_tbeg + 4020 == {76: 4096, 77: 4097, 1100: 5120, 1: 4021}[sub]
    f = features(res)
    assert f["reasons"][8] == 2 and f["idflags"] == [0x3, 0x7]
    # the piles of classes 0, 1 and 3 miss the weak amplicon test by tot = 2 002 > 2 000, that of class 2 passes it by 1 998: one read more or
    # less in a border sum flips a pile.  Every kept alignment that is not of the amplicon pile is not an amplicon.
    assert res["n_amplicon"] == gc.PILE
    lo, hi = cols["pos"].min() + 2000 - P.fetch_tbeg, cols["endpos"].max() - 1 + 2000 - P.fetch_tbeg
    assert lo == 11 - 1 and hi == sub + 3988 + 1              # one beyond the lowest and the highest admitted bin: the two OUT_OF_RANGE
    kept = res["filter_reason"] == 0
    assert (cols["mpos"][kept & (cols["flag"] == 0x53)] + 2000 - P.fetch_tbeg).min() == 11 and (cols["endpos"][kept] - 1 + 2000 - P.fetch_tbeg).max() == sub + 3988
    assert oracle_side(res) == python_side(P, cols)
    lost = python_side(P, cols, scan_round=1024)
    assert lost != oracle_side(res) and lost[1] > res["n_amplicon"]


def test_low_tbeg(oracle_lib):
    f = {s: features(gc.reference(oracle_lib, "low_tbeg", s)) for s in gc.SUBCASES["low_tbeg"]}
    at0 = {s: gc.reference(oracle_lib, "low_tbeg", s)["filter_reason"][gc.case("low_tbeg", s)[1]["pos"] == 0] for s in f}
    assert all((gc.case("low_tbeg", s)[1]["pos"] == 0).sum() >= 5 for s in f)
    assert (at0[0] == 0).all() and (at0[5] == 0).all()                       # position 0 is inside the window and the histograms
    assert set(at0[2001]) == {8} and set(at0[2002]) == {100}                 # the window begins at 0, then at 1
    assert all(f[s]["n_kept"] > 50 for s in f)


def test_every_reason(oracle_lib):
    f = features(gc.reference(oracle_lib, "every_reason", None))
    assert set(f["reasons"]) == {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 100, 101}
    assert f["reasons"][0] == 120 and all(f["reasons"][r] >= 6 for r in (1, 2, 3, 4, 5, 6, 7, 8, 9, 100, 101))


def test_mates_elsewhere(oracle_lib):
    _, cols, _, _ = gc.case("mates_elsewhere", None)
    res = gc.reference(oracle_lib, "mates_elsewhere", None)
    assert set(cols["tid"]) == {3} and set(cols["mtid"]) == {0, 3, 7, -1} and (cols["flag"] & 0x8).any()
    fams, _ = structure(res)
    fam_of = {i: k for k, (seq, _, _) in enumerate(fams) for _, i in seq}
    assert (res["filter_reason"] == 0).all()
    for pos in (gc.TB + 100, gc.TB + 300):          # equal positions, three mate references: three families of three
        rows = {m: [i for i in range(len(cols["pos"])) if cols["pos"][i] == pos and cols["mtid"][i] == m and cols["flag"][i] == 0x61 and cols["mpos"][i] in (5000, pos)] for m in (0, 3, 7)}
        assert all(len(v) == 3 and len({fam_of[i] for i in v}) == 1 for v in rows.values()) and len({fam_of[v[0]] for v in rows.values()}) == 3
    ab = np.abs(cols["isize"])
    assert ((ab >= 1500) & (ab < 2000)).any() and (ab >= 2000).any() and ((ab > 0) & (ab < 1500)).any()
    assert {d & 8 for _, d, _ in fams} == {0, 8}


def test_duplex_families(oracle_lib):
    mixed, big = (features(gc.reference(oracle_lib, "duplex_families", s)) for s in ("mixed", "big"))
    assert mixed["two_strand"] >= 3 and mixed["frags_per_strand"] >= 3 and mixed["largest_fragment"] == 5
    assert {0x9, 0xA, 0xB} <= set(mixed["idflags"]) and mixed["n_fams"] >= 2000
    res = gc.reference(oracle_lib, "duplex_families", "mixed")
    sizes = np.bincount(res["fam_id"])
    assert (sizes == 1).sum() == 2000 and (res["fam_idflag"] == 0x9).sum() >= 8 and (res["fam_idflag"] == 0xA).sum() >= 8
    # the five alignments of one name are not neighbours in the file
    five = [fr for fr in structure(res)[1] if len(fr) == 5][0]
    assert all(b - a > 1 for a, b in zip(five, five[1:]))
    assert big["largest_family"] == 5000 and big["two_strand"] >= 2 and big["frags_per_strand"] >= 1200


def test_hash_edges(oracle_lib):
    _, cols, _, _ = gc.case("hash_edges", None)
    res = gc.reference(oracle_lib, "hash_edges", None)
    assert res["filter_reason"].tolist()[:5] == [0, 101, 0, 0, 101]
    fams, frags = structure(res)
    assert (0, 2) in frags and (3,) in frags                  # A and B: one fragment; A outside the region: kept, alone (C is gone)
    first = [seq for seq, _, _ in fams if (0, 0) in seq][0]
    q17 = [int(cols["qname_hash17"][i]) for s, i in first if s == 0]
    assert q17 == sorted(q17) and {0, gc.U64, 1 << 63, (1 << 63) - 1} <= set(q17) and {s for s, _ in first} == {0, 1}
    n1 = 5 + 2 * 8 + 3
    assert (cols["umi_kind"][n1] == 1 and cols["umi_hash31"][n1] == 0 and cols["umi_hash17"][n1] == 0)
    fam_of = {i: k for k, (seq, _, _) in enumerate(fams) for _, i in seq}
    assert fam_of[n1] != fam_of[n1 + 1] == fam_of[n1 + 2]
    n3 = [fam_of[i] for i in range(n1 + 3, n1 + 10)]
    assert n3[0] == n3[6] and len(set(n3)) == 6


@pytest.mark.parametrize("mult", gc.SUBCASES["center_thresholds"])
def test_center_thresholds(oracle_lib, mult):
    P, cols = gc.params(oracle_lib, "center_thresholds", mult)
    res = gc.reference(oracle_lib, "center_thresholds", mult)
    assert res["n_amplicon"] == 0 and (res["filter_reason"] == 0).all() and set(res["fam_idflag"]) == {0x3}
    exact = oracle_side(res)
    assert exact == python_side(P, cols)
    low, high = python_side(P, cols, pow_scale=1.0 - 2.0 ** -52), python_side(P, cols, pow_scale=1.0 + 2.0 ** -52)
    if mult in gc.EXACT_MULTS:
        # per strand and histogram (the two classes of a strand meet in one family): of the nine groups the three with one count more
        # snap, so 9 * 2 - 3 families; a power one ulp low snaps the three equalities as well, one ulp high changes nothing
        assert len(exact[3][0]) == 4 * 15 and len(low[3][0]) == 4 * 12 and high == exact
    assert low != exact or high != exact


def test_exact_powers_are_exact():
    from fractions import Fraction
    for mult in gc.EXACT_MULTS:
        for d in (1, 2, 3):
            assert Fraction(mult ** d) == Fraction(mult) ** d
            for locnt, hicnt, dd, delta in gc._exact_groups(mult):
                assert dd != d or Fraction(hicnt + 1) == Fraction(locnt + 1) * Fraction(mult) ** d + delta


def test_inexact_constants_are_what_the_search_finds():
    for mult, found in gc.INEXACT.items():
        assert gc.search_inexact(mult) == found


def test_host_pow_constants_part_the_host_power_from_the_rounded_one():
    """where this host's pow is the rounded cube after all, the constants still tell one ulp (test_center_thresholds); nothing to find then"""
    import math
    for mult, [(locnt, hicnt, d)] in gc.HOST_POW.items():
        if math.pow(mult, 3.0) != gc.rounded_cube(mult):
            assert gc.search_host_pow([locnt + 1], [hicnt + 1]) == {mult: (locnt, hicnt, d)}


def test_call_again(oracle_lib):
    """the order of calls of the GPU test, on the oracle"""
    from uvc_amd import group
    first = oracle_side(gc.reference(oracle_lib, "duplex_families", "mixed"))
    for name, sub in (("duplex_families", "mixed"), ("sizes", 1), ("duplex_families", "mixed")):
        assert oracle_side(group.group_families(oracle_lib, *gc.params(oracle_lib, name, sub))) == (first if name != "sizes" else oracle_side(gc.reference(oracle_lib, name, sub)))
