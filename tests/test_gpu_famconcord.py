"""uvcgpu_region_family_concordance (Region.family_concordance) and the report built from it (uvc1-mi355x --family-concordance-out).  Every
number is an integer and is compared for equality:
  * the row of the HIP library against the restatement of the contract (tests/famconcord_restatement.py) on families placed by hand
    (tests/famconcord_cases.py), on both platforms, over many range lists and with parameters off their defaults; each test first asserts on
    the RESTATED row that the cells it is about are not zero, so that a kernel that writes zeros cannot pass;
  * at size, identities that tie the row to the bit-exact planes (FAM cDP12 / cDP21, DUPLEX dDP1 / dDP2), without a restatement;
  * that the call moves nothing else, the refusals of the ABI, and the command line's report against the Python chain."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import famconcord_cases as fc
import famconcord_restatement as fr
from test_gpu_coverage import panel, run_cli
from test_gpu_parity import CASES
from util import run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
E = _ffi.ENUMS
ROW, EINVAL = E["UVC_FAMCONC_ROW"], E["UVCGPU_EINVAL"]
LINK_M, LINK_NN, BASE_NN = 6, 13, 5
FAM = "cDP1 cDP12 cDP2 cDP3 cDPM cDPm cDP21 cDPD".split()


def params_of(lib, platform, setting=()):
    P = region.default_params(lib, platform=platform)
    for k, v in setting:
        region.set_param(P, None, k, v)
    return P


@functools.lru_cache(maxsize=None)
def restated_votes(case, platform, setting=()):
    """(reads, P, codes, proton, votes) of a case: the expensive half of the restatement, once per (case, platform, setting)"""
    reads = getattr(fc, case)()
    P = params_of(region.gpu_lib(), platform, setting)
    kw = fr.restated_inputs(reads, P, platform)
    return reads, P, kw["codes"], kw["proton"], fr.all_unit_votes(reads, P, **kw)


def want_row(case, platform, ranges, setting=()):
    reads, P, codes, proton, votes = restated_votes(case, platform, setting)
    return fr.concordance_row(reads, votes, P, codes, proton, ranges)


def whole(reads):
    return [(reads["beg"], reads["end"] + 1)]


def assert_row(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


def section(row, name):
    first, words = {n: (f, w) for n, f, w in fr.SECTIONS}[name]
    return row[first:first + words]


# ------------------------------------------------------------------------------------------------ 1. planted families, both platforms
@pytest.mark.parametrize("platform", [1, 2], ids=["illumina", "iontorrent"])
def test_planted_families_equal_the_restatement(platform, gpu_lib):
    reads = fc.planted()
    want = want_row("planted", platform, tuple(whole(reads)))
    base_pos = section(want, "base_pos").reshape(2, fr.NBIN, 2)
    link_pos = section(want, "link_pos").reshape(fr.NBIN, 2)
    base = section(want, "base").reshape(2, fr.NBIN, fr.NBASE, fr.NBASE)
    link = section(want, "link").reshape(fr.NBIN, fr.NLINK, fr.NLINK)
    off_diag = ~np.eye(fr.NBASE, dtype=bool)
    assert (base_pos[:, :, 0].sum(0) > 0).all() and (link_pos[:, 0] > 0).all(), "every depth bin"
    assert base[:, :, off_diag].sum() > 0 and (base_pos[:, :, 0] > base_pos[:, :, 1]).any(), "dissenting bases"
    assert base_pos[1].sum() > 0, "a consensus that is not the reference (the 2:2 tie or the quality-0 dissent)"
    assert link[:, 0, 1:7].sum() > 0, "an InDel out-voted by LINK_M"
    assert want[fr.C["base_no_ref"]] > 0 and want[fr.C["base_no_vote"]] > 0 and want[fr.C["link_no_vote"]] > 0
    assert want[fr.C["units_seen"]] == len(fc.UNIT_SIZES) + 3 + 4 and not section(want, "dup_base").any()
    R = run_region(gpu_lib, reads, params=params_of(gpu_lib, platform))
    try:
        assert_row(R.family_concordance(whole(reads)), want, "the whole region")
    finally:
        R.close()


# ------------------------------------------------------------------------------------------------ 2. duplex
@pytest.mark.parametrize("padded_flag", [2, 3], ids=["default", "padded_deletions_ignored"])
def test_duplex_votes_equal_the_restatement(padded_flag, gpu_lib):
    reads = fc.duplex_planted()
    setting = (("microadjust_padded_deletion_flag", padded_flag),)
    want = want_row("duplex_planted", 1, tuple(whole(reads)), setting)
    db = section(want, "dup_base").reshape(4, 7, 7)
    dl = section(want, "dup_link").reshape(9, 9)
    two = db[:, :6, :6]
    assert two[:, np.arange(6), np.arange(6)].sum() > 0, "agreeing strands"
    assert db[1, 1, 3] == 1, "the C / T conflict"
    assert dl[0, 1:8].sum() > 0, "a deletion on strand 1 alone"
    assert db[:, :6, 6].sum() > 0 and db[:, 6, :6].sum() > 0, "positions one strand covers (partial overlap) or votes on (the 1:1 tie) alone"
    assert want[fr.C["duplex_no_vote"]] > 0
    # five duplex families; the sixth has both strands and no duplex tag: its positions are in no duplex cell
    spans = sum(80 + 2 for _ in range(3)) + (50 + 80 + 1) + (80 + 2)
    assert db.sum() + dl.sum() + want[fr.C["duplex_no_vote"]] + want[fr.C["duplex_base_no_ref"]] == 2 * spans
    other = want_row("duplex_planted", 1, tuple(whole(reads)), (("microadjust_padded_deletion_flag", 5 - padded_flag),))
    assert not np.array_equal(want, other), "the padded-deletion rule changes the row"
    R = run_region(gpu_lib, reads, params=params_of(gpu_lib, 1, setting))
    try:
        assert_row(R.family_concordance(whole(reads)), want, "the whole region")
    finally:
        R.close()


# ------------------------------------------------------------------------------------------------ 3. ranges
def test_range_lists_pick_their_positions_and_rows_add(gpu_lib):
    reads = fc.planted()
    beg, end = reads["beg"], reads["end"] + 1
    mid = beg + 200                                        # inside several units, none of which begins there, and inside the window 192..255
    lists = {
        "one position": [(mid, mid + 1)],
        "the first position": [(beg, beg + 1)],
        "the last position": [(end - 1, end)],
        "a boundary inside a unit and a window, left part": [(beg, mid)],
        "right part": [(mid, end)],
        "200 ranges of 3 bp": [(beg + 3 * k, beg + 3 * k + 3) for k in range(200)],          # they touch: the whole of [beg, beg + 600)
        "every other one of them": [(beg + 3 * k, beg + 3 * k + 3) for k in range(0, 200, 2)],
        "the others": [(beg + 3 * k, beg + 3 * k + 3) for k in range(1, 200, 2)],
        "64-position boundaries": [(beg, beg + 64), (beg + 64, beg + 127), (beg + 127, beg + 129), (beg + 192, beg + 448), (beg + 449, beg + 512)],
        "the whole region": [(beg, end)],
    }
    R = run_region(gpu_lib, reads, params=params_of(gpu_lib, 1))
    try:
        got = {}
        for what, ranges in lists.items():
            want = want_row("planted", 1, tuple(ranges))
            assert want[fr.C["unit_positions"]] > 0 and (section(want, "base").any() or what == "the last position"), what
            got[what] = R.family_concordance(ranges)
            assert_row(got[what], want, what)
        # row(A u B) = row(A) + row(B); two "tiles" of owned positions sum to the whole
        assert_row(got["a boundary inside a unit and a window, left part"] + got["right part"], got["the whole region"], "two tiles")
        assert sorted(lists["every other one of them"] + lists["the others"]) == lists["200 ranges of 3 bp"]
        assert_row(got["every other one of them"] + got["the others"], got["200 ranges of 3 bp"], "A u B")
        assert got["one position"][fr.C["unit_positions"]] >= 2 and got["one position"][fr.C["units_seen"]] == 0
    finally:
        R.close()


# ------------------------------------------------------------------------------------------------ 4. parameters off default
@pytest.mark.parametrize("value", [7, 38])
def test_a_moved_vote_threshold_moves_the_row(value, gpu_lib):
    """fam_thres_highBQ_snv = 7: the pair whose mates disagree 37 : 30 votes at that position (2 * 37 - 67 = 7); 38: no base of quality 37
    votes, LINK votes alone are left."""
    reads = fc.planted()
    setting = (("fam_thres_highBQ_snv", value),)
    want = want_row("planted", 1, tuple(whole(reads)), setting)
    dflt = want_row("planted", 1, tuple(whole(reads)))
    assert not np.array_equal(want, dflt) and section(want, "link").any()
    if value == 7:
        assert section(want, "base").sum() == section(dflt, "base").sum() + 1
    else:   # what is left are the votes of the deletion's padded symbol, whose value is no base quality
        assert want[fr.C["base_no_vote"]] > dflt[fr.C["base_no_vote"]] and section(want, "base").reshape(2, fr.NBIN, fr.NBASE, fr.NBASE)[:, :, :BASE_NN].sum() == 0
    R = run_region(gpu_lib, reads, params=params_of(gpu_lib, 1, setting))
    try:
        assert_row(R.family_concordance(whole(reads)), want, "fam_thres_highBQ_snv = %d" % value)
    finally:
        R.close()


# ------------------------------------------------------------------------------------------------ 5. tie to the bit-exact planes, at size
def test_the_row_ties_to_the_planes_on_a_duplex_umi_tile(gpu_lib):
    reads = synth.generate_region(**CASES["config4shape_1kb_2000x_duplex"])
    assert set(reads["refseq"]) <= set("ACGT"), "the identities need a reference base at every position of the ranges"
    beg, end = reads["beg"], reads["end"]                  # [beg, end): every position with a reference base (the plane of `end` has none)
    R = run_region(gpu_lib, reads)
    try:
        lists = [[(beg, end)], [(beg + 3, beg + 500), (beg + 500, beg + 501), (beg + 640, end - 7)]]
        fam, dup = R.fetch("FAM").astype(np.int64), R.fetch("DUPLEX").astype(np.int64)
        for ranges in lists:
            inside = np.zeros(R.npos, bool)
            for a, b in ranges:
                inside[a - beg:b - beg] = True
            row = R.family_concordance(ranges)
            base_pos = section(row, "base_pos").reshape(2, fr.NBIN, 2)
            link_pos = section(row, "link_pos").reshape(fr.NBIN, 2)
            cdp12, cdp21 = fam[:, FAM.index("cDP12")][:, :, inside], fam[:, FAM.index("cDP21")][:, :, inside]
            assert row[fr.C["base_no_ref"]] == 0 and row[fr.C["duplex_base_no_ref"]] == 0
            assert base_pos[:, :, 0].sum() == cdp12[:, :BASE_NN + 1].sum() > 0
            assert base_pos[:, 0, 0].sum() == cdp21[:, :BASE_NN + 1].sum() > 0
            assert link_pos[:, 0].sum() == cdp12[:, LINK_M:LINK_NN + 1].sum() > 0
            assert link_pos[0, 0] == cdp21[:, LINK_M:LINK_NN + 1].sum() > 0
            assert base_pos[:, 1:, 0].sum() > 0, "families of two and more fragments"
            db = section(row, "dup_base").reshape(4, 7, 7)
            dl = section(row, "dup_link").reshape(9, 9)
            assert db.sum() == dup[0][:BASE_NN + 1][:, inside].sum() > 0 and db[:, :6, :6].sum() == dup[1][:BASE_NN + 1][:, inside].sum() > 0
            assert dl.sum() == dup[0][LINK_M:LINK_NN + 1][:, inside].sum() > 0 and dl[:8, :8].sum() == dup[1][LINK_M:LINK_NN + 1][:, inside].sum() > 0
            # every vote of the BASE section belongs to a counted position: the consensus symbol's votes are the diagonal
            base = section(row, "base").reshape(2, fr.NBIN, fr.NBASE, fr.NBASE)
            assert base.sum() >= base_pos[:, :, 0].sum() and base[:, 0].sum() == base_pos[:, 0, 0].sum()      # bin 1: one vote per position
    finally:
        R.close()


# ------------------------------------------------------------------------------------------------ 6. nothing else moves
def test_the_call_moves_nothing_else_and_repeats_its_bits(gpu_lib):
    reads = synth.generate_region(**CASES["umi_duplex_2kb_400x"])
    groups = ["PREP32", "THRES", "SEG32", "SEG64", "BQSUM", "FRAG", "FAM", "FAMINFO32", "FAMINFO64", "DUPLEX", "VQ", "RTR"]
    out = []
    for with_call in (False, True):
        R = run_region(gpu_lib, reads)
        rows = [R.family_concordance(whole(reads)) for _ in range(2)] if with_call else None
        planes = [R.fetch(g).tobytes() for g in groups]
        alleles = R.indel_alleles()
        rec = R.score()
        text = R.vcf_records("chrS", rec)
        if with_call:
            assert np.array_equal(rows[0], rows[1]) and rows[0][fr.C["unit_positions"]] > 0 and section(rows[0], "dup_base").any()
            assert np.array_equal(R.family_concordance(whole(reads)), rows[0]), "after a score"
        out.append((planes, alleles, {k: v.tobytes() for k, v in rec.items()}, text))
        R.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][2] == out[1][2] and out[0][3] == out[1][3] and len(out[0][3]) > 100


# ------------------------------------------------------------------------------------------------ 7. refusals and the legality window
def test_refusals_launch_nothing_and_leave_out_alone(gpu_lib):
    reads = fc.duplex_planted()
    beg, end = reads["beg"], reads["end"] + 1
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    fn = R._ranges_fn("region_family_concordance", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    sentinel = -7

    def call(ranges, n=None, null_ranges=False, null_out=False, handle=True):
        arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(*q) for q in ranges])
        out = np.full(ROW, sentinel, np.int64)
        rc = fn(R.h if handle else None, None if null_ranges else arr, len(ranges) if n is None else n, None if null_out else out.ctypes.data)
        return rc, out, gpu_lib.last_error()

    ok = [(beg + 5, beg + 100), (beg + 100, beg + 101), (beg + 300, end)]
    rc, out, msg = call(ok)
    assert rc == EINVAL and "family_concordance before set_reads" in msg and (out == sentinel).all()
    rc, out, msg = call(ok, handle=False)
    assert rc == EINVAL and "null region" in msg and (out == sentinel).all()
    R.set_reads(reads)
    rc, out, msg = call(ok)
    assert rc == EINVAL and "family_concordance before accumulate" in msg and (out == sentinel).all()
    R.accumulate()
    want = want_row("duplex_planted", 1, tuple(ok))
    assert section(want, "dup_base").any()
    assert_row(R.family_concordance(ok), want, "after accumulate")
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250), (beg + 10, beg + 50)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50), (beg + 49, beg + 60)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50), (beg + 60, beg + 60)]), "range 1"),
        ("reversed", dict(ranges=[(beg + 50, beg + 10)]), "range 0"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20), (end - 3, end + 1)]), "range 1"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("a negative count", dict(ranges=ok, n=-3), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null_ranges=True), "NULL"),
        ("NULL out", dict(ranges=ok, null_out=True), "NULL"),
    ]
    for what, kw, word in bad_calls:
        rc, out, msg = call(**kw)
        assert rc == EINVAL and word in msg and "family_concordance" in msg, (what, rc, msg)
        assert (out == sentinel).all(), what
        assert_row(R.family_concordance(ok), want, "a valid call after: " + what)
    # the window: a releasing score gives up the planes, which the call does not read; an open score stream does not get in the way
    R.score(release_state=True)
    assert_row(R.family_concordance(ok), want, "after a releasing score")
    R.accumulate()
    gen = R.score_stream(4096)
    next(gen)
    assert_row(R.family_concordance(ok), want, "while a score stream is open")
    gen.close()
    # correct_bq ends the accumulate: refused until the next one
    R.correct_bq()
    rc, out, msg = call(ok)
    assert rc == EINVAL and "before accumulate" in msg and (out == sentinel).all()
    # zero reads: nothing to accumulate, a row of zeros; a reset takes the reads away
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and k != "fam_dflag" else v) for k, v in reads.items()}
    empty["n_reads"] = 0
    R.set_reads(empty)
    rc, out, msg = call(ok)
    assert rc == 0 and not out.any()
    R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    rc, out, msg = call(ok)
    assert rc == EINVAL and "set_reads" in msg and (out == sentinel).all()
    R.close()


# ------------------------------------------------------------------------------------------------ 8. command line
def test_cli_family_concordance_report(tmp_path, gpu_lib):
    """The report of the command line equals the Python chain's rows summed over the BED lines, for one worker and two, for the lines as they
    are and cut into tiles (every position is owned by one tile), and the VCF is that of the run without the option.  (--shard is refused
    with this report as with the error profile: every shard would write a part of the row.)"""
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    total = np.zeros(ROW, np.int64)
    for chrom, b, e, _ in lines:
        b, e = max(0, b), min(e, clen[chrom])
        res = pipeline.call_region(gpu_lib, hb, hf, chrom, b, e, keep_handle=True) if e > b else None
        if res is not None:
            a, z = res["score_range"][0], min(res["score_range"][1], e)
            if z > a:
                total += res["region"].family_concordance([(a, z)])
            res["region"].close()
    assert total[fr.C["unit_positions"]] > 0 and section(total, "base").any() and section(total, "link").any()
    with uio.FamilyConcordance() as s:
        s.add(total)
        s.write(o("want.tsv"))
    want = open(o("want.tsv")).read()
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2")
    vcf_with = run_cli(bam, fa, o("f.vcf.gz"), "-R", bed, "-t", "2", "--family-concordance-out", o("f.tsv"))
    got = open(o("f.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100
    assert run_cli(bam, fa, o("g.vcf.gz"), "-R", bed, "-t", "1", "--family-concordance-out", o("g.tsv")) == vcf_without and open(o("g.tsv")).read() == got
    # tiles: every position is counted once, by the tile that owns it -- but a family is seen as its tile sees it (uvcgpu.h), so the cells may
    # move between bins where a cut goes through a family; what is counted per position does not depend on the cuts
    for extra in (["--tile", "1000", "-t", "2"], ["--tile", "1000", "-t", "1"]):
        run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "--family-concordance-out", o("t%s.tsv" % extra[-1]), *extra)
    assert open(o("t2.tsv")).read() == open(o("t1.tsv")).read()
