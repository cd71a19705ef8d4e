"""The background error profile of ranges of the accumulated planes (uvcgpu_region_error_profile, Region.error_profile) and the report built
from it (uvc1-mi355x --error-profile-out).  Every number is an integer and is compared for equality:
  * all 5 x 712 values of the HIP library against the numpy restatement of the definitions (tests/errprofile_restatement.py) over the ORACLE's
    fetched planes (FRAG / FAM / DUPLEX) and the reference string, for the ten range lists of the coverage test and four gates;
  * assertions on the oracle's own profile that an unwired level or an inert gate could not meet;
  * the refusals of the ABI, which launch nothing, leave `out` alone and leave the handle usable;
  * the report of the command line against the Python chain (uvc_amd.pipeline regions + Region.error_profile), across --tile, -t,
    --merge-regions, --score-mem-mb and together with --coverage-out."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import errprofile_restatement as er
from test_gpu_coverage import panel, range_lists, run_cli
from test_gpu_parity import CASES
from util import run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
E = _ffi.ENUMS
NLEVEL, ROW = E["UVC_NERRLEVEL"], E["UVC_ERR_ROW"]
EINVAL = E["UVCGPU_EINVAL"]
GATES = [(20, 50), (1, 1000), (1, 0), (500, 50)]
LEVEL = {n: i for i, n in enumerate(region.ERROR_LEVELS)}


def n_reference(reads):
    """The same reads over a reference string with a 70-base stretch of N and a few single Ns (both ends of the string among them)."""
    s = list(reads["refseq"])
    for a in list(range(1000, 1070)) + [0, 1, len(s) - 1, 2500, 2502, 4000]:
        s[a] = "N"
    out = dict(reads)
    out["refseq"] = "".join(s)
    return out


INPUTS = {
    "plain_5kb_300x": lambda: synth.generate_region(**CASES["config2shape_5kb_300x"]),
    "umi_2kb_400x": lambda: synth.generate_region(**CASES["umi_duplex_2kb_400x"]),
    "duplex_1kb_2000x": lambda: synth.generate_region(**CASES["config4shape_1kb_2000x_duplex"]),
    "plain_5kb_300x_N_reference": lambda: n_reference(synth.generate_region(**CASES["config2shape_5kb_300x"])),
}


def non_reference(p):
    """The bins of a profile with the reference-symbol bins (BASE: the context's middle base; LINK: M) set to 0 -> (non-reference, reference)."""
    ref = np.zeros(ROW, bool)
    for ctx in range(er.NCTX):
        ref[er.BASE_BINS + ctx * er.NBASE + ((ctx >> 2) & 3)] = True
        ref[er.LINK_BINS + ctx * er.NLINK] = True
    bins = np.arange(ROW) < er.COUNTERS
    return np.where(bins & ~ref, p, 0), np.where(ref, p, 0)


@pytest.mark.parametrize("name", list(INPUTS))
def test_rows_equal_the_numpy_restatement_over_the_oracles_planes(name, oracle_lib, gpu_lib):
    reads = INPUTS[name]()
    Ro = run_region(oracle_lib, reads)
    cells = er.level_cells(Ro.fetch)
    Ro.close()
    Rg = run_region(gpu_lib, reads)
    beg, npos = Rg.beg, Rg.npos
    assert cells.shape == (NLEVEL, _ffi.NSYM, npos) and npos == reads["end"] - reads["beg"] + 1
    whole = [(beg, beg + npos)]
    rest = {g: er.Restatement(cells, reads["refseq"], beg, *g) for g in GATES}
    # ---- the oracle's own profile: every level is wired and every gate bites (else the comparison below could pass on zeros)
    want = {g: rest[g].profile(whole) for g in GATES}
    p = want[(20, 50)]
    print(name, "counters at bDP with (20, 50):", dict(zip(er.COUNTER_NAMES, p[0, er.COUNTERS:].tolist())))
    if name.startswith("plain_5kb"):
        assert p[LEVEL["bDP"], er.C["BASE_high_alt"]] >= 1 and any(v[1] == "snv" and v[3] == 0.5 for v in reads["variants"])
        assert (non_reference(p)[0][LEVEL["bDP"], er.BASE_BINS:er.LINK_BINS] > 0).sum() >= 6
        assert p[LEVEL["bDP"], er.C["LINK_counted"]] > 0
    if name.startswith("umi"):
        assert (p[LEVEL["cDP2"], :er.COUNTERS] > 0).any(), "no family large enough for a consensus: cDP2 cannot be told from an unwired plane"
    if name.startswith("duplex"):
        assert (p[LEVEL["dDP1"], :er.COUNTERS] > 0).any(), "no duplex family: dDP1 cannot be told from an unwired plane"
    if name.endswith("N_reference"):
        assert p[0, er.C["no_context"]] >= 72 and (p[:, er.C["no_context"]] == p[0, er.C["no_context"]]).all()
    nonref, ref = non_reference(want[(1, 0)])
    assert not nonref.any() and ref[LEVEL["bDP"]].any() and ref[LEVEL["cDP1"]].any()
    assert not want[(1, 1000)][:, [er.C["BASE_high_alt"], er.C["LINK_high_alt"]]].any()
    # ---- the HIP library against it: ten range lists x four gates, all 5 x 712 values
    rng = np.random.default_rng(17)
    n_lists = 0
    for what, ranges in range_lists(rng, beg, npos):
        for g in GATES:
            got = Rg.error_profile(ranges, *g)
            w = rest[g].profile(ranges)
            assert got.shape == (NLEVEL, ROW) and got.dtype == np.int64
            bad = np.argwhere(got != w)
            assert len(bad) == 0, (name, what, g, [(tuple(i), int(got[tuple(i)]), int(w[tuple(i)])) for i in bad[:6]])
        n_lists += 1
        if len(ranges) >= 2:   # profiles of disjoint position sets add
            h = len(ranges) // 2
            assert np.array_equal(Rg.error_profile(ranges[:h]) + Rg.error_profile(ranges[h:]), Rg.error_profile(ranges)), what
    assert n_lists == 10
    # the same bits from call to call
    a, b = Rg.error_profile(whole, 20, 50), Rg.error_profile(whole, 20, 50)
    assert np.array_equal(a, b) and np.array_equal(a, want[(20, 50)]) and not a[:, er.COUNTERS + E["UVC_ERRC_reserved"]].any()
    Rg.close()


def test_sharded_profile_equals_the_restatement(oracle_lib, gpu_lib):
    """From 128 blocks (32 768 compact positions) on the blocks add into copies of the profile and the shared fold (uvc_launch_sum_fold, with
    the profile's 3 560 words as its run-time row length) sums them: 40 000 positions in one range are 157 blocks and 2 copies."""
    reads = synth.generate_region(region_len=40000, depth=8, seed=21)
    Ro = run_region(oracle_lib, reads)
    cells = er.level_cells(Ro.fetch)
    Ro.close()
    Rg = run_region(gpu_lib, reads)
    beg, npos = Rg.beg, Rg.npos
    blocks = -(-npos // 256)
    assert 128 <= blocks < 192 and blocks // 64 == 2, (npos, blocks)   # err_geometry: one step per block, shards = blocks / 64
    whole = [(beg, beg + npos)]
    for g in [(1, 1000), (5, 50)]:
        want = er.Restatement(cells, reads["refseq"], beg, *g).profile(whole)
        got = Rg.error_profile(whole, *g)
        assert want[LEVEL["bDP"], er.BASE_BINS:er.LINK_BINS].any() and (g != (1, 1000) or want[LEVEL["bDP"], er.C["BASE_counted"]] > 20000)   # (the oracle's profile is not zeros)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (g, [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])
    Rg.close()


def test_argument_checks(oracle_lib, gpu_lib):
    reads = synth.generate_region(**CASES["tiny_600bp_5x"])
    fn = gpu_lib.dll.uvcgpu_region_error_profile
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, end = R.beg, R.beg + R.npos
    sentinel = -123456789

    def call(ranges, gate=(1, 50), n=None, null_ranges=False, null_req=False, null_out=False):
        arr = (_ffi.UvcCoverageRange * max(len(ranges), 1))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])
        req = _ffi.UvcErrorProfileRequest(*gate)
        out = np.full((NLEVEL, ROW), sentinel, np.int64)
        rc = fn(R.h, None if null_ranges else arr, len(ranges) if n is None else n, None if null_req else C.byref(req), None if null_out else out.ctypes.data)
        return rc, out, gpu_lib.last_error()

    ok = [(beg + 5, beg + 100), (beg + 100, beg + 101), (beg + 300, end)]
    # before set_reads / accumulate: refused with a message, not garbage
    rc, out, msg = call(ok)
    assert rc == EINVAL and "accumulate" in msg and (out == sentinel).all()
    R.set_reads(reads)
    rc, out, msg = call(ok)
    assert rc == EINVAL and "accumulate" in msg and (out == sentinel).all()
    R.accumulate()
    Ro = run_region(oracle_lib, reads)
    want = er.Restatement(er.level_cells(Ro.fetch), reads["refseq"], beg, 1, 50).profile(ok)
    Ro.close()
    assert want[:, :er.COUNTERS].any() and np.array_equal(R.error_profile(ok, 1, 50), want)
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250), (beg + 10, beg + 50)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50), (beg + 49, beg + 60)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50), (beg + 60, beg + 60)]), "range 1"),
        ("reversed", dict(ranges=[(beg + 50, beg + 10)]), "range 0"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20), (end - 3, end + 1)]), "range 1"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null_ranges=True), "NULL"),
        ("NULL request", dict(ranges=ok, null_req=True), "NULL"),
        ("NULL out", dict(ranges=ok, null_out=True), "NULL"),
        ("min_depth 0", dict(ranges=ok, gate=(0, 50)), "min_depth"),
        ("max_alt_permille -1", dict(ranges=ok, gate=(1, -1)), "max_alt_permille"),
        ("max_alt_permille 1001", dict(ranges=ok, gate=(1, 1001)), "max_alt_permille"),
    ]
    for what, kw, word in bad_calls:
        rc, out, msg = call(**kw)
        assert rc == EINVAL and word in msg, (what, rc, msg)
        assert (out == sentinel).all(), what
        # the handle is as usable as before: the next valid call gives the right profile
        assert np.array_equal(R.error_profile(ok, 1, 50), want), what
    # a plain score keeps the planes: the profile still answers; a releasing score comes after it, and then it is refused
    R.score()
    assert np.array_equal(R.error_profile(ok, 1, 50), want)
    R.score(release_state=True)
    rc, out, msg = call(ok)
    assert rc == EINVAL and "release" in msg and (out == sentinel).all()
    # the next accumulate brings the planes back
    R.set_reads(reads)
    R.accumulate()
    assert np.array_equal(R.error_profile(ok, 1, 50), want)
    # while a score stream is open the planes may go at any moment: refused; after its end the handle answers again
    gen = R.score_stream(4096)
    next(gen)
    rc, out, msg = call(ok)
    assert rc == EINVAL and "stream" in msg and (out == sentinel).all()
    gen.close()
    assert np.array_equal(R.error_profile(ok, 1, 50), want)
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def chain_profile(gpu_lib, bam, fa, chrom, beg, end, gate):
    """The profile of the positions that one region [beg, end) of the Python chain (uvc_amd.pipeline.call_region) owns."""
    res = pipeline.call_region(gpu_lib, bam, fa, chrom, beg, end, keep_handle=True) if end > beg else None
    p = np.zeros((NLEVEL, ROW), np.int64)
    if res is not None:
        a, b = res["score_range"][0], min(res["score_range"][1], end)
        if b > a:
            p = res["region"].error_profile([(a, b)], *gate)
        res["region"].close()
    return p


def test_cli_error_profile_report(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    gate = (10, 100)
    opts = ["--error-profile-min-depth", str(gate[0]), "--error-profile-max-alt-permille", str(gate[1])]
    # the report equals the Python chain: every BED line its own region, the profiles of the owned positions summed
    total = np.zeros((NLEVEL, ROW), np.int64)
    for chrom, b, e, _ in lines:
        total += chain_profile(gpu_lib, hb, hf, chrom, max(0, b), min(e, clen[chrom]), gate)
    want = er.report_text(region.ERROR_LEVELS, total, *gate)
    assert total[LEVEL["bDP"], er.C["BASE_counted"]] > 1000 and non_reference(total)[0][LEVEL["bDP"]].any()
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2")
    vcf_with = run_cli(bam, fa, o("e.vcf.gz"), "-R", bed, "-t", "2", "--error-profile-out", o("e.tsv"), *opts)
    got = open(o("e.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100
    # the same bytes however the lines are cut, however many workers run and however the tiles are scored
    for extra in (["--tile", "1000", "-t", "1"], ["--tile", "7000", "-t", "4"], ["-t", "1"], ["-t", "4"], ["-t", "2", "--score-mem-mb", "16"]):
        vcf = run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "--error-profile-out", o("t.tsv"), *opts, *extra)
        assert open(o("t.tsv")).read() == got, extra
        assert vcf == (run_cli(bam, fa, o("u.vcf.gz"), "-R", bed, *extra) if "--tile" in extra else vcf_without), extra   # the same tiling without the option
    # merged regions see the reads of the gaps between their lines: the same bytes across -t, and the VCF of the run without it
    vcf_m = run_cli(bam, fa, o("m.vcf.gz"), "-R", bed, "-t", "1", "--merge-regions", "2000")
    for threads in ("1", "4"):
        vcf = run_cli(bam, fa, o("m%s.vcf.gz" % threads), "-R", bed, "-t", threads, "--merge-regions", "2000", "--error-profile-out", o("m%s.tsv" % threads), *opts)
        assert vcf == vcf_m
    assert open(o("m1.tsv")).read() == open(o("m4.tsv")).read() and open(o("m1.tsv")).read().startswith("##error_profile_min_depth=10\n")
    # with --coverage-out as well: both reports and the VCF are those of the runs with one of them; .gz is the same text, block-gzipped
    run_cli(bam, fa, o("c.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("c.tsv"))
    vcf_b = run_cli(bam, fa, o("b.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("b.cov.tsv"), "--error-profile-out", o("b.tsv.gz"), *opts)
    assert vcf_b == vcf_without and open(o("b.cov.tsv")).read() == open(o("c.tsv")).read()
    assert gzip.open(o("b.tsv.gz"), "rt").read() == got and open(o("b.tsv.gz"), "rb").read()[12:16] == b"BC\x02\x00"
    # the defaults are 20 and 50
    run_cli(bam, fa, o("d.vcf.gz"), "-R", bed, "-t", "2", "--error-profile-out", o("d.tsv"))
    assert open(o("d.tsv")).read().startswith("##error_profile_min_depth=20\n##error_profile_max_alt_permille=50\n")
