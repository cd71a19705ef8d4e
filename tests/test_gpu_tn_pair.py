"""Pair mode of uvc1-mi355x (--normal-bam, the tumor records handed over in memory) against the two-pass flow it replaces (uvcTN.sh:120-127:
tumor pass with --bed-out-fname, normal pass with --bed-in-fname and --tumor-vcf): the tumor VCF, the normal VCF and the region table
are the same, without the two header lines that state the time and the command line of a run."""
import gzip

import pytest

from test_pipeline import _run_cli, make_tn_files
from uvc_amd import pipeline


def text(path):
    return [l for l in gzip.open(path, "rt").read().splitlines() if not l.startswith(("##fileDate=", "##variantCallerCommand="))]


def body(path):
    return [l for l in gzip.open(path, "rt").read().splitlines() if not l.startswith("#")]


@pytest.fixture(scope="module")
def tn(tmp_path_factory):
    d = tmp_path_factory.mktemp("tnpair")
    rd = make_tn_files(d)
    return dict(d=d, tb=str(d / "tumor.bam"), nb=str(d / "normal.bam"), fa=str(d / "tn.fa"), b0=rd["tumor"]["beg"])


def two_pass(tn, tag, shared, tside=(), nside=()):
    d = tn["d"]
    tv, nv, bed = str(d / (tag + "_T.vcf.gz")), str(d / (tag + "_N.vcf.gz")), str(d / (tag + "_T.bed"))
    _run_cli([tn["tb"], "-f", tn["fa"], "-s", "TUM", "-o", tv, "--tn-is-paired", "1", "--bed-out-fname", bed] + shared + list(tside))
    _run_cli([tn["nb"], "-f", tn["fa"], "-s", "NOR", "-o", nv, "--tn-is-paired", "1", "--bed-in-fname", bed, "--tumor-vcf", tv] + shared + list(nside))
    return tv, nv, bed


def pair(tn, tag, shared, tside=(), nside=(), extra=()):
    d = tn["d"]
    tv, nv, bed = str(d / (tag + "_pT.vcf.gz")), str(d / (tag + "_pN.vcf.gz")), str(d / (tag + "_pT.bed"))
    args = [tn["tb"], "--normal-bam", tn["nb"], "-f", tn["fa"], "-s", "TUM,NOR", "-o", nv, "--tumor-output", tv, "--bed-out-fname", bed] + shared + list(extra)
    if tside:
        args += ["--tumor-params"] + list(tside)
    if nside:
        args += ["--normal-params"] + list(nside)
    err = _run_cli(args)
    return tv, nv, bed, err


def assert_same(a, b):
    assert text(a[0]) == text(b[0])                      # tumor VCF
    assert text(a[1]) == text(b[1])                      # normal VCF
    assert open(a[2]).read() == open(b[2]).read()        # region table


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", ["tile", "reference"])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("fmt", [1, 0])
def test_pair_mode_equals_the_two_pass_flow(tn, gpu_lib, cuts, threads, fmt):
    b0 = tn["b0"]
    if cuts == "tile":
        shared = ["--targets", "chrT:%d-%d" % (b0 + 1, b0 + 5000), "--tile", "1000"]
    else:   # the reference's own cuts, small enough that the span is cut into abutting regions (continuing tiles on the normal side)
        shared = ["--mem-per-thread", "2"]
    shared += ["-t", str(threads), "--is-tumor-format-retrieved", str(fmt)]
    tag = "%s_%d_%d" % (cuts, threads, fmt)
    ref = two_pass(tn, tag, shared)
    got = pair(tn, tag, shared, extra=["--timing"])
    assert_same(got, ref)
    err = got[3]
    assert "tumor records handed to the normal tiles in memory" in err and "device memory at the peak" in err, err
    if cuts == "reference":
        bed = [l.split("\t") for l in open(ref[2]).read().splitlines()]
        assert len(bed) >= 3 and any(bed[i][0] == bed[i + 1][0] and bed[i][2] == bed[i + 1][1] for i in range(len(bed) - 1)), bed
    nb = body(got[1])
    assert len(nb) >= 20 and sum(1 for l in nb if "\tSOMATIC" in l) >= 3
    assert text(got[1])[[l.startswith("#CHROM") for l in text(got[1])].index(True)].split("\t")[-2:] == (["NOR", "TUM"] if fmt else ["FORMAT", "NOR"])


@pytest.mark.gpu
def test_side_parameters_reach_their_side_only(tn, gpu_lib):
    b0 = tn["b0"]
    shared = ["--targets", "chrT:%d-%d" % (b0 + 1, b0 + 5000), "--tile", "1000", "-t", "2"]
    tside, nside = ["--fam-thres-highBQ-snv", "27"], ["--tn-syserr-norm-devqual", "-1.0"]
    ref = two_pass(tn, "sides", shared, tside, nside)
    got = pair(tn, "sides", shared, tside, nside)
    assert_same(got, ref)
    plain = pair(tn, "plain", shared)
    assert body(got[1]) != body(plain[1])


@pytest.mark.gpu
def test_pair_shards_join_to_the_one_process_output(tn, gpu_lib):
    """--shard i/2 with 500 bp tiles: a normal tile's tumor fetch range reaches several tumor tiles past the shard edge (the halo)."""
    b0 = tn["b0"]
    shared = ["--targets", "chrT:%d-%d" % (b0 + 1, b0 + 5000), "--tile", "500", "-t", "2"]
    one = pair(tn, "one500", shared)
    assert_same(one, two_pass(tn, "one500", shared))
    tparts, nparts = [], []
    for i in range(2):
        got = pair(tn, "shard%d" % i, shared, extra=["--shard", "%d/2" % i])
        assert "shard %d of 2 takes" % i in got[3] and "more as the halo" in got[3], got[3]
        assert "(tumor; 0 more" not in got[3], got[3]
        tparts.append(got[0]); nparts.append(got[1])
    d = tn["d"]
    tj, nj = str(d / "joined_T.vcf.gz"), str(d / "joined_N.vcf.gz")
    _run_cli(["--concat", tj] + tparts)
    _run_cli(["--concat", nj] + nparts)
    assert text(tj) == text(one[0]) and text(nj) == text(one[1])
    assert all(len(body(p)) >= 1 for p in tparts + nparts)


@pytest.mark.gpu
def test_python_pair_writes_the_command_line_bodies(tn, gpu_lib):
    b0 = tn["b0"]
    d = tn["d"]
    got = pair(tn, "py", ["--targets", "chrT:%d-%d" % (b0 + 1, b0 + 5000), "--tile", "1000", "-t", "2"])
    tv, nv = str(d / "py_T.vcf.gz"), str(d / "py_N.vcf.gz")
    n_t, n_n = pipeline.write_vcf_pair(gpu_lib, tn["tb"], tn["nb"], tn["fa"], "chrT", b0, b0 + 5000, tv, nv, tumor_sample="TUM", normal_sample="NOR", tile=1000)
    assert body(tv) == body(got[0]) and body(nv) == body(got[1])
    assert n_t == len(body(tv)) > 20 and n_n == len(body(nv)) > 20
    assert [l for l in text(nv) if l.startswith("#CHROM")] == [l for l in text(got[1]) if l.startswith("#CHROM")]
