"""The read profile of the HIP library (uvcgpu_region_read_profile, Region.read_profile) and the report built from it (uvc1-mi355x
--read-profile-out).  Every number is an integer and is compared for equality:
  * all 5 712 words against the restatement of the definitions (tests/readprofile_restatement.py) for the ten range lists of the coverage
    test and five gates, on four synthetic inputs -- as generated and with random qualities 0..79 -- on the hand-made reads of the CPU test
    and on one synthetic 20 kb read with forty InDels (the chunked CIGAR path);
  * assertions on the restatement's own row that an unwired section could not meet;
  * the corrected qualities after correct_bq, the legality window and the refusals of the ABI;
  * the report of the command line against the Python chain, across --tile, -t, --score-mem-mb and --merge-regions, with the VCF and the
    other four reports unchanged."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import readprofile_restatement as rr
import test_readprofile_cpu as cpu
from test_bq_correction import expected_quals, make_reads
from test_gpu_coverage import panel, range_lists, run_cli
from test_gpu_device_reads import DeviceColumns
from test_gpu_parity import CASES
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
EINVAL = _ffi.ENUMS["UVCGPU_EINVAL"]
ROW = _ffi.ENUMS["UVC_READPROF_ROW"]
GATES = [(0, 20, 50), (0, 1, 1000), (0, 1, 0), (30, 20, 50), (0, 500, 50)]
# The parity cases, with the variant tracks of the generator brought into reach where the case as it stands gets none: it plants nothing
# within 500 bp of either end, so the 800 bp and 600 bp cases hold no variant at all, the 2 kb case one SNV and one deletion, and the 5 kb
# case (one InDel per 5 000 bp) no insertion.  Region length, depth, seed and UMI mode -- what the cases are about -- stay.
INPUTS = {
    "tiny_600bp_5x": dict(CASES["tiny_600bp_5x"], variant_inset=100, snv_every=150, clip_frac=0.3),
    "config2shape_5kb_300x": dict(CASES["config2shape_5kb_300x"], indel_every=700),
    "umi_duplex_2kb_400x": dict(CASES["umi_duplex_2kb_400x"], variant_inset=100, snv_every=400, indel_every=150),
    "deep_nonumi_800bp_3000x": dict(CASES["deep_nonumi_800bp_3000x"], variant_inset=100, snv_every=150, indel_every=50),
}
# What the 20 reads of tiny_600bp_5x cannot meet, whatever the options: no position reaches the depth 20 of the gate (0, 20, 50), so none is
# high_alt under it; and the generator's InDel track begins 400 bp behind its SNV track, which a 600 bp region has no room for, so CYC
# kinds 2 (ins) and 3 (del) stay empty.  Every other assertion holds on it as on the other three.
TINY_CANNOT = "tiny_600bp_5x"


def open_region(lib, reads):
    R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    return R


def diff(got, want):
    return [(int(i), int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:8]]


@pytest.mark.parametrize("quals", ["as_generated", "random_0_79"])
@pytest.mark.parametrize("name", list(INPUTS))
def test_rows_equal_the_restatement(name, quals, gpu_lib):
    reads = synth.generate_region(**INPUTS[name])
    if quals == "random_0_79":
        reads = dict(reads, quals=np.random.default_rng(3).integers(0, 80, len(reads["quals"])).astype(np.uint8))
    rs = rr.Restatement(reads)
    R = open_region(gpu_lib, reads)
    beg, npos = R.beg, R.npos
    whole = [(beg, beg + npos)]
    # ---- the restatement's own row: every section is wired and every gate bites
    want = {g: rs.row(whole, *g) for g in GATES}
    q, cyc, sub, cnt = rr.sections(want[(0, 1, 1000)])
    print(name, quals, dict(zip(rr.COUNTER_NAMES, rr.sections(want[(0, 20, 50)])[3].tolist())), "CYC kinds", cyc.sum((0, 1)).tolist())
    assert (q.sum((1, 2)) > 0).all(), "a read class is missing"
    assert (sub * (1 - np.eye(4, dtype=np.int64)) > 0).sum() >= 6
    assert len(np.unique(reads["mapq"])) > 1 and want[(30, 20, 50)][rr.C["bases_low_mapq"]] > 0
    assert want[(0, 1, 1000)][rr.C["positions_high_alt"]] == 0
    kinds = cyc.sum((0, 1))
    assert kinds[1] > 0 and kinds[4] > 0, "CYC kinds 1 (mismatch) and 4 (clip)"
    if name != TINY_CANNOT:
        assert kinds[2] > 0 and kinds[3] > 0, "CYC kinds 2 (ins) and 3 (del)"
        assert want[(0, 20, 50)][rr.C["positions_high_alt"]] >= 1
    if quals == "random_0_79":
        assert q[:, 63].sum() > q[:, 62].sum() * 4 > 0, "the last quality bin takes 63..79"
    assert not want[(0, 1, 0)][rr.Q_BINS + 1:rr.CYC_BINS:2].any()   # max_alt_permille 0: a position with a mismatch is not clean
    # ---- the HIP library: ten range lists x five gates, all 5 712 words
    rng = np.random.default_rng(17)
    n_lists = 0
    for what, ranges in range_lists(rng, beg, npos):
        for g in GATES:
            got = R.read_profile(ranges, *g)
            assert got.shape == (ROW,) and got.dtype == np.int64
            w = rs.row(ranges, *g)
            assert np.array_equal(got, w), (name, what, g, diff(got, w))
            rr.check_identities(got, sum(e - b for b, e in ranges))
        n_lists += 1
        if len(ranges) >= 2:   # rows of disjoint position sets add
            h = len(ranges) // 2
            assert np.array_equal(R.read_profile(ranges[:h]) + R.read_profile(ranges[h:]), R.read_profile(ranges)), what
    assert n_lists == 10
    a, b = R.read_profile(whole), R.read_profile(whole)   # the same bits from call to call
    assert np.array_equal(a, b) and np.array_equal(a, want[(0, 20, 50)]) and not a[rr.COUNTERS + 10:].any()
    R.close()


def hand_made_sets():
    A = cpu
    b0 = [0, 0] + [A.REF[10], A.REF[11], (A.REF[12] + 1) % 4, A.REF[13]] + [3, 3, 3]
    b1 = [2] + [A.REF[50], A.REF[51], A.REF[52]]
    yield A.hand_made([(10, 0x0, [(A.S, 2), (A.M, 4), (A.S, 3)], b0, [30, 30, 31, 32, 33, 34, 2, 2, 2]), (50, 0x90, [(A.H, 2), (A.S, 1), (A.M, 3), (A.H, 2)], b1, [70, 40, 41, 63])])
    aligned = [100, 101, 102, 105, 106, 112, 113]
    b = [1, 2, 2] + [A.REF[p] for p in aligned[:5]] + [A.REF[112], 0, A.REF[113]]
    yield A.hand_made([(100, 0x80, [(A.S, 1), (A.I, 2), (A.M, 3), (A.D, 2), (A.M, 2), (A.N, 5), (A.M, 1), (A.I, 1), (A.M, 1)], b, [20] * 11)])
    same = [A.REF[200], A.REF[201], A.REF[202], A.REF[203]]
    yield A.hand_made([(200, 0, [(A.M, 4)], same, [30] * 4), (200, 0, [(A.M, 4)], [same[0], 4, (same[2] + 2) % 4, same[3]], [10, 11, 12, 13]), (200, 0x10, [(A.M, 4)], same, [40] * 4)],
                      mapq=[60, 60, 5], ref_edit={203: "N"})
    b = [A.REF[k] for k in range(300)]
    yield A.hand_made([(0, 0, [(A.M, 300)], b, [25] * 300), (0, 0x10, [(A.M, 300)], b, [25] * 300)])
    # a deletion in front of the first base and one behind the last; reads at both ends of the region, a clip anchored at the first position
    yield A.hand_made([(5, 0, [(A.D, 2), (A.M, 10), (A.D, 3)], [A.REF[7 + k] for k in range(10)], [33] * 10),
                       (0, 0x10, [(A.S, 3), (A.M, 12)], [1] * 15, [35] * 15), (A.REF_LEN - 11, 0x80, [(A.M, 10), (A.I, 2)], [2] * 12, [36] * 12)])


def test_hand_made_reads(gpu_lib):
    n = 0
    for reads in hand_made_sets():
        rs, R = rr.Restatement(reads), open_region(gpu_lib, reads)
        beg, npos = R.beg, R.npos
        for ranges in ([(beg, beg + npos)], [(beg + 104, beg + 113)], [(beg, beg + 1), (beg + 100, beg + 101), (beg + 201, beg + 204), (beg + npos - 1, beg + npos)]):
            for g in ((0, 1, 1000), (10, 2, 500), (10, 1, 499), (0, 20, 50)):
                got, w = R.read_profile(ranges, *g), rs.row(ranges, *g)
                assert np.array_equal(got, w), (n, ranges, g, diff(got, w))
        R.close()
        n += 1
    assert n == 5


def long_read(seed=4):
    """One alignment of about 20 000 query bases with some forty I / D ops (and a leading clip): 83 CIGAR ops, 300-odd chunks."""
    rng = np.random.default_rng(seed)
    ref_len = 21000
    refseq = rng.integers(0, 4, ref_len)
    cigar, bases, p = [(cpu.S, 37)], list(rng.integers(0, 4, 37)), 50
    for k in range(41):
        ln = int(rng.integers(300, 650))
        seg = refseq[p:p + ln].copy()
        err = rng.random(ln) < 0.01
        seg[err] = (seg[err] + 1 + rng.integers(0, 3, int(err.sum()))) % 4
        cigar.append((cpu.M, ln)); bases += list(seg); p += ln
        if k < 40:
            g = int(rng.integers(1, 70))
            if k % 2:
                cigar.append((cpu.I, g)); bases += list(rng.integers(0, 4, g))
            else:
                cigar.append((cpu.D, g)); p += g
    assert p < ref_len - 10
    quals = rng.integers(2, 42, len(bases))
    r = make_reads([(50, 0x10, cigar, bases, list(quals)), (60, 0x0, [(cpu.M, 120)], list(refseq[60:180]), [30] * 120)], beg=2_000_000, ref_len=ref_len)
    r["refseq"] = "".join("ACGT"[i] for i in refseq)
    return r


def test_one_long_read_with_forty_indels(gpu_lib):
    reads = long_read()
    assert reads["l_qseq"][0] > 19000 and reads["n_cigar"][0] == 82
    rs, R = rr.Restatement(reads), open_region(gpu_lib, reads)
    beg, npos = R.beg, R.npos
    w = rs.row([(beg, beg + npos)], 0, 1, 1000)
    cyc = rr.sections(w)[1]
    assert (cyc[1].sum(0) > 0).all() and cyc[1, 255].sum() > 18000 and cyc[1, :255, 0].sum() > 100
    for what, ranges in range_lists(np.random.default_rng(5), beg, npos):
        for g in ((0, 1, 1000), (0, 1, 50), (0, 2, 1000)):
            got, w = R.read_profile(ranges, *g), rs.row(ranges, *g)
            assert np.array_equal(got, w), (what, g, diff(got, w))
    R.close()


def test_corrected_qualities_and_the_legality_window(gpu_lib):
    reads = synth.generate_region(seed=33, region_len=3000, depth=80, clip_frac=0.3, indel_every=400)
    p = region.default_params(gpu_lib)
    p.assay_sequencing_BQ_max, p.assay_sequencing_BQ_inc = 37, 2
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, npos = R.beg, R.npos
    ok = [(beg + 5, beg + 100), (beg + 100, beg + 101), (beg + 300, beg + npos)]
    fn = gpu_lib.dll.uvcgpu_region_read_profile
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    sentinel = -123456789

    def call(ranges, gate=(0, 20, 50), n=None, null_ranges=False, null_req=False, null_out=False):
        arr = (_ffi.UvcCoverageRange * max(len(ranges), 1))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])
        req = _ffi.UvcReadProfileRequest(*gate)
        out = np.full(ROW, sentinel, np.int64)
        rc = fn(R.h, None if null_ranges else arr, len(ranges) if n is None else n, None if null_req else C.byref(req), None if null_out else out.ctypes.data)
        return rc, out, gpu_lib.last_error()

    rc, out, msg = call(ok)   # before set_reads
    assert rc == EINVAL and "set_reads" in msg and "has no reads yet" in msg and "family" not in msg and (out == sentinel).all()
    R.set_reads(reads)
    before = rr.Restatement(reads)
    want = before.row(ok)
    assert want[:rr.COUNTERS].any() and np.array_equal(R.read_profile(ok), want)
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250), (beg + 10, beg + 50)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50), (beg + 49, beg + 60)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50), (beg + 60, beg + 60)]), "range 1"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20), (beg + npos - 3, beg + npos + 1)]), "range 1"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null_ranges=True), "NULL"),
        ("NULL request", dict(ranges=ok, null_req=True), "NULL"),
        ("NULL out", dict(ranges=ok, null_out=True), "NULL"),
        ("min_mapq -1", dict(ranges=ok, gate=(-1, 20, 50)), "min_mapq"),
        ("min_mapq 256", dict(ranges=ok, gate=(256, 20, 50)), "min_mapq"),
        ("min_depth 0", dict(ranges=ok, gate=(0, 0, 50)), "min_depth"),
        ("max_alt_permille -1", dict(ranges=ok, gate=(0, 1, -1)), "max_alt_permille"),
        ("max_alt_permille 1001", dict(ranges=ok, gate=(0, 1, 1001)), "max_alt_permille"),
    ]
    for what, kw, word in bad_calls:
        rc, out, msg = call(**kw)
        assert rc == EINVAL and word in msg and "read_profile" in msg, (what, rc, msg)
        assert (out == sentinel).all(), what
        assert np.array_equal(R.read_profile(ok), want), what   # the handle is as usable as before
    # the corrected qualities: the row of the restatement over them, and not the row before
    R.correct_bq()
    after = rr.Restatement(reads, quals=expected_quals(reads, 37, 2))
    got = R.read_profile(ok)
    assert np.array_equal(got, after.row(ok)), diff(got, after.row(ok))
    assert not np.array_equal(got, want) and got[rr.C["bases_clean"]] == want[rr.C["bases_clean"]]
    want = after.row(ok)
    # legal after accumulate, after a plain and a releasing score, while a score stream is open
    R.accumulate()
    assert np.array_equal(R.read_profile(ok), want)
    R.score()
    assert np.array_equal(R.read_profile(ok), want)
    R.score(release_state=True)
    assert np.array_equal(R.read_profile(ok), want)
    R.accumulate()
    gen = R.score_stream(4096)
    next(gen)
    assert np.array_equal(R.read_profile(ok), want)
    gen.close()
    R.close()
    # after a reset: refused until the next set_reads; zero reads: the positions_* words alone
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    assert np.array_equal(R.read_profile(ok), before.row(ok))
    R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    rc, out, msg = call_on(fn, R, ok)
    assert rc == EINVAL and "set_reads" in gpu_lib.last_error() and (out == sentinel).all()
    none = dict(reads, n_reads=0, n_fams=0)
    for k in ("pos", "mpos", "isize", "flag", "mapq", "nm", "l_qseq", "seq_off", "cigar_off", "n_cigar", "frag_id", "fam_id", "fam_strand", "bases", "quals", "cigars", "fam_dflag"):
        none[k] = reads[k][:0]
    R.set_reads(none)
    got = R.read_profile(ok)
    n_pos = sum(e - b for b, e in ok)
    assert got[rr.C["positions_low_depth"]] == n_pos - 1 and got[rr.C["positions_no_ref"]] == 1 and got.sum() == n_pos
    assert np.array_equal(got, rr.Restatement(none).row(ok))
    R.close()


def call_on(fn, R, ranges, gate=(0, 20, 50)):
    arr = (_ffi.UvcCoverageRange * len(ranges))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])
    req = _ffi.UvcReadProfileRequest(*gate)
    out = np.full(ROW, -123456789, np.int64)
    return fn(R.h, arr, len(ranges), C.byref(req), out.ctypes.data), out, None


def test_set_reads_device_path(gpu_lib):
    reads = synth.generate_region(**CASES["umi_duplex_2kb_400x"])
    cols = DeviceColumns(reads)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads_device((cols.soa, cols))
    rs = rr.Restatement(reads)
    for ranges in ([(R.beg, R.beg + R.npos)], [(R.beg + 64, R.beg + 127), (R.beg + 500, R.beg + 1500)]):
        got, w = R.read_profile(ranges), rs.row(ranges)
        assert np.array_equal(got, w), diff(got, w)
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def chain_row(gpu_lib, bam, fa, chrom, beg, end, gate):
    """The row of the positions that one region [beg, end) of the Python chain (uvc_amd.pipeline.call_region) owns, with the BAM's own
    qualities: the chain without its BQ correction, which moves neither the region nor the positions the tile owns."""
    res = pipeline.call_region(gpu_lib, bam, fa, chrom, beg, end, keep_handle=True, correct_bq=False) if end > beg else None
    row = np.zeros(ROW, np.int64)
    if res is not None:
        a, b = res["score_range"][0], min(res["score_range"][1], end)
        if b > a:
            row = res["region"].read_profile([(a, b)], *gate)
        res["region"].close()
    return row


def test_cli_read_profile_report(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    gate = (10, 10, 100)
    opts = ["--read-profile-min-mapq", "10", "--read-profile-min-depth", "10", "--read-profile-max-alt-permille", "100"]
    total = np.zeros(ROW, np.int64)
    for chrom, b, e, _ in lines:   # every BED line its own region, the rows of the owned positions summed
        total += chain_row(gpu_lib, hb, hf, chrom, max(0, b), min(e, clen[chrom]), gate)
    want = rr.report_text(total, *gate)
    assert total[rr.C["bases_clean"]] > 10000 and (rr.sections(total)[1].sum((0, 1)) > 0).all()
    others = ["--coverage-out", o("c.tsv"), "--error-profile-out", o("e.tsv"), "--family-stats-out", o("f.tsv"), "--callable-out", o("k.bed")]
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2", *others)
    reports = [open(o(n)).read() for n in ("c.tsv", "e.tsv", "f.tsv", "k.bed")]
    vcf_with = run_cli(bam, fa, o("r.vcf.gz"), "-R", bed, "-t", "2", *others, "--read-profile-out", o("r.tsv"), *opts)
    got = open(o("r.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100                  # the VCF and the other four reports do not see the option
    assert [open(o(n)).read() for n in ("c.tsv", "e.tsv", "f.tsv", "k.bed")] == reports
    # the same bytes however the lines are cut, however many workers run and however the tiles are scored
    for extra in (["--tile", "1000", "-t", "1"], ["--tile", "7000", "-t", "4"], ["-t", "1"], ["-t", "4"], ["-t", "2", "--score-mem-mb", "16"]):
        run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "--read-profile-out", o("t.tsv"), *opts, *extra)
        assert open(o("t.tsv")).read() == got, extra
    # merged regions see the reads of the gaps between their lines: compared with itself across -t; .gz is the same text, block-gzipped
    for threads in ("1", "4"):
        run_cli(bam, fa, o("m%s.vcf.gz" % threads), "-R", bed, "-t", threads, "--merge-regions", "2000", "--read-profile-out", o("m%s.tsv.gz" % threads), *opts)
    m1 = gzip.open(o("m1.tsv.gz"), "rt").read()
    assert m1 == gzip.open(o("m4.tsv.gz"), "rt").read() and m1.startswith("##read_profile_min_mapq=10\n") and open(o("m1.tsv.gz"), "rb").read()[12:16] == b"BC\x02\x00"
    run_cli(bam, fa, o("d.vcf.gz"), "-R", bed, "-t", "2", "--read-profile-out", o("d.tsv"))   # the defaults are 0, 20 and 50
    assert open(o("d.tsv")).read().startswith("##read_profile_min_mapq=0\n##read_profile_min_depth=20\n##read_profile_max_alt_permille=50\n")
