"""Family statistics of ranges from the device family units (uvcgpu_region_family_stats, Region.family_stats) and the per-target report built
from them (uvc1-mi355x --family-stats-out).  Every number is an integer and is compared for equality with tests/famstats_restatement.py,
which restates the definitions from the read columns alone:
  * hand-built reads that hold every family shape the row distinguishes (single-strand, both strands, around the 16 cap of `strands` and the
    64 cap of `size`, fragments of two alignments, one 3000-fragment pile, thousands of small families), against ranges placed on the edges
    of the overlap, CONTINUES and prev_end rules;
  * the suite's synthetic inputs against the ten range lists of test_gpu_coverage;
  * the refusals of the ABI, which launch nothing, leave `out` alone and leave the handle usable, and the states the call stays legal in;
  * the report of the command line against the Python chain (uvc_amd.pipeline regions + Region.family_stats + the restatement's text)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import famstats_restatement as fr
from test_gpu_coverage import panel, range_lists, run_cli
from test_gpu_device_reads import DeviceColumns
from test_gpu_parity import CASES
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
E = _ffi.ENUMS
ROW, EINVAL = E["UVC_FAMSTAT_ROW"], E["UVCGPU_EINVAL"]
B, LEN = 5_000_000, 3000   # the hand-built region: [B, B + LEN)


# ------------------------------------------------------------------------------------------------ hand-built reads
def hand_built():
    """-> (reads, named): reads in the dict form of synth.generate_region; named[label] = fam_id of a family placed for a range situation.
    A family is (a, b, dflag, x, read length, two_aln): a / b fragments on strand 0 / 1, every alignment at region offset x (+ 0..2 for the
    large ones), and with two_aln the first fragment of strand 0 has two alignments."""
    rng = np.random.default_rng(41)
    fams, named = [], {}

    def fam(a, b, dflag, x, L=40, two_aln=False, label=None, jitter=0):
        if label:
            named[label] = len(fams)
        fams.append((a, b, dflag, x, L, two_aln, jitter))
    # the range situations live in [0, 600): nothing else begins there
    fam(1, 0, 0, 200, label="lo_is_pos_end")        # [200, 240) against range [100, 200)
    fam(1, 0, 1, 60, label="hi_is_pos_beg")         # [60, 100)
    fam(1, 0, 0, 50, L=60, label="before_prev_end")  # [50, 110): overlaps [100, 200), begins in front of its prev_end 60
    fam(2, 0, 1, 320, label="straddles_joint")      # [320, 360) over the joint 340 of [300, 340) | [340, 400) CONTINUES
    fam(1, 1, 3, 350, label="inside_continuing")    # [350, 390)
    fam(1, 0, 4, 420, label="between")              # [420, 460): between [340, 400) and [500, 510)
    fam(1, 0, 0, 495, L=60, label="spans_three")    # [495, 555) over [500, 510) [520, 530) [540, 550)
    # family sizes around the caps, single and both strands, a fragment of two alignments beside one of one, the pile
    for a, b in ((1, 0), (0, 1), (1, 1), (15, 1), (16, 16), (17, 0), (31, 32), (32, 32), (40, 30)):
        fam(a, b, 3 if (a and b) else 1, int(rng.integers(700, 2900)), jitter=3)
    fam(2, 0, 1, 1000, two_aln=True, label="two_alignments")
    fam(3000, 0, 4, 1500, jitter=3, label="pile")
    for _ in range(6200):
        d = int(rng.choice([0, 1, 3, 4]))
        fam(int(rng.integers(1, 4)), int(rng.integers(0, 3)) if d == 3 else 0, d, int(rng.integers(700, 2900)), L=int(rng.integers(30, 60)), jitter=2)
    cols = dict(pos=[], l_qseq=[], frag_id=[], fam_id=[], fam_strand=[], flag=[])
    frag = 0
    for f, (a, b, dflag, x, L, two_aln, jitter) in enumerate(fams):
        for strand, cnt in ((0, a), (1, b)):
            for k in range(cnt):
                for _ in range(2 if (two_aln and strand == 0 and k == 0) else 1):
                    cols["pos"].append(B + x + (int(rng.integers(0, jitter)) if jitter else 0)); cols["l_qseq"].append(L)
                    cols["frag_id"].append(frag); cols["fam_id"].append(f); cols["fam_strand"].append(strand); cols["flag"].append(16 if strand else 0)
                frag += 1
    n = len(cols["pos"])
    lq = np.asarray(cols["l_qseq"], np.int32)
    ref = rng.integers(0, 4, LEN)
    seq_off = np.concatenate(([0], np.cumsum(lq)))[:n].astype(np.int64)
    idx = np.concatenate([np.arange(p - B, p - B + L) for p, L in zip(cols["pos"], lq)])
    reads = dict(n_reads=n, pos=np.asarray(cols["pos"], np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), flag=np.asarray(cols["flag"], np.uint16),
                 mapq=np.full(n, 60, np.uint8), nm=np.zeros(n, np.int32), l_qseq=lq, seq_off=seq_off, cigar_off=np.arange(n, dtype=np.int64), n_cigar=np.ones(n, np.int32),
                 frag_id=np.asarray(cols["frag_id"], np.int32), fam_id=np.asarray(cols["fam_id"], np.int32), fam_strand=np.asarray(cols["fam_strand"], np.uint8), n_fams=len(fams),
                 fam_dflag=np.asarray([f[2] for f in fams], np.uint8), bases=ref[idx].astype(np.uint8), quals=np.full(int(lq.sum()), 30, np.uint8), cigars=(lq.astype(np.uint32) << 4),
                 tid=2, beg=B, end=B + LEN, refseq="".join("ACGT"[b] for b in ref))
    return reads, named


SITUATIONS = [(B + 100, B + 200, B + 60, 0), (B + 300, B + 340, B + 200, 0), (B + 340, B + 400, B + 340, 1),
              (B + 500, B + 510, B + 400, 0), (B + 520, B + 530, B + 510, 0), (B + 540, B + 550, B + 530, 0)]


@pytest.fixture(scope="module")
def hand(gpu_lib):
    reads, named = hand_built()
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    yield reads, named, fr.families(reads), R
    R.close()


def assert_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == np.int64, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:8]])


def test_the_hand_built_input_holds_what_it_is_for(hand):
    reads, named, fams, _ = hand
    assert reads["end"] - reads["beg"] <= 3000 and len(fams["a"]) >= 6000 + 18
    sizes = set(zip(fams["a"].tolist(), fams["b"].tolist()))
    assert {(1, 0), (0, 1), (1, 1), (15, 1), (16, 16), (17, 0), (31, 32), (32, 32), (40, 30), (3000, 0)} <= sizes
    two = named["two_alignments"]
    assert (fams["a"][two], fams["n"][two]) == (2, 3)                      # a fragment of two alignments beside one of one
    assert set(fams["dflag"].tolist()) == {0, 1, 3, 4}
    lo, hi = fams["lo"], fams["hi"]
    r = SITUATIONS
    assert lo[named["lo_is_pos_end"]] == r[0][1] and hi[named["hi_is_pos_beg"]] == r[0][0]
    assert lo[named["before_prev_end"]] < r[0][2] and hi[named["before_prev_end"]] > r[0][0]
    assert r[1][1] == r[2][0] and r[2][3] == 1 and lo[named["straddles_joint"]] < r[2][0] < hi[named["straddles_joint"]]
    assert hi[named["between"]] <= r[3][0] and lo[named["between"]] >= r[2][1]
    assert lo[named["spans_three"]] < r[3][1] and hi[named["spans_three"]] > r[5][0]
    # ... and the restatement's own rows show each situation: literal TARGET / FIRST family counts of the six ranges
    want = fr.rows(fams, SITUATIONS)
    assert want[:, fr.TARGET].tolist() == [1, 1, 1, 1, 1, 1]     # before_prev_end; straddles_joint (once over the two pieces); inside_continuing; spans_three x 3
    assert want[:, fr.FIRST].tolist() == [0, 1, 1, 1, 0, 0]      # before_prev_end is TARGET only; spans_three is in one FIRST block
    assert want[:, fr.TARGET + 1].tolist() == [1, 2, 2, 1, 1, 1] and want[2, fr.TARGET + 3] == 1 and want[2, fr.FLAGS + 1] == 1
    whole = fr.rows(fams, [(B, B + LEN + 1, B, 0)])[0]
    assert whole[fr.TARGET] == whole[fr.FIRST] == len(fams["a"])
    assert (whole[:fr.FLAGS + 3] > 0).all() and whole[fr.FLAGS + 3] == 0, "every counter is non-zero somewhere"
    assert whole[fr.SIZE + 62] == 1 and whole[fr.SIZE + 63] == 3, "a + b = 63, and 64 / 70 / 3000 in the 64+ bin"
    S = lambda a, b: whole[fr.STRANDS + a * 17 + b]   # noqa: E731
    assert S(16, 16) == 4 and S(16, 0) == 2 and S(15, 1) == 1 and S(0, 1) >= 1, "the capped strand bins: (16,16) (31,32) (32,32) (40,30) -> [16][16]; (17,0) and the pile -> [16][0]"


def test_hand_built_rows_equal_the_restatement(hand):
    reads, named, fams, R = hand
    lists = {"the situations": SITUATIONS,
             "the whole region": [(B, B + LEN + 1, B, 0)],
             "1000 one-base ranges": [(B + 700 + k, B + 701 + k, B + 700 + max(k, 0), 0) for k in range(1000)],
             "1000 one-base ranges, every second continuing": [(B + 1400 + k, B + 1401 + k, B + 1400 + k, k & 1) for k in range(1000)],
             "seventeen ranges (one more than a block's window)": [(B + 600 + 140 * k, B + 600 + 140 * k + 100, B + 600 + 140 * k - (40 if k else 0), 0) for k in range(17)]}
    for what, ranges in lists.items():
        got = R.family_stats(ranges)
        assert_rows(got, fr.rows(fams, ranges), what)
        assert got.any(), what
        assert np.array_equal(R.family_stats(ranges), got), "two calls, the same bits"


# ------------------------------------------------------------------------------------------------ synthetic inputs
@pytest.mark.parametrize("name", ["umi_duplex_2kb_400x", "config4shape_1kb_2000x_duplex", "config2shape_5kb_300x"])
def test_synthetic_rows_equal_the_restatement(name, gpu_lib):
    reads = synth.generate_region(**CASES[name])
    fams = fr.families(reads)
    p = region.default_params(gpu_lib)
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    cols = DeviceColumns(reads)
    Rd = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Rd.set_reads_device((cols.soa, cols))
    rng = np.random.default_rng(17)
    n_lists = 0
    for what, pairs in range_lists(rng, R.beg, R.npos):
        ranges = [(a, b, pairs[k - 1][1] if k else a, 0) for k, (a, b) in enumerate(pairs)]
        got = R.family_stats(ranges)
        assert_rows(got, fr.rows(fams, ranges), (name, what))
        assert np.array_equal(R.family_stats(ranges), got), (name, what, "two calls, the same bits")
        assert np.array_equal(Rd.family_stats(ranges), got), (name, what, "device columns")
        n_lists += 1
    assert n_lists == 10
    beg, end = R.beg, R.beg + R.npos
    whole = R.family_stats([(beg, end, beg, 0)])[0]
    print(name, dict(zip(fr.FIRST_NAMES, whole[fr.FIRST:fr.FIRST + 7].tolist())))
    assert whole[fr.FIRST] == len(fams["a"]) > 0
    if "duplex" in name:
        assert whole[fr.FIRST + 3] > 0 and whole[fr.TARGET + 3] > 0, "the duplex input has no family on both strands"
    cuts = [beg, beg + 70, beg + 71, beg + 200, beg + R.npos // 2, end - 5, end]
    part = R.family_stats([(a, b, a, 0) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(part[:, fr.FIRST:].sum(0), whole[fr.FIRST:]), "the FIRST blocks over a partition sum to the FIRST block of the whole"
    assert part[:, fr.TARGET].sum() >= whole[fr.TARGET]
    Rd.close(); cols.free(); R.close()


# ------------------------------------------------------------------------------------------------ argument checks and states
def test_refusals_and_legal_states(gpu_lib):
    reads = synth.generate_region(**CASES["umi_duplex_2kb_400x"])
    fams = fr.families(reads)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, end = R.beg, R.beg + R.npos
    fn = gpu_lib.dll.uvcgpu_region_family_stats
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    sentinel = -0x5151515151515151

    def call(ranges, n=None, null_ranges=False, null_out=False):
        arr = (_ffi.UvcFamilyRange * len(ranges))(*[_ffi.UvcFamilyRange(*q) for q in ranges])
        out = np.full((len(ranges), ROW), sentinel, np.int64)
        rc = fn(R.h, None if null_ranges else arr, len(ranges) if n is None else n, None if null_out else out.ctypes.data)
        return rc, out, gpu_lib.last_error()

    ok = [(beg + 5, beg + 100, beg + 5, 0), (beg + 100, beg + 101, beg + 100, 1), (beg + 300, end, beg + 150, 0)]
    rc, out, msg = call(ok)
    assert rc == EINVAL and "set_reads" in msg and (out == sentinel).all()
    R.set_reads(reads)
    want = fr.rows(fams, ok)
    assert want.any()
    assert_rows(R.family_stats(ok), want, "after set_reads, before accumulate")
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
        ("NULL ranges", dict(ranges=ok, null_ranges=True), "NULL"),
        ("NULL out", dict(ranges=ok, null_out=True), "NULL"),
    ]
    for what, kw, word in bad_calls:
        rc, out, msg = call(**kw)
        assert rc == EINVAL and word in msg and "family_stats" in msg, (what, rc, msg)
        assert (out == sentinel).all(), what
        assert_rows(R.family_stats(ok), want, "a valid call after: " + what)
    # accumulate and scores neither are needed nor get in the way: the units belong to the reads, a releasing score gives up the planes only
    R.accumulate()
    assert_rows(R.family_stats(ok), want, "after accumulate")
    R.score()
    assert_rows(R.family_stats(ok), want, "after a plain score")
    R.score(release_state=True)
    assert_rows(R.family_stats(ok), want, "after a releasing score")
    R.accumulate()
    gen = R.score_stream(4096)
    first = next(gen)
    assert_rows(R.family_stats(ok), want, "while a score stream is open")
    assert len(first[0]["refpos"]) > 0
    for _ in gen:
        pass
    assert_rows(R.family_stats(ok), want, "after the stream")
    # a region with zero reads gives rows of zeros; a reset takes the units away
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and k != "fam_dflag" else v) for k, v in reads.items()}
    empty["n_reads"] = 0
    R.set_reads(empty)
    rc, out, msg = call(ok)
    assert rc == 0 and not out.any()
    R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    rc, out, msg = call(ok)
    assert rc == EINVAL and "set_reads" in msg and (out == sentinel).all()
    R.close()


def test_a_library_without_the_symbol_says_so(oracle_lib):
    reads = synth.generate_region(**CASES["tiny_600bp_5x"])
    R = region.Region(oracle_lib, region.default_params(oracle_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    with pytest.raises(region.UvcError, match="region_family_stats"):
        R.family_stats([(R.beg, R.beg + 10)])
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def chain_report(gpu_lib, hb, hf, lines, clen):
    """The report from the Python chain: one region per BED line (uvc_amd.pipeline.call_region), Region.family_stats with the line as the one
    piece and prev_end = the largest end of the lines before it on the contig (at most the line's begin; 0 for the first), the
    restatement's text.  -> (text, the summed rows of the run)."""
    total, per_target, targets, reach = np.zeros(ROW, np.int64), [], [], {}
    for chrom, b, e, name in lines:
        cb, ce = max(0, b), min(e, clen[chrom])
        row = np.zeros(ROW, np.int64)
        res = pipeline.call_region(gpu_lib, hb, hf, chrom, cb, ce, keep_handle=True) if ce > cb else None
        if res is not None:
            row = res["region"].family_stats([(cb, ce, min(cb, reach.get(chrom, 0)), 0)])[0]
            res["region"].close()
        if ce > cb:
            reach[chrom] = max(reach.get(chrom, 0), ce)
        total += row
        per_target.append(row[:4])
        targets.append((chrom, b, e, name))
    return fr.report_text(targets, per_target, total), total


def summary_of(text):
    sec = text.split("#summary\n")[1].split("#family_size")[0]
    return {l.split("\t")[0]: int(l.split("\t")[1]) for l in sec.splitlines()}


def test_cli_family_stats_report(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    want, total = chain_report(gpu_lib, hb, hf, lines, clen)
    assert total[fr.FIRST] > 100 and total[fr.FIRST + 1] > total[fr.FIRST]
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2")
    vcf_with = run_cli(bam, fa, o("f.vcf.gz"), "-R", bed, "-t", "2", "--family-stats-out", o("f.tsv"))
    got = open(o("f.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100
    for threads in (1, 4):
        assert run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "-t", str(threads), "--family-stats-out", o("t.tsv")) == vcf_without
        assert open(o("t.tsv")).read() == got, threads
    assert run_cli(bam, fa, o("s.vcf.gz"), "-R", bed, "-t", "2", "--score-mem-mb", "16", "--family-stats-out", o("s.tsv")) == vcf_without
    assert open(o("s.tsv")).read() == got
    # merged regions group the reads of a batch together: the same bytes for any number of workers, and the unchanged VCF
    vcf_m = run_cli(bam, fa, o("m0.vcf.gz"), "-R", bed, "-t", "2", "--merge-regions", "2000")
    merged = []
    for threads in (1, 4):
        assert run_cli(bam, fa, o("m.vcf.gz"), "-R", bed, "-t", str(threads), "--merge-regions", "2000", "--family-stats-out", o("m.tsv")) == vcf_m
        merged.append(open(o("m.tsv")).read())
    assert merged[0] == merged[1] and summary_of(merged[0])["families"] > 100
    # .gz is the same text, block-gzipped
    run_cli(bam, fa, o("z.vcf.gz"), "-R", bed, "-t", "2", "--family-stats-out", o("z.tsv.gz"))
    assert gzip.open(o("z.tsv.gz"), "rt").read() == got and open(o("z.tsv.gz"), "rb").read()[12:16] == b"BC\x02\x00"
    # the three reports together are the reports of the runs with one of them
    run_cli(bam, fa, o("c1.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("c1.tsv"))
    run_cli(bam, fa, o("e1.vcf.gz"), "-R", bed, "-t", "2", "--error-profile-out", o("e1.tsv"))
    vcf_all = run_cli(bam, fa, o("a.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("c3.tsv"), "--error-profile-out", o("e3.tsv"), "--family-stats-out", o("f3.tsv"))
    assert vcf_all == vcf_without
    assert open(o("c3.tsv")).read() == open(o("c1.tsv")).read() and open(o("e3.tsv")).read() == open(o("e1.tsv")).read() and open(o("f3.tsv")).read() == got
    # --tile cuts the long line: a family next to a cut is the family of the tile's own fetch, so only the VCF and the
    # report's own consistency are promised
    vcf_tile0 = run_cli(bam, fa, o("k0.vcf.gz"), "-R", bed, "-t", "2", "--tile", "1000")
    assert run_cli(bam, fa, o("k.vcf.gz"), "-R", bed, "-t", "2", "--tile", "1000", "--family-stats-out", o("k.tsv")) == vcf_tile0
    k = open(o("k.tsv")).read()
    size_sec = k.split("#family_size\tfamilies\n")[1].split("#strand0_size")[0]
    assert summary_of(k)["families"] == sum(int(l.split("\t")[1]) for l in size_sec.splitlines()) > 100
    assert [l.split("\t")[:4] for l in k.split(fr.TARGET_HEADER + "\n")[1].splitlines()] == [[c, str(b), str(e), n or "."] for c, b, e, n in lines]
    # fixed windows without a BED file
    vcf_w0 = run_cli(bam, fa, o("w0.vcf.gz"), "-t", "2", "--tile", "1000000")
    assert run_cli(bam, fa, o("w.vcf.gz"), "-t", "2", "--tile", "1000000", "--family-stats-window", "5000", "--family-stats-out", o("w.tsv")) == vcf_w0
    w = open(o("w.tsv")).read()
    rows = [l.split("\t") for l in w.split(fr.TARGET_HEADER + "\n")[1].splitlines()]
    assert [(r[0], int(r[1]), int(r[2])) for r in rows] == [(c, q * 5000, min((q + 1) * 5000, clen[c])) for c in ("chrA", "chrB", "chrC") for q in range(-(-clen[c] // 5000))]
    s = summary_of(w)
    # every window is a target of its own: a family over a window border counts in both, so the target lines sum to at least the summary
    assert s["families"] > 100 and sum(int(r[4]) for r in rows) >= s["families"] and all(r[4] == "0" for r in rows if r[0] == "chrC")
