"""Depth statistics of ranges of the accumulated planes (uvcgpu_region_coverage, Region.coverage) and the per-target report built from them
(uvc1-mi355x --coverage-out).  Every number is an integer and is compared for equality:
  * the rows of the HIP library against numpy reductions of the ORACLE's fetched planes (PREP32 / FRAG / FAM / DUPLEX), with the sums of
    include/uvc_coverage.def -- both strands, the six BASE symbols;
  * aDP / bDP / cDP1 / cDP12 of single positions against columns 8 / 4 / 5 / 6 of the block statistics the MGVCF writer reads on the same handle;
  * the refusals of the ABI, which launch nothing, leave `out` alone and leave the handle usable;
  * the report of the command line against the Python chain (uvc_amd.pipeline regions + Region.coverage), across --tile, -t, --merge-regions
    and --score-mem-mb, with targets that have no reads, and as fixed windows.
Range lists: ~200 random disjoint ranges of 1-5000 bp need a few hundred kb: the 300 kb region holds them; the suite's oracle-sized regions
(1-5 kb) get ~200 random disjoint ranges as long as they can hold."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bamwriter
from test_gpu_parity import CASES
from util import run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
E = _ffi.ENUMS
NCOV, ROW, GE = E["UVC_NCOV"], E["UVC_COV_ROW"], E["UVC_COV_GE"]
EINVAL = E["UVCGPU_EINVAL"]
INPUTS = {
    "plain_300x": CASES["config2shape_5kb_300x"],
    "umi_2kb_400x": CASES["umi_duplex_2kb_400x"],
    "duplex_1kb_2000x": CASES["config4shape_1kb_2000x_duplex"],
    "wide_300kb_8x": dict(region_len=300000, depth=8, seed=21),
}
THR = [1, 20, 100, 500]


def measures_of(fetch):
    """Per-position values of the six measures, int64 [NCOV][npos], from a `fetch(group)` of plane groups: the sums of uvc_coverage.def."""
    base = slice(E["UVC_BASE_A"], E["UVC_BASE_NN"] + 1)
    prep, frag, fam, dup = (fetch(g) for g in ("PREP32", "FRAG", "FAM", "DUPLEX"))
    return np.stack([prep[E["UVC_P_a_dp"]].astype(np.int64),
                     frag[:, E["UVC_FRAG_bDP"], base].sum((0, 1), dtype=np.int64),
                     fam[:, E["UVC_FAM_cDP1"], base].sum((0, 1), dtype=np.int64),
                     fam[:, E["UVC_FAM_cDP12"], base].sum((0, 1), dtype=np.int64),
                     fam[:, E["UVC_FAM_cDP2"], base].sum((0, 1), dtype=np.int64),
                     dup[E["UVC_DUPLEX_dDP1"], base].sum(0, dtype=np.int64)])


def rows_of(m, beg, ranges, thr):
    out = np.zeros((len(ranges), NCOV, GE + len(thr)), np.int64)
    for i, (a, b) in enumerate(ranges):
        d = m[:, a - beg:b - beg]
        out[i, :, 0], out[i, :, 1], out[i, :, 2] = d.sum(1), d.min(1), d.max(1)
        for k, t in enumerate(thr):
            out[i, :, GE + k] = (d >= t).sum(1)
    return out


def random_disjoint(rng, lo, hi, n, max_len):
    """Up to n sorted disjoint ranges inside [lo, hi) with lengths 1..max_len (log-uniform) and gaps 0.. (neighbours may touch)."""
    out, at = [], lo
    room = max(1, (hi - lo) // n)
    while at < hi and len(out) < n:
        at += int(rng.integers(0, room)) if rng.random() < 0.7 else 0
        if at >= hi:
            break
        ln = min(int(min(max_len, np.exp(rng.uniform(0, np.log(max_len))))), hi - at)
        out.append((at, at + ln))
        at += ln
    return out


def range_lists(rng, beg, npos):
    end = beg + npos
    yield "the whole region", [(beg, end)]
    yield "single positions at both ends", [(beg, beg + 1), (end - 1, end)]
    yield "the first and the last two", [(beg, beg + 2), (end - 2, end)]
    yield "adjacent ranges that share end points", [(beg + 3, beg + 70), (beg + 70, beg + 71), (beg + 71, beg + 200), (beg + 200, end - 5), (end - 5, end)]
    yield "every position of a stretch", [(p, p + 1) for p in range(beg + 100, beg + 300)]
    yield "64-position boundaries", [(beg, beg + 64), (beg + 64, beg + 127), (beg + 127, beg + 129), (beg + 192, beg + 448), (beg + 449, beg + 512)]
    for k in range(3):
        r = random_disjoint(rng, beg, end, 200, (min(5000, npos), max(8, npos // 25), 40)[k])
        yield "random %d (%d ranges, longest %d)" % (k, len(r), max(b - a for a, b in r)), r
    r = random_disjoint(rng, beg, end, 200, 12)
    yield "random short (%d ranges)" % len(r), r


@pytest.mark.parametrize("name", list(INPUTS))
def test_rows_equal_numpy_over_the_oracles_planes(name, oracle_lib, gpu_lib):
    reads = synth.generate_region(**INPUTS[name])
    Ro, Rg = run_region(oracle_lib, reads), run_region(gpu_lib, reads)
    m = measures_of(Ro.fetch)
    Ro.close()
    assert m.shape == (NCOV, Rg.npos) and Rg.npos == reads["end"] - reads["beg"] + 1
    tot = dict(zip(region.COVERAGE_MEASURES, m.sum(1).tolist()))
    print(name, "per-measure totals over the region:", tot)
    assert tot["aDP"] > 0 and tot["bDP"] > 0 and tot["cDP1"] > 0 and tot["cDP12"] > 0
    if name.startswith("umi"):
        assert tot["cDP2"] > 0, "the UMI input has no family large enough for a consensus: cDP2 cannot be told from an unwired plane"
    if name.startswith("duplex"):
        assert tot["dDP1"] > 0 and tot["cDP2"] > 0, "the duplex input has no duplex family: dDP1 cannot be told from an unwired plane"
    rng = np.random.default_rng(17)
    n_lists = 0
    for what, ranges in range_lists(rng, Rg.beg, Rg.npos):
        for thr in (THR, [], [0, 1, 2, 3, 5, 8, 13, 2000]):
            got = Rg.coverage(ranges, thr)
            want = rows_of(m, Rg.beg, ranges, thr)
            assert got.shape == want.shape and got.dtype == np.int64
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (name, what, thr, [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])
        n_lists += 1
    assert n_lists == 10
    # unused threshold slots of a row are 0 in the ABI's own layout
    fn = gpu_lib.dll.uvcgpu_region_coverage
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    arr = (_ffi.UvcCoverageRange * 1)(_ffi.UvcCoverageRange(Rg.beg, Rg.beg + Rg.npos))
    raw = np.full((1, NCOV, ROW), -7, np.int64)
    thr2 = np.array([1, 50], np.int32)
    assert fn(Rg.h, arr, 1, thr2.ctypes.data, 2, raw.ctypes.data) == 0
    assert np.array_equal(raw[:, :, :GE + 2], rows_of(m, Rg.beg, [(Rg.beg, Rg.beg + Rg.npos)], [1, 50])) and not raw[:, :, GE + 2:].any()
    Rg.close()


@pytest.mark.parametrize("name", ["plain_300x", "umi_2kb_400x"])
def test_single_positions_equal_the_block_statistics_of_the_writer(name, gpu_lib):
    """The MGVCF writer's per-position numbers (uvcgpu_region_block_stats_, the library's internal entry point behind uvcgpu_region_vcf_records:
    10 ints per position, block_stats_at) on the same handle: o[8] = aDP, o[4] = bDP, o[5] = cDP1, o[6] = cDP12 of the BASE type."""
    reads = synth.generate_region(**INPUTS[name])
    R = run_region(gpu_lib, reads)
    fn = gpu_lib.dll.uvcgpu_region_block_stats_
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    st = np.zeros((R.npos, 10), np.int32)
    assert fn(R.h, R.beg, R.beg + R.npos, st.ctypes.data) == 0, gpu_lib.last_error()
    got = R.coverage([(p, p + 1) for p in range(R.beg, R.beg + R.npos)], [1])
    assert got.shape == (R.npos, NCOV, GE + 1)
    for mi, col in ((0, 8), (1, 4), (2, 5), (3, 6)):
        for stat in (0, 1, 2):   # a single position: sum = min = max = the depth
            assert np.array_equal(got[:, mi, stat], st[:, col].astype(np.int64)), (region.COVERAGE_MEASURES[mi], col, stat)
        assert np.array_equal(got[:, mi, GE], (st[:, col] >= 1).astype(np.int64))
    assert st[:, 8].sum() > 0 and st[:, 4].sum() > 0 and st[:, 5].sum() > 0 and st[:, 6].sum() > 0
    R.close()


def test_argument_checks(oracle_lib, gpu_lib):
    reads = synth.generate_region(**CASES["tiny_600bp_5x"])
    fn = gpu_lib.dll.uvcgpu_region_coverage
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, end = R.beg, R.beg + R.npos
    sentinel = -123456789

    def call(ranges, thr=(1, 20), n_thr=None, n=None, null_ranges=False, null_out=False):
        arr = (_ffi.UvcCoverageRange * max(len(ranges), 1))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])
        t = np.ascontiguousarray(thr, dtype=np.int32)
        out = np.full((max(len(ranges), 1), NCOV, ROW), sentinel, np.int64)
        rc = fn(R.h, None if null_ranges else arr, len(ranges) if n is None else n, t.ctypes.data if len(t) else None, len(t) if n_thr is None else n_thr, None if null_out else out.ctypes.data)
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
    m = measures_of(Ro.fetch)
    Ro.close()
    want = rows_of(m, beg, ok, [1, 20])
    assert np.array_equal(R.coverage(ok, [1, 20]), want)
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250), (beg + 10, beg + 50)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50), (beg + 49, beg + 60)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50), (beg + 60, beg + 60)]), "range 1"),
        ("reversed", dict(ranges=[(beg + 50, beg + 10)]), "range 0"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20), (end - 3, end + 1)]), "range 1"),
        ("descending thresholds", dict(ranges=ok, thr=(20, 1)), "threshold 1"),
        ("equal thresholds", dict(ranges=ok, thr=(5, 5)), "threshold 1"),
        ("negative threshold", dict(ranges=ok, thr=(-1, 5)), "threshold 0"),
        ("nine thresholds", dict(ranges=ok, thr=tuple(range(1, 10))), "n_thresholds"),
        ("negative n_thresholds", dict(ranges=ok, n_thr=-1), "n_thresholds"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null_ranges=True), "NULL"),
        ("NULL out", dict(ranges=ok, null_out=True), "NULL"),
    ]
    for what, kw, word in bad_calls:
        rc, out, msg = call(**kw)
        assert rc == EINVAL and word in msg, (what, rc, msg)
        assert (out == sentinel).all(), what
        # the handle is as usable as before: the next valid call gives the right rows
        assert np.array_equal(R.coverage(ok, [1, 20]), want), what
    # a plain score keeps the planes: coverage still answers; a releasing score comes after it, and then it is refused
    R.score()
    assert np.array_equal(R.coverage(ok, [1, 20]), want)
    R.score(release_state=True)
    rc, out, msg = call(ok)
    assert rc == EINVAL and "release" in msg and (out == sentinel).all()
    # the next accumulate brings the planes back
    R.set_reads(reads)
    R.accumulate()
    assert np.array_equal(R.coverage(ok, [1, 20]), want)
    # while a score stream is open the planes may go at any moment: refused; after its end the handle answers again
    gen = R.score_stream(4096)
    next(gen)
    rc, out, msg = call(ok)
    assert rc == EINVAL and "stream" in msg and (out == sentinel).all()
    gen.close()
    assert np.array_equal(R.coverage(ok, [1, 20]), want)
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def panel(d):
    """A synthetic BAM over three contigs -- chrA and chrB with reads over 30 000..36 000, chrC without any -- and a BED file: some twenty short
    lines (sorted per contig, two that abut), one long line that --tile cuts, a line beyond the reads, one on the read-less contig and one
    that runs over the end of its contig."""
    refs, recs, seqs = [], [], []
    rng = np.random.default_rng(9)
    for tid, (name, seed) in enumerate((("chrA", 51), ("chrB", 53))):
        reads = synth.generate_region(seed=seed, region_len=6000, depth=60, beg=30000, snv_every=120, somatic_every=400, indel_every=300)
        recs += bamwriter.records_from_reads(reads, tid=tid, qname_fmt=name + "r%d")
        chrom_len = reads["end"] + 5000
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, chrom_len))
        seqs.append((name, seq[:reads["beg"]] + reads["refseq"] + seq[reads["end"]:]))
        refs.append((name, chrom_len))
    refs.append(("chrC", 3000))
    seqs.append(("chrC", "".join("ACGT"[i] for i in rng.integers(0, 4, 3000))))
    bam, fa = os.path.join(d, "p.bam"), os.path.join(d, "p.fa")
    bamwriter.write_bam(bam, refs, recs)
    bamwriter.write_fasta(fa, seqs)
    lines = []
    for name, n in (("chrA", 12), ("chrB", 9)):
        starts = np.sort(rng.choice(np.arange(30300, 35400, 260), n, replace=False))
        for k, s in enumerate(starts.tolist()):
            lines.append((name, s, s + int(rng.integers(40, 250)), "%s exon %d" % (name, k)))   # a name with blanks: column 4 runs to the next tab
    lines.insert(5, (lines[4][0], lines[4][2], lines[4][2] + 3, "abuts"))
    clen = dict(refs)
    lines.append(("chrB", 29500, 36400, "long"))                             # cut by --tile 1000; begins in front of the reads
    lines.append(("chrB", 38000, 38100, "beyond_the_reads"))
    lines.append(("chrC", 100, 400, None))                                   # no name column
    lines.append(("chrB", clen["chrB"] - 100, clen["chrB"] + 200, "over_the_end"))
    bed = os.path.join(d, "panel.bed")
    with open(bed, "w") as f:
        f.write("# a panel\n" + "".join(("%s\t%d\t%d" % l[:3]) + ("\t%s\t0\t+\n" % l[3] if l[3] else "\n") for l in lines))
    return bam, fa, bed, lines, clen


def run_cli(bam, fa, out, *extra):
    r = subprocess.run([EXE, bam, "-f", fa, "-o", out, "-s", "S"] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l for l in gzip.open(out, "rt").read().splitlines() if not l.startswith(("##fileDate=", "##variantCallerCommand="))]


def tsv_header(thr):
    return "\t".join(["#chrom", "beg", "end", "name", "len"] + [m + s for m in region.COVERAGE_MEASURES for s in ["_sum", "_min", "_max"] + ["_ge%d" % t for t in thr]])


def chain_depths(gpu_lib, bam, fa, chrom, beg, end):
    """Per-position values of the six measures over [beg, end) of a contig from the Python chain: one region (uvc_amd.pipeline.call_region), the
    positions it owns through Region.coverage as single-position ranges, 0 elsewhere."""
    d = np.zeros((NCOV, end - beg), np.int64)
    res = pipeline.call_region(gpu_lib, bam, fa, chrom, beg, end, keep_handle=True) if end > beg else None
    if res is not None:
        a, b = res["score_range"][0], min(res["score_range"][1], end)
        if b > a:
            d[:, a - beg:b - beg] = res["region"].coverage([(p, p + 1) for p in range(a, b)], [])[:, :, 0].T
        res["region"].close()
    return d


def test_cli_coverage_report(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    # (a) the report equals the Python chain, merged per BED line: each line its own region, the owned positions reduced with numpy's rules
    want = [tsv_header(THR)]
    per_line = []
    for chrom, b, e, name in lines:
        cb, ce = max(0, b), min(e, clen[chrom])
        dep = chain_depths(gpu_lib, hb, hf, chrom, cb, ce)
        per_line.append(dep)
        row = rows_of(dep, 0, [(0, ce - cb)], THR)[0] if ce > cb else np.zeros((NCOV, GE + len(THR)), np.int64)
        want.append("\t".join([chrom, str(b), str(e), name or ".", str(max(0, ce - cb))] + [str(v) for v in row.reshape(-1)]))
    want = "\n".join(want) + "\n"
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2")
    vcf_with = run_cli(bam, fa, o("cov.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("cov.tsv"))
    got = open(o("cov.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    # (e) the VCF does not know about the report
    assert vcf_with == vcf_without and len(vcf_with) > 100
    # (f) targets without reads are rows of zeros with the right length
    rows = {l.split("\t")[3]: l.split("\t") for l in got.splitlines()[1:]}
    assert rows["beyond_the_reads"][4] == "100" and set(rows["beyond_the_reads"][5:]) == {"0"}
    assert rows["."][0] == "chrC" and rows["."][4] == "300" and set(rows["."][5:]) == {"0"}
    assert rows["over_the_end"][4] == "100" and set(rows["over_the_end"][5:]) == {"0"}
    assert int(rows["long"][5]) > 0 and rows["long"][6] == "0"                 # begins in front of the reads: aDP_min 0
    assert [l.split("\t")[3] for l in got.splitlines()[1:]] == [n or "." for _, _, _, n in lines]   # BED file order
    # (b) the same bytes however the lines are cut and however many workers run
    for tile, threads in ((1000, 1), (7000, 4), (1000, 4)):
        run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "-t", str(threads), "--tile", str(tile), "--coverage-out", o("t.tsv"))
        assert open(o("t.tsv")).read() == got, (tile, threads)
    run_cli(bam, fa, o("t1.vcf.gz"), "-R", bed, "-t", "1", "--coverage-out", o("t1.tsv"))
    assert open(o("t1.tsv")).read() == got
    # (c) merged regions hold the same depths
    run_cli(bam, fa, o("m.vcf.gz"), "-R", bed, "-t", "2", "--merge-regions", "2000", "--coverage-out", o("m.tsv"))
    assert open(o("m.tsv")).read() == got
    # (d) the streamed score comes after the report, like the one call
    vcf_s = run_cli(bam, fa, o("s.vcf.gz"), "-R", bed, "-t", "2", "--score-mem-mb", "16", "--coverage-out", o("s.tsv"))
    assert open(o("s.tsv")).read() == got and vcf_s == vcf_without
    run_cli(bam, fa, o("ms.vcf.gz"), "-R", bed, "-t", "2", "--merge-regions", "2000", "--score-mem-mb", "16", "--coverage-out", o("ms.tsv"))
    assert open(o("ms.tsv")).read() == got
    # (h) .gz is the same text, block-gzipped; other thresholds change the count columns only
    run_cli(bam, fa, o("z.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("z.tsv.gz"))
    assert gzip.open(o("z.tsv.gz"), "rt").read() == got and open(o("z.tsv.gz"), "rb").read()[12:16] == b"BC\x02\x00"
    run_cli(bam, fa, o("k.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("k.tsv"), "--coverage-thresholds", "0,30")
    k = open(o("k.tsv")).read().splitlines()
    assert k[0] == tsv_header([0, 30])
    for lk, lg, dep, (chrom, b, e, name) in zip(k[1:], got.splitlines()[1:], per_line, lines):
        fk, fg = lk.split("\t"), lg.split("\t")
        w = rows_of(dep, 0, [(0, dep.shape[1])], [0, 30])[0] if dep.shape[1] else np.zeros((NCOV, GE + 2), np.int64)
        assert fk[:5] == fg[:5] and fk[5:] == [str(v) for v in w.reshape(-1)], name
    # (g) fixed windows without a BED file: the rows of a contig sum to the per-position totals of the chain over that contig
    whole = {c: chain_depths(gpu_lib, hb, hf, c, 0, clen[c]) for c in clen}
    for extra in (["--tile", "1000000"], ["--tile", "1700"], []):           # one tile per contig, tiles that cut windows, the reference's own region cuts
        run_cli(bam, fa, o("w.vcf.gz"), "-t", "2", "--coverage-window", "1000", "--coverage-out", o("w.tsv"), *extra)
        w = [l.split("\t") for l in open(o("w.tsv")).read().splitlines()]
        assert "\t".join(w[0]) == tsv_header(THR)
        at = 1
        for c in ("chrA", "chrB", "chrC"):                                  # window order per contig, contigs in header order
            n_win = -(-clen[c] // 1000)
            mine = w[at:at + n_win]
            at += n_win
            assert [(r[0], int(r[1]), int(r[2]), r[3], int(r[4])) for r in mine] == [(c, q * 1000, min((q + 1) * 1000, clen[c]), ".", min((q + 1) * 1000, clen[c]) - q * 1000) for q in range(n_win)], (extra, c)
            for q, r in enumerate(mine):
                dep = whole[c][:, q * 1000:min((q + 1) * 1000, clen[c])]
                assert r[5:] == [str(v) for v in rows_of(dep, 0, [(0, dep.shape[1])], THR)[0].reshape(-1)], (extra, c, q)
        assert at == len(w)
    # --targets clips the windows to the called span
    run_cli(bam, fa, o("g.vcf.gz"), "-t", "2", "--tile", "1000000", "--targets", "chrA:31501-33200", "--coverage-window", "1000", "--coverage-out", o("g.tsv"))
    g = [l.split("\t") for l in open(o("g.tsv")).read().splitlines()[1:]]
    assert [(r[0], r[1], r[2], r[4]) for r in g] == [("chrA", "31500", "32000", "500"), ("chrA", "32000", "33000", "1000"), ("chrA", "33000", "33200", "200")]
