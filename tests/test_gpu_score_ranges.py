"""Many ranges of one accumulated region in one score call (uvcgpu_region_score_ranges / uvcgpu_region_vcf_records_ranges): the records are
those of uvcgpu_region_score called once per range on the same handle, concatenated in range order -- every int32 field equal, germ_ref /
germ_alt1 / germ_alt2 re-based to the returned array -- and the record text is the single-range texts one after another, byte for byte,
MGVCF block and ADDITIONAL_INDEL_CANDIDATE lines included (the default --outvar-flag).  The same records hold against the oracle called
once per range in the suite's tolerance classes (compare_records of test_gpu_parity).  uvc1-mi355x --merge-regions N calls the BED lines
of a batch as ranges of one region: its output equals the Python chain that builds the same batches and calls every line as a single range,
and agrees with the unmerged run in the class DESIGN.md 4c states for cut against uncut runs."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bamwriter
from test_gpu_parity import CASES, compare_records, tumor_keys_from
from util import run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
PLANES = ["PREP32", "PREP64", "SEG32", "SEG64", "FRAG", "FAM", "FAMINFO32", "FAMINFO64", "DUPLEX", "VQ"]
INPUTS = {
    "plain_300x": dict(CASES["config2shape_5kb_300x"], indel_every=300),
    "umi_duplex": CASES["umi_duplex_2kb_400x"],
    "fuzz_weird": None,
}
INDEX_FIELDS = ("germ_ref", "germ_alt1", "germ_alt2")


def reads_of(name):
    if INPUTS[name] is None:                                               # clipped, gapped, N-rich reads of every length (test_gpu_fuzz)
        from test_gpu_fuzz import weird_region
        return weird_region(5, n_frag=400)
    return synth.generate_region(**INPUTS[name])


def range_lists(rng, beg, end):
    """Named lists of (pos_beg, pos_end, base_at_pos_beg, region_beg) inside the scorable span [beg, end - 1) of a region [beg, end)."""
    lo, hi = beg + 1, end - 1
    mid = (lo + hi) // 2
    yield "one range", [(lo + 30, hi - 30, 0, 0)]
    yield "the default range", [(lo, hi, 0, 0)]
    yield "two ranges that touch", [(lo + 10, mid, 0, lo + 10), (mid, hi - 5, 1, lo + 10)]
    yield "two that touch, no base in the second", [(lo + 10, mid, 1, 0), (mid, hi - 5, 0, mid)]
    yield "one position", [(mid, mid + 1, 0, 0)]
    yield "one position with its base, then more", [(mid - 40, mid - 39, 1, mid - 40), (mid - 39, mid - 38, 0, 0), (mid, mid + 1, 1, 0), (mid + 3, mid + 60, 0, mid + 3)]
    yield "the first scorable position", [(beg, beg + 25, 0, beg), (beg + 25, beg + 26, 1, 0), (hi - 20, hi, 1, hi - 20)]
    yield "an empty range among others", [(lo + 5, lo + 5, 0, 0), (lo + 5, lo + 90, 1, 0), (mid, mid, 1, 0), (mid + 7, mid + 99, 0, mid + 7), (hi, hi, 0, 0)]
    for k in range(4):
        n = int(rng.integers(2, 40))
        cuts = np.sort(rng.choice(np.arange(lo, hi + 1), 2 * n, replace=False))
        if k == 3:                                                          # many short ranges: a panel's lines
            starts = np.sort(rng.choice(np.arange(lo, hi - 30, 35), min(60, (hi - lo) // 40), replace=False))
            cuts = np.stack([starts, starts + rng.integers(1, 30, len(starts))], axis=1).reshape(-1)
        out = []
        for a, b in cuts.reshape(-1, 2).tolist():
            out.append((a, b, int(rng.integers(0, 2)), int(rng.choice([0, a, a + 1, (a // 1000) * 1000]))))
        yield "random %d (%d ranges)" % (k, len(out)), out


def concat(parts):
    """Records of single-range calls, one after another, with the record indices moved to the joined array."""
    out, off, offs = {}, 0, []
    for p in parts:
        offs.append(off)
        off += len(p["refpos"])
    for f in parts[0]:
        out[f] = np.concatenate([(np.where(p[f] >= 0, p[f] + o, p[f]) if f in INDEX_FIELDS else p[f]) for p, o in zip(parts, offs)])
    return out


def assert_same(got, want, what):
    assert len(got["refpos"]) == len(want["refpos"]), (what, len(got["refpos"]), len(want["refpos"]))
    bad = [f for f in want if not np.array_equal(got[f], want[f])]
    assert not bad, (what, bad[:6], [(int(np.argmax(got[f] != want[f])), int(got[f][np.argmax(got[f] != want[f])]), int(want[f][np.argmax(got[f] != want[f])])) for f in bad[:3]])


def singles(R, ranges, **kw):
    return [R.score(pos_beg=a, pos_end=b, base_at_pos_beg=bool(c), region_beg=d, **kw) for a, b, c, d in ranges]


@pytest.mark.parametrize("name", list(INPUTS))
def test_ranges_call_equals_the_single_range_calls(name, gpu_lib):
    reads = reads_of(name)
    R = run_region(gpu_lib, reads)
    planes = {g: R.fetch(g).copy() for g in PLANES}
    rng = np.random.default_rng(len(name) + 3)
    n_written = n_block = n_cand = 0
    for what, ranges in range_lists(rng, reads["beg"], reads["end"]):
        inside = np.concatenate([np.arange(a, b) for a, b, _, _ in ranges] + [np.zeros(0, np.int64)])
        gaps = np.concatenate([np.arange(q[1], p[0]) for q, p in zip(ranges, ranges[1:])] + [np.zeros(0, np.int64)])
        sites = np.unique(np.concatenate([rng.choice(inside, min(25, len(inside)), replace=False) if len(inside) else [], rng.choice(gaps, min(10, len(gaps)), replace=False) if len(gaps) else [],
                                          [ranges[0][0] - 3, ranges[-1][1] + 2, ranges[0][0], ranges[-1][1]]]).astype(np.int64))
        for mode in (dict(), dict(all_out=True), dict(kept_only=True), dict(all_out=True, kept_only=True), dict(force_sites=sites), dict(force_sites=sites, kept_only=True)):
            parts = singles(R, ranges, **mode)
            got = R.score_ranges(ranges, **mode)
            assert_same(got, concat(parts), (name, what, sorted(mode)))
            if "kept_only" in mode and "all_out" in mode:
                continue
            # the text, byte for byte: the default outvar_flag writes MGVCF blocks and ADDITIONAL_INDEL_CANDIDATE lines
            text = R.vcf_records_ranges("chrR", got, ranges)
            want = "".join(R.vcf_records("chrR", p, pos_beg=a, pos_end=b, base_at_pos_beg=bool(c), region_beg=d) for p, (a, b, c, d) in zip(parts, ranges))
            assert text == want, (name, what, sorted(mode))
            n_block += text.count("<NON_REF>"); n_cand += text.count("<ADDITIONAL_INDEL_CANDIDATE>"); n_written += int((got["keep"] & got["out"]).sum())
        if len(ranges) == 1:                                               # n_ranges == 1 is the plain call
            a, b, c, d = ranges[0]
            assert_same(R.score_ranges(ranges), R.score(pos_beg=a, pos_end=b, base_at_pos_beg=bool(c), region_beg=d), (name, what, "plain"))
    print(name, "written", n_written, "block lines", n_block, "candidate lines", n_cand)
    assert n_written > 50 and n_block > 20, (n_written, n_block, n_cand)
    # scoring with ranges does not touch the planes
    assert all(np.array_equal(R.fetch(g), planes[g]) for g in PLANES)
    # release_state: the same records while the planes are zeroed behind the kernels
    ranges = list(range_lists(rng, reads["beg"], reads["end"]))[-1][1]
    want = concat(singles(R, ranges))
    assert_same(R.score_ranges(ranges, release_state=True), want, "release_state")
    with pytest.raises(region.UvcError):
        R.score_ranges(ranges)
    R.accumulate()
    assert_same(R.score_ranges(ranges), want, "after the next accumulate")
    R.close()


def test_ranges_with_the_callers_indel_alleles(gpu_lib):
    reads = reads_of("plain_300x")
    R = run_region(gpu_lib, reads)
    full = R.score(all_out=True)
    indel = np.nonzero(np.isin(full["symbol"], (7, 8, 9, 10, 11, 12)) & (full["bDPa"] > 0))[0][::3]
    alleles = sorted(set((int(full["refpos"][i]), int(full["symbol"][i]), 7, 5, 1 + i % 3) for i in indel))
    assert len(alleles) >= 3
    rng = np.random.default_rng(2)
    for what, ranges in range_lists(rng, reads["beg"], reads["end"]):
        assert_same(R.score_ranges(ranges, all_out=True, indel_alleles=alleles), concat(singles(R, ranges, all_out=True, indel_alleles=alleles)), what)
    R.close()


@pytest.mark.parametrize("name", ["plain_300x", "umi_duplex"])
def test_ranges_with_tumor_keys(name, gpu_lib):
    reads = reads_of(name)
    R0 = run_region(gpu_lib, reads)
    keys = tumor_keys_from(R0.score(all_out=False))
    R0.close()
    cols = ["0/1:%d" % i for i in range(len(keys))]
    ras = ["A\tAC" if k[1] in (10, 11, 12) else "AC\tA" if k[1] in (7, 8, 9) else "A\tC" for k in keys]
    p = region.default_params(gpu_lib)
    p.tumor_vcf_is_provided = 1
    R = run_region(gpu_lib, reads, params=p)
    rng = np.random.default_rng(9)
    n = 0
    for what, ranges in range_lists(rng, reads["beg"], reads["end"]):
        parts = singles(R, ranges, tumor_keys=keys)
        got = R.score_ranges(ranges, tumor_keys=keys)
        assert_same(got, concat(parts), (name, what))
        n += int((got["tkey"] >= 0).sum())
        text = R.vcf_records_ranges("chrT", got, ranges, tumor_keys=keys, tumor_sample_columns=cols, tumor_ref_alt=ras)
        want = "".join(R.vcf_records("chrT", q, tumor_keys=keys, pos_beg=a, pos_end=b, base_at_pos_beg=bool(c), region_beg=d, tumor_sample_columns=cols, tumor_ref_alt=ras)
                       for q, (a, b, c, d) in zip(parts, ranges))
        assert text == want, (name, what)
    assert n > 20
    with pytest.raises(region.UvcError, match="force_sites"):
        R.score_ranges(ranges, tumor_keys=keys, force_sites=[ranges[0][0]])
    R.close()


@pytest.mark.parametrize("name,mode", [("config2shape_5kb_300x", "default"), ("config2shape_5kb_300x", "all_out"), ("umi_duplex_2kb_400x", "all_out"),
                                       ("config4shape_1kb_2000x_duplex", "default"), ("config1_10kb_30x", "tumor_keys")])
def test_ranges_records_match_the_oracle_called_once_per_range(name, mode, oracle_lib, gpu_lib):
    """The comparison of test_gpu_parity.test_score_records_match_oracle (depth / count fields exact, Phred-like within 1, x100 within 1 %),
    with the oracle's records made by one plain call per range."""
    reads = synth.generate_region(**CASES[name])
    kw, params = dict(all_out=(mode == "all_out")), {}
    if mode == "tumor_keys":
        R0 = run_region(oracle_lib, reads)
        kw = dict(tumor_keys=tumor_keys_from(R0.score(all_out=False)))
        R0.close()
        for lib in (oracle_lib, gpu_lib):
            params[lib.prefix] = region.default_params(lib)
            params[lib.prefix].tumor_vcf_is_provided = 1
    Ro, Rg = run_region(oracle_lib, reads, params=params.get(oracle_lib.prefix)), run_region(gpu_lib, reads, params=params.get(gpu_lib.prefix))
    rng = np.random.default_rng(31)
    n = 0
    for what, ranges in range_lists(rng, reads["beg"], reads["end"]):
        ro = concat(singles(Ro, ranges, **kw))
        rg = Rg.score_ranges(ranges, **kw)
        worst = compare_records(ro, rg)
        n += len(ro["refpos"])
        print(name, mode, what, len(ro["refpos"]), {k: v for k, v in worst.items() if v})
    assert n > 100
    Ro.close(); Rg.close()


def test_refusals(gpu_lib):
    reads = synth.generate_region(region_len=1500, depth=40, seed=4)
    R = run_region(gpu_lib, reads)
    beg, end = reads["beg"], reads["end"]
    fn = gpu_lib.dll.uvcgpu_region_score_ranges
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(_ffi.UvcScoreRequest), C.c_void_p, C.c_int64, C.POINTER(_ffi.UvcScoreOut)]
    buf = np.zeros((_ffi.NUM_SCORE_FIELDS, 4096), np.int32)
    out = _ffi.UvcScoreOut(4096, 0, buf.ctypes.data)
    EINVAL = _ffi.ENUMS["UVCGPU_EINVAL"]

    def call(ranges, n=None, **req_kw):
        req, _keep = R.make_request(**req_kw)
        arr, nr = R.make_ranges(ranges)
        rc = fn(R.h, C.byref(req), arr, nr if n is None else n, C.byref(out))
        return rc, gpu_lib.last_error()

    ok = [(beg + 10, beg + 50, 0, 0), (beg + 60, beg + 90, 1, 0)]
    assert call(ok)[0] == 0
    for what, (rc, msg), word in [
        ("pos_beg in the request", call(ok, pos_beg=beg + 10, pos_end=beg + 90), "pos_beg"),
        ("base_at_pos_beg in the request", call(ok, base_at_pos_beg=True), "base_at_pos_beg"),
        ("region_beg in the request", call(ok, region_beg=beg), "region_beg"),
        ("no ranges", call(ok, n=0), "n_ranges"),
        ("overlap", call([(beg + 10, beg + 50, 0, 0), (beg + 49, beg + 90, 0, 0)]), "range 1"),
        ("unsorted", call([(beg + 60, beg + 90, 0, 0), (beg + 10, beg + 50, 0, 0)]), "range 1"),
        ("end in front of begin", call([(beg + 10, beg + 50, 0, 0), (beg + 80, beg + 70, 0, 0)]), "range 1"),
        ("in front of the region", call([(beg - 1, beg + 50, 0, 0)]), "range 0"),
        ("base at the region's begin", call([(beg, beg + 50, 1, 0)]), "range 0"),
        ("behind the region", call([(beg + 10, beg + 50, 0, 0), (beg + 60, beg + 90, 0, 0), (end - 10, end + 5, 0, 0)]), "range 2"),
    ]:
        assert rc == EINVAL and word in msg, (what, rc, msg)
    assert fn(R.h, None, None, 1, C.byref(out)) == EINVAL                  # no ranges array
    # the text call refuses a malformed list too
    rec = R.score_ranges(ok)
    with pytest.raises(region.UvcError, match="range 1"):
        R.vcf_records_ranges("chrR", rec, [(beg + 60, beg + 90, 0, 0), (beg + 10, beg + 50, 0, 0)])
    # a refused call launched nothing and changed nothing: the next good call gives the records again
    assert_same(R.score_ranges(ok), rec, "after the refusals")
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def panel(d):
    """A synthetic BAM over two contigs (the Python writer of test_pipeline) and some twenty short BED lines on them, in file order: sorted,
    some a few bases apart, some far apart, two that abut."""
    refs, recs, seqs = [], [], []
    rng = np.random.default_rng(5)
    for tid, (name, seed) in enumerate((("chrA", 41), ("chrB", 43))):
        reads = synth.generate_region(seed=seed, region_len=6000, depth=60, beg=30000, snv_every=120, somatic_every=400, indel_every=300)
        recs += bamwriter.records_from_reads(reads, tid=tid, qname_fmt=name + "r%d")
        chrom_len = reads["end"] + 5000
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, chrom_len))
        seqs.append((name, seq[:reads["beg"]] + reads["refseq"] + seq[reads["end"]:]))
        refs.append((name, chrom_len))
    bam, fa = os.path.join(d, "p.bam"), os.path.join(d, "p.fa")
    bamwriter.write_bam(bam, refs, recs)
    bamwriter.write_fasta(fa, seqs)
    lines = []
    for name, n in (("chrA", 12), ("chrB", 9)):
        starts = np.sort(rng.choice(np.arange(30300, 35400, 260), n, replace=False))
        for s in starts.tolist():
            lines.append((name, s, s + int(rng.integers(40, 250))))
    lines.insert(5, (lines[4][0], lines[4][2], lines[4][2] + 3))            # abuts its predecessor: opens a batch of its own
    bed = os.path.join(d, "panel.bed")
    with open(bed, "w") as f:
        f.write("# a panel\n" + "".join("%s\t%d\t%d\tamplicon\n" % l for l in lines))
    return bam, fa, bed, lines, [r[0] for r in refs]


def run_cli(bam, fa, out, *extra):
    r = subprocess.run([EXE, bam, "-f", fa, "-o", out, "-s", "S", "-t", "2"] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l for l in gzip.open(out, "rt").read().splitlines() if not l.startswith(("##fileDate=", "##variantCallerCommand="))]


def body(lines):
    return [l for l in lines if not l.startswith("#")]


def test_cli_merge_regions(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, contigs = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    plain = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed)
    assert run_cli(bam, fa, o("zero.vcf.gz"), "-R", bed, "--merge-regions", "0") == plain   # N = 0 is the run without the option, byte for byte
    is_rec = lambda l: "<NON_REF>" not in l and "<ADDITIONAL_INDEL_CANDIDATE>" not in l      # noqa: E731
    key = lambda l: tuple(l.split("\t")[i] for i in (0, 1, 3, 4))          # noqa: E731
    a = {key(l): l.split("\t") for l in body(plain) if is_rec(l)}
    assert len(a) > 30
    for N in (300, 5000):
        merged = run_cli(bam, fa, o("m%d.vcf.gz" % N), "-R", bed, "--merge-regions", str(N), "--bed-out-fname", o("m%d.bed" % N))
        # the Python chain: the same batches, every BED line a single-range call on its batch's region / all lines of a batch in one ranges call
        tid = [contigs.index(c) for c, _, _ in lines]
        pieces = uio.plan_bed_batches(tid, [b for _, b, _ in lines], [e for _, _, e in lines], N, 1000000)
        assert len(pieces) == len(lines) and 1 < len(set(p["batch"] for p in pieces)) < len(lines)   # something was merged, not everything
        for single_ranges in (True, False):
            want = pipeline.call_bed_batches(gpu_lib, bam, fa, pieces, single_ranges=single_ranges)
            assert body(merged) == want.splitlines(), (N, single_ranges)
        # one row per BED line in the region table
        rows = open(o("m%d.bed" % N)).read().splitlines()
        assert [tuple(r.split("\t")[:3]) for r in rows] == [(c, str(b), str(e)) for c, b, e in lines if e > b]
        # against the unmerged run: the same records; depth-like values equal, qualities within one unit (as test_tiles compares
        # tiled and uncut runs)
        b = {key(l): l.split("\t") for l in body(merged) if is_rec(l)}
        assert set(a) == set(b), (N, sorted(set(a) ^ set(b))[:5])
        for k in a:
            fa_, fb_ = dict(zip(a[k][8].split(":"), a[k][9].split(":"))), dict(zip(b[k][8].split(":"), b[k][9].split(":")))
            for tag in ("DP", "AD", "bDP", "bAD"):
                assert fa_[tag] == fb_[tag], (N, k, tag, fa_[tag], fb_[tag])
            for tag in ("cVQ1", "cVQ2"):
                assert all(abs(int(x) - int(y)) <= 1 for x, y in zip(fa_[tag].split(","), fb_[tag].split(","))), (N, k, tag, fa_[tag], fb_[tag])
            assert abs(float(a[k][5]) - float(b[k][5])) <= 1.0, (N, k, a[k][5], b[k][5])
