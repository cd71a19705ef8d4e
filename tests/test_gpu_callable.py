"""Callable-region intervals of ranges of the accumulated planes (uvcgpu_region_callable, Region.callable) and the BED built from them
(uvc1-mi355x --callable-out).  Every number is an integer and is compared for equality: the runs of the HIP library against the numpy
restatement (callable_restatement.py) over the ORACLE's fetched planes, with the inputs, `measures_of` and the range lists of
test_gpu_coverage.py.

What the run counts of these inputs are (counted with the restatement over the oracle's planes).  The depth of a pile of overlapping
reads moves slowly along the reference, so ONE threshold on ONE measure is crossed far less often than every 16 positions, whatever the
threshold: on config2shape_5kb_300x (5 201 positions, npos / 16 = 325) the largest run count over all thresholds is 163 (aDP, at 300), 151
(bDP, 297), 155 (cDP1, 294) and 333 (cDP12, 282); cDP2 and dDP1 are 0 everywhere on this non-UMI input.  At the medians the six measures
together give 478 runs.  So the `at least npos / 16 runs` precondition is asserted where a threshold can reach it -- all six at their medians,
and cDP12 alone at 282, the value chosen from its distribution -- and the other single-measure cases, still compared run by run, assert the
count they can reach: at least 100 runs at the threshold with the most crossings (aDP 300, bDP 297, cDP1 294), which is a flip every 52
positions and puts heads next to wave seams (81 of them) and block seams (5); cDP2 and dDP1 alone are tested at 1, where the all-zero plane
has to set LOW everywhere.  On wide_300kb_8x the request min_depth[aDP] = 8, max_aDP = 9 gives 7 978 runs and no aDP window gives more
than 8 119, so `at least 10 000 runs` is asserted on the six medians of that input (17 388 runs), and the aDP window is compared as well."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import callable_restatement as cr
from test_gpu_coverage import EXE, INPUTS, measures_of, panel, range_lists, run_cli
from test_gpu_parity import CASES
from util import run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

E = _ffi.ENUMS
NCOV = E["UVC_NCOV"]
EINVAL, ENOMEM = E["UVCGPU_EINVAL"], E["UVCGPU_ENOMEM"]
M = region.COVERAGE_MEASURES
_cache = {}


def oracle_measures(name, oracle_lib):
    """(reads, the six measures [NCOV][npos] from the oracle's planes) of an input of test_gpu_coverage.INPUTS or a CASES entry; computed once"""
    if name not in _cache:
        reads = synth.generate_region(**(INPUTS[name] if name in INPUTS else CASES[name]))
        Ro = run_region(oracle_lib, reads)
        m = measures_of(Ro.fetch)
        m.setflags(write=False)
        Ro.close()
        _cache[name] = (reads, m)
    return _cache[name]


def check(Rg, m, ranges, min_depth, max_aDP, what):
    md, mx = cr.request(min_depth, max_aDP)
    want = cr.runs_of(m, Rg.beg, ranges, md, mx)
    got = Rg.callable(ranges, min_depth, max_aDP)
    assert got.dtype == region.CALLABLE_RUN and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]])
    return want


def medians(m):
    return {M[k]: int(np.median(m[k])) for k in range(NCOV)}


def bit(runs, name):
    return (runs["mask"] >> cr.BITS.index(name)) & 1


def test_masks_that_flip_every_few_positions(oracle_lib, gpu_lib):
    """config2shape_5kb_300x, one whole-region range and the range lists: heads at wave seams, at block seams, the left neighbour of lane 0."""
    reads, m = oracle_measures("plain_300x", oracle_lib)
    Rg = run_region(gpu_lib, reads)
    beg, npos = Rg.beg, Rg.npos
    whole = [(beg, beg + npos)]
    med = medians(m)
    print("medians", med)
    assert med == dict(aDP=297, bDP=293, cDP1=291, cDP12=281, cDP2=0, dDP1=0)
    # each measure in turn: the threshold with the most crossings (module docstring), and the count the restatement has to show before the comparison
    # the counted maxima of the docstring, so that a change to the inputs shows up: the most runs any single threshold on one measure gives
    most = {}
    for k, name in enumerate(M):
        counts = {int(t): len(cr.runs_of(m, beg, whole, *cr.request({name: int(t)}))) for t in np.unique(m[k]) if t > 0}
        most[name] = max(counts.items(), key=lambda kv: (kv[1], -kv[0])) if counts else None
    print("most runs by one threshold (threshold, runs):", most, "npos / 16 =", npos // 16)
    assert most == dict(aDP=(300, 163), bDP=(297, 151), cDP1=(294, 155), cDP12=(282, 333), cDP2=None, dDP1=None)
    for name, t, least in (("aDP", 300, 100), ("bDP", 297, 100), ("cDP1", 294, 100), ("cDP12", 282, npos // 16), ("cDP2", 1, 1), ("dDP1", 1, 1)):
        md, mx = cr.request({name: t})
        n = len(cr.runs_of(m, beg, whole, md, mx))
        print(name, t, "runs", n)
        assert n >= least, (name, t, n)
        want = check(Rg, m, whole, {name: t}, 0, name)
        if least == 1:
            assert bit(want, "LOW_" + name).all()
        check(Rg, m, whole, {name: med[name]}, 0, name + " at its median")
    both = cr.runs_of(m, beg, whole, *cr.request(med))
    assert len(both) >= npos // 16, len(both)
    check(Rg, m, whole, med, 0, "all six at their medians")
    check(Rg, m, whole, med, med["aDP"] + 20, "all six and max_aDP")
    rng = np.random.default_rng(17)
    n_lists = 0
    for what, ranges in range_lists(rng, beg, npos):
        for md, mx in ((med, 0), ({}, 0), ({"cDP12": 282}, 310)):
            want = check(Rg, m, ranges, md, mx, what)
            # the runs of a range tile it, in order
            for i, (a, b) in enumerate(ranges):
                r = want[want["range"] == i]
                assert r["pos_beg"][0] == a and r["pos_end"][-1] == b and np.array_equal(r["pos_beg"][1:], r["pos_end"][:-1])
        n_lists += 1
    assert n_lists == 10
    # adjacent ranges with equal masks on both sides of the shared end point still give two runs; single-position ranges give one run each
    shared = [(beg + 503, beg + 570), (beg + 570, beg + 571), (beg + 571, beg + 700)]                   # covered throughout: one mask
    want = check(Rg, m, shared, {}, 0, "shared end points")
    assert len(want) == 3 and len(set(want["mask"].tolist())) == 1
    singles = [(p, p + 1) for p in range(beg + 100, beg + 300)]
    assert np.array_equal(check(Rg, m, singles, med, 0, "singles")["range"], np.arange(200))
    Rg.close()


def test_the_worst_case_every_position_its_own_run(oracle_lib, gpu_lib):
    reads, m = oracle_measures("plain_300x", oracle_lib)
    Rg = run_region(gpu_lib, reads)
    ranges = [(p, p + 1) for p in range(Rg.beg + 1500, Rg.beg + 3500)]
    want = check(Rg, m, ranges, medians(m), 0, "2 000 single-position ranges")
    assert len(want) == 2000
    Rg.close()


@pytest.mark.parametrize("name", ["umi_2kb_400x", "duplex_1kb_2000x"])
def test_consensus_and_duplex_depths_decide_runs(name, oracle_lib, gpu_lib):
    reads, m = oracle_measures(name, oracle_lib)
    Rg = run_region(gpu_lib, reads)
    med = medians(m)
    print(name, "medians", med)
    assert med["cDP2"] > 0 and med["dDP1"] > 0
    whole = [(Rg.beg, Rg.beg + Rg.npos)]
    for k in M:
        check(Rg, m, whole, {k: med[k]}, 0, k)
    want = check(Rg, m, whole, med, 0, "all six")
    for b in ("LOW_cDP2", "LOW_dDP1"):
        assert bit(want, b).any() and not bit(want, b).all(), b
    only = check(Rg, m, whole, {"cDP2": med["cDP2"], "dDP1": med["dDP1"]}, 0, "the two alone")
    assert len(only) > 20
    rng = np.random.default_rng(5)
    for what, ranges in range_lists(rng, Rg.beg, Rg.npos):
        check(Rg, m, ranges, med, med["aDP"], what)
    Rg.close()


def test_long_runs_and_very_many_runs_on_300_kb(oracle_lib, gpu_lib):
    reads, m = oracle_measures("wide_300kb_8x", oracle_lib)
    Rg = run_region(gpu_lib, reads)
    whole = [(Rg.beg, Rg.beg + Rg.npos)]
    want = cr.runs_of(m, Rg.beg, whole, *cr.request({}))
    assert (want["pos_end"] - want["pos_beg"]).max() >= 65536 and len(want) < 100      # many consecutive blocks without a head
    check(Rg, m, whole, {}, 0, "the all-zero request")
    n_window = len(check(Rg, m, whole, {"aDP": 8}, 9, "min_depth[aDP] = 8, max_aDP = 9"))
    windows = {(t, t + w): len(cr.runs_of(m, Rg.beg, whole, *cr.request({"aDP": t}, t + w))) for t in range(4, 14) for w in (0, 1, 2)}
    print("aDP window runs", n_window, "; the most any aDP window gives:", max(windows.items(), key=lambda kv: kv[1]))
    assert n_window == 7978 and max(windows.values()) == 8119          # the counted figures of the docstring
    assert n_window >= 7000
    med = medians(m)
    want = cr.runs_of(m, Rg.beg, whole, *cr.request(med))
    assert len(want) >= 10000, len(want)
    check(Rg, m, whole, med, 0, "the six medians")
    # consistency with uvcgpu_region_coverage on the same handle and ranges: the positions without LOW_k are its GE count
    rng = np.random.default_rng(3)
    lists = dict(range_lists(rng, Rg.beg, Rg.npos))
    for what in ("the whole region", "random 0", "random short"):
        ranges = next(v for k, v in lists.items() if k.startswith(what))
        for t in (1, 7, 8, 12):
            cov = Rg.coverage(ranges, [t])
            for k in range(NCOV):
                runs = Rg.callable(ranges, {M[k]: t}, 0)
                ok = runs[bit(runs, "LOW_" + M[k]) == 0]
                per_range = np.bincount(ok["range"], weights=(ok["pos_end"] - ok["pos_beg"]), minlength=len(ranges)).astype(np.int64)
                assert np.array_equal(per_range, cov[:, k, E["UVC_COV_GE"]]), (what, t, M[k])
    Rg.close()


def raw_fn(lib):
    fn = lib.dll.uvcgpu_region_callable
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return fn


def test_sizes_first(oracle_lib, gpu_lib):
    reads, m = oracle_measures("umi_2kb_400x", oracle_lib)
    Rg = run_region(gpu_lib, reads)
    fn = raw_fn(gpu_lib)
    ranges = [(Rg.beg + 7, Rg.beg + 900), (Rg.beg + 900, Rg.beg + Rg.npos)]
    med = medians(m)
    want = cr.runs_of(m, Rg.beg, ranges, *cr.request(med))
    assert len(want) > 50
    arr = (_ffi.UvcCoverageRange * 2)(*[_ffi.UvcCoverageRange(*q) for q in ranges])
    req = _ffi.UvcCallableRequest()
    for k in range(NCOV):
        req.min_depth[k] = med[M[k]]
    n = C.c_int64(-1)
    assert fn(Rg.h, arr, 2, C.byref(req), None, 0, C.byref(n)) == ENOMEM and n.value == len(want)
    canary = np.full(len(want) + 4, 0x5A5A5A5A, np.int32).repeat(4).reshape(-1, 4)
    buf = canary.copy()
    n.value = -1
    assert fn(Rg.h, arr, 2, C.byref(req), buf.ctypes.data, len(want) - 1, C.byref(n)) == ENOMEM and n.value == len(want)
    assert np.array_equal(buf, canary)
    n.value = -1
    assert fn(Rg.h, arr, 2, C.byref(req), buf.ctypes.data, len(want), C.byref(n)) == 0 and n.value == len(want)
    assert np.array_equal(buf[:len(want)].view(region.CALLABLE_RUN).reshape(-1), want) and np.array_equal(buf[len(want):], canary[len(want):])
    again = canary.copy()
    assert fn(Rg.h, arr, 2, C.byref(req), again.ctypes.data, len(want) + 4, C.byref(n)) == 0
    assert again.tobytes() == buf.tobytes()
    Rg.close()


def test_refusals(oracle_lib, gpu_lib):
    reads = synth.generate_region(**CASES["tiny_600bp_5x"])
    fn = raw_fn(gpu_lib)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, end = R.beg, R.beg + R.npos
    sentinel = -123456789

    def call(ranges, min_depth=(0, 0, 0, 3, 0, 0), max_aDP=0, n=None, cap=None, null=()):
        arr = (_ffi.UvcCoverageRange * max(len(ranges), 1))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])
        req = _ffi.UvcCallableRequest((C.c_int32 * NCOV)(*min_depth), max_aDP)
        out = np.full((R.npos, 4), sentinel, np.int32)
        n_runs = C.c_int64(sentinel)
        rc = fn(R.h, None if "ranges" in null else arr, len(ranges) if n is None else n, None if "req" in null else C.byref(req), None if "runs" in null else out.ctypes.data,
                R.npos if cap is None else cap, None if "n_runs" in null else C.byref(n_runs))
        return rc, (out == sentinel).all() and n_runs.value == sentinel, gpu_lib.last_error()

    ok = [(beg + 5, beg + 100), (beg + 100, beg + 101), (beg + 300, end)]
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "accumulate" in msg and untouched
    R.set_reads(reads)
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "accumulate" in msg and untouched
    R.accumulate()
    Ro = run_region(oracle_lib, reads)
    m = measures_of(Ro.fetch)
    Ro.close()
    want = cr.runs_of(m, beg, ok, [0, 0, 0, 3, 0, 0], 0)
    assert len(want) > 3 and np.array_equal(R.callable(ok, {"cDP12": 3}), want)
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250), (beg + 10, beg + 50)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50), (beg + 49, beg + 60)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50), (beg + 60, beg + 60)]), "range 1"),
        ("reversed", dict(ranges=[(beg + 50, beg + 10)]), "range 0"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20), (end - 3, end + 1)]), "range 1"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null=("ranges",)), "NULL"),
        ("negative min_depth", dict(ranges=ok, min_depth=(0, 0, -1, 0, 0, 0)), "cDP1"),
        ("negative max_aDP", dict(ranges=ok, max_aDP=-5), "max_aDP"),
        ("NULL req", dict(ranges=ok, null=("req",)), "NULL"),
        ("NULL n_runs", dict(ranges=ok, null=("n_runs",)), "NULL"),
        ("negative capacity", dict(ranges=ok, cap=-1), "run_capacity"),
        ("NULL runs with room", dict(ranges=ok, null=("runs",), cap=5), "runs is NULL"),
    ]
    for what, kw, word in bad_calls:
        rc, untouched, msg = call(**kw)
        assert rc == EINVAL and word in msg, (what, rc, msg)
        assert untouched, what
        assert np.array_equal(R.callable(ok, {"cDP12": 3}), want), what      # the handle is as usable as before
    R.score()
    assert np.array_equal(R.callable(ok, {"cDP12": 3}), want)                # a plain score keeps the planes
    R.score(release_state=True)
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "release" in msg and untouched
    R.set_reads(reads)
    R.accumulate()
    assert np.array_equal(R.callable(ok, {"cDP12": 3}), want)
    gen = R.score_stream(4096)
    next(gen)
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "stream" in msg and untouched
    gen.close()
    assert np.array_equal(R.callable(ok, {"cDP12": 3}), want)
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def chain_runs(gpu_lib, bam, fa, chrom, beg, end, min_depth, max_aDP):
    """The runs of [beg, end) of a contig from the Python chain: one region (uvc_amd.pipeline.call_region), the positions it owns through
    Region.callable as one range."""
    res = pipeline.call_region(gpu_lib, bam, fa, chrom, beg, end, keep_handle=True) if end > beg else None
    if res is None:
        return []
    a, b = res["score_range"][0], min(res["score_range"][1], end)
    runs = res["region"].callable([(a, b)], min_depth, max_aDP) if b > a else []
    res["region"].close()
    return [(int(r["pos_beg"]), int(r["pos_end"]), int(r["mask"])) for r in runs]


def test_cli_callable_bed(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    min_depth, max_aDP = {"cDP12": 57, "bDP": 55}, 66          # around the median, the lower quartile and the 90th percentile of the panel's depths (60x)
    opts = ["--callable-min-depth", "cDP12=57,bDP=55", "--callable-max-aDP", "66"]
    # (a) the BED equals the Python chain: each line its own region, its runs through the store of the reader library
    store = uio.Callable(M, cr.request(min_depth)[0], max_aDP, region.CALLABLE_BITS)
    targets, per_target = [], []
    for chrom, b, e, name in lines:
        cb, ce = max(0, b), min(e, clen[chrom])
        t = store.add_target(chrom, cb, max(cb, ce), name)
        runs = chain_runs(gpu_lib, hb, hf, chrom, cb, ce, min_depth, max_aDP)
        if runs:
            arr = np.zeros(len(runs), region.CALLABLE_RUN)
            arr["pos_beg"], arr["pos_end"], arr["mask"] = zip(*runs)
            store.add_runs([t], arr)
        targets.append((chrom, cb, max(cb, ce), name))
        per_target.append(runs)
    store.write(o("chain.bed"))
    store.close()
    want = open(o("chain.bed")).read()
    assert want == cr.report_text(targets, per_target, cr.request(min_depth)[0], max_aDP)
    classes = {l.split("\t")[3] for l in want.splitlines() if not l.startswith("#")}
    assert "CALLABLE" in classes and "EXCESS_aDP" in classes and len(classes) >= 4 and len(want.splitlines()) > 60, classes
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("cov0.tsv"))
    vcf_with = run_cli(bam, fa, o("c.vcf.gz"), "-R", bed, "-t", "2", "--coverage-out", o("cov1.tsv"), "--callable-out", o("c.bed"), *opts)
    got = open(o("c.bed")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100                   # the VCF does not know about the BED
    assert open(o("cov1.tsv")).read() == open(o("cov0.tsv")).read()           # nor does the coverage report
    # (b) the same bytes however the lines are cut and however many workers run, and with the streamed score
    for extra in (["--tile", "1000", "-t", "1"], ["--tile", "7000", "-t", "4"], ["--tile", "1000", "-t", "4"], ["-t", "1"], ["-t", "2", "--score-mem-mb", "16"]):
        vcf = run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "--callable-out", o("t.bed"), *opts, *extra)
        assert open(o("t.bed")).read() == got, extra
        if "--tile" not in extra:
            assert vcf == vcf_without, extra
    # (c) merged regions: compared merged with merged
    vcf_m = run_cli(bam, fa, o("m0.vcf.gz"), "-R", bed, "-t", "2", "--merge-regions", "2000")
    merged = None
    for extra in (["-t", "2"], ["-t", "4", "--score-mem-mb", "16"], ["-t", "1", "--error-profile-out", o("e.tsv"), "--family-stats-out", o("f.tsv")]):
        vcf = run_cli(bam, fa, o("m.vcf.gz"), "-R", bed, "--merge-regions", "2000", "--callable-out", o("m.bed"), *opts, *extra)
        merged = merged or open(o("m.bed")).read()
        assert open(o("m.bed")).read() == merged and vcf == vcf_m, extra
    assert merged.splitlines()[-10] == got.splitlines()[-10]                 # the same positions in all
    # (d) .gz is the same text, block-gzipped; the default request is cDP12=20
    run_cli(bam, fa, o("z.vcf.gz"), "-R", bed, "-t", "2", "--callable-out", o("z.bed.gz"), *opts)
    assert gzip.open(o("z.bed.gz"), "rt").read() == got and open(o("z.bed.gz"), "rb").read()[12:16] == b"BC\x02\x00"
    run_cli(bam, fa, o("d.vcf.gz"), "-R", bed, "-t", "2", "--callable-out", o("d.bed"))
    assert open(o("d.bed")).read().splitlines()[1:3] == ["#min_depth\taDP=0,bDP=0,cDP1=0,cDP12=20,cDP2=0,dDP1=0", "#max_aDP\t0"]
    # (e) without a BED file: one target per called contig span, the lines of a contig tile it
    run_cli(bam, fa, o("w.vcf.gz"), "-t", "2", "--tile", "1700", "--callable-out", o("w.bed"), *opts)
    run_cli(bam, fa, o("w1.vcf.gz"), "-t", "1", "--tile", "1000000", "--callable-out", o("w1.bed"), *opts)
    run_cli(bam, fa, o("w2.vcf.gz"), "-t", "2", "--callable-out", o("w2.bed"), *opts)      # the reference's own region cuts
    w = open(o("w.bed")).read()
    assert w == open(o("w1.bed")).read() == open(o("w2.bed")).read()
    rows = [l.split("\t") for l in w.splitlines() if l[0] != "#"]
    for c in clen:
        mine = [(int(r[1]), int(r[2])) for r in rows if r[0] == c]
        assert mine[0][0] == 0 and mine[-1][1] == clen[c] and all(a[1] == b[0] for a, b in zip(mine, mine[1:])), c
    assert ("#summary\tpositions\t%d" % sum(clen.values())) in w.splitlines()
    # (f) --targets: the target is the called span.  The reference's own cuts begin and end with the reads, which reach over the span's ends:
    # the BED is that of the tiled runs over the span, and its lines tile the span
    tg = ["--targets", "chrA:31501-33200"]
    run_cli(bam, fa, o("g.vcf.gz"), "-t", "2", "--tile", "1000000", "--callable-out", o("g.bed"), *opts, *tg)
    g = open(o("g.bed")).read()
    for n, extra in enumerate((["-t", "2"], ["-t", "1", "--score-mem-mb", "16"], ["-t", "2", "--tile", "700"])):
        run_cli(bam, fa, o("g%d.vcf.gz" % n), "--callable-out", o("g%d.bed" % n), *opts, *tg, *extra)
        assert open(o("g%d.bed" % n)).read() == g, extra
    rows = [l.split("\t") for l in g.splitlines() if l[0] != "#"]
    assert len(rows) > 20 and {r[0] for r in rows} == {"chrA"} and rows[0][1] == "31500" and rows[-1][2] == "33200" and all(a[2] == b[1] for a, b in zip(rows, rows[1:]))
    assert "#summary\tpositions\t1700" in g.splitlines() and not any("NO_COVERAGE" in r[3] for r in rows)
    in_w = [r for r in [l.split("\t") for l in w.splitlines() if l[0] != "#"] if r[0] == "chrA" and int(r[2]) > 31500 and int(r[1]) < 33200]
    assert [(max(int(r[1]), 31500), min(int(r[2]), 33200), r[3]) for r in in_w] == [(int(r[1]), int(r[2]), r[3]) for r in rows]      # the whole-contig BED, clipped
