"""The clip sites of the HIP library (uvcgpu_region_clip_sites, Region.clip_sites) and the report built from them (uvc1-mi355x
--clip-sites-out).  Every number is an integer and is compared for equality:
  * totals, site rows and event rows against the restatement of the definitions (tests/clipsites_restatement.py) for four gates and two
    range lists on the four synthetic inputs of the read-profile test with clip_frac = 0.2, on the hand-made alignments of the CPU test,
    on 1, 255, 256 and 257 alignments (a block of the passes over the alignments takes 256 per step), on the 83-op read of the
    read-profile test and on 3 000 reads clipped at one boundary with one string;
  * assertions on the restatement's own output that an unwired branch could not meet;
  * two calls return the same bytes; sizes first; every refusal by its message; the legality window; the device-column path; zero reads;
  * the report of the command line against the Python chain, across --tile, with the VCF unchanged.
The key list of the sites is searched in global memory (no LDS staging), so there is no site count at which the lookup changes its path."""
import ctypes as C
import os

import numpy as np
import pytest

import clipsites_restatement as cr
import test_clipsites_cpu as cpu
from test_gpu_coverage import panel, run_cli
from test_gpu_device_reads import DeviceColumns
from test_gpu_parity import CASES
from test_gpu_readprofile import INPUTS, long_read, open_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
EINVAL, ENOMEM = _ffi.ENUMS["UVCGPU_EINVAL"], _ffi.ENUMS["UVCGPU_ENOMEM"]
ROW = _ffi.ENUMS["UVC_CLIPSITE_ROW"]
GATES = [(0, 10, 1), (0, 10, 3), (0, 20, 2), (30, 10, 1)]
EXEMPT = "tiny_600bp_5x"   # its 20 reads have sites only at min_reads = 1
_memo = {}


def clipped(name):
    """The input `name` of the read-profile test with clip_frac = 0.2 and its restatement, made once and shared (nobody writes to them)."""
    if name not in _memo:
        reads = synth.generate_region(**dict(INPUTS[name], clip_frac=0.2))
        _memo[name] = (reads, cr.Restatement(reads))
    return _memo[name]


def range_lists(beg, npos):
    yield "the whole region", [(beg, beg + npos)]
    yield "three ranges, one of a single position", [(beg + 50, beg + 200), (beg + 300, beg + 301), (beg + 400, beg + npos - 20)]


def events_of(ev):
    return np.stack([ev[k] for k in region.CLIP_READ.names], axis=1).astype(np.int64).reshape(-1, 4)


def check(R, rs, ranges, gate, what):
    totals, rows, ev = R.clip_sites(ranges, *gate, want_reads=True)
    wt, wr, we = rs.run(ranges, *gate)
    assert totals.dtype == np.int64 and rows.dtype == np.int64 and rows.shape[1:] == (ROW,) and ev.dtype == region.CLIP_READ
    assert totals.tolist() == wt.tolist(), (what, gate, totals.tolist(), wt.tolist())
    assert rows.shape == wr.shape, (what, gate, rows.shape, wr.shape)
    assert np.array_equal(rows, wr), (what, gate, [(int(i), int(j), int(rows[i, j]), int(wr[i, j])) for i, j in np.argwhere(rows != wr)[:6]])
    assert np.array_equal(events_of(ev), we), (what, gate, len(ev), len(we))
    t0, r0, e0 = R.clip_sites(ranges, *gate)                      # without the event rows: the same totals and rows
    assert e0 is None and np.array_equal(t0, totals) and np.array_equal(r0, rows)
    return totals, rows, ev


@pytest.mark.parametrize("name", list(INPUTS))
def test_rows_totals_and_event_rows_equal_the_restatement(name, gpu_lib):
    reads, rs = clipped(name)
    whole = [(rs.beg, rs.beg + rs.npos)]
    # ---- the condition on the inputs, on the restatement's own output
    wt, wr, we = rs.run(whole, 0, 10, 3)
    two = (wr[:, cr.VOTE:].reshape(-1, cr.NCONS, cr.NCODE) > 0).sum(2).max(1) >= 2 if len(wr) else np.zeros(0, bool)
    print(name, "sites at (0, 10, 3):", len(wr), "with two bases at some k:", int(two.sum()), "totals", wt.tolist())
    if name != EXEMPT:
        assert len(wr) >= 10 and two.any()
        assert wr[:, cr.W["len_max"]].max() > 20 and (wr[:, cr.W["spanning"]] > 0).any() and wr[:, cr.W["reads_fwd"]].sum() not in (0, wr[:, cr.W["reads"]].sum())
    assert len(rs.run(whole, 0, 10, 1)[1]) > 0
    assert rs.run(whole, 30, 10, 1)[0][0] < wt[0] and rs.run(whole, 0, 20, 2)[0][3] > 0           # the mapq gate drops alignments, min_clip 20 makes short events
    # ---- the HIP library
    R = open_region(gpu_lib, reads)
    for what, ranges in range_lists(R.beg, R.npos):
        for g in GATES:
            check(R, rs, ranges, g, what)
    a, b = R.clip_sites(whole, 0, 10, 1, True), R.clip_sites(whole, 0, 10, 1, True)   # two calls return the same bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    R.close()


def test_hand_made_alignments(gpu_lib):
    for make in cpu.HAND_MADE:
        reads = make()
        rs, R = cr.Restatement(reads), open_region(gpu_lib, reads)
        for what, ranges in [("whole", cpu.WHOLE), ("three", [(cpu.BEG, cpu.BEG + 1), (cpu.BEG + 120, cpu.BEG + 121), (cpu.BEG + 171, cpu.BEG + cpu.NPOS)])]:
            for g in GATES + [(0, 3, 1), (0, 13, 1), (35, 10, 1), (0, 1, 1)]:
                check(R, rs, ranges, g, (make.__name__, what))
        R.close()


def many_reads(n, distinct):
    """n alignments 20M12S / 12S20M in turn; `distinct` boundaries, so that sites hold one or several events; the clipped bases vary."""
    rng = np.random.default_rng(n)
    specs = []
    for i in range(n):
        off = 10 + (i * 7) % distinct
        clip = list(rng.integers(0, 5, 12))
        specs.append((off, 0x10 if i % 3 == 0 else 0, [(cpu.M, 20), (cpu.S, 12)], [0] * 20 + clip) if i % 2 == 0 else (off + 20, 0, [(cpu.S, 12), (cpu.M, 20)], clip + [0] * 20))
    return cpu.reads_of(specs, mapq=[60 - (i % 40) for i in range(n)])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_alignment_counts_around_a_block_step(n, gpu_lib):
    reads = many_reads(n, 300)
    rs, R = cr.Restatement(reads), open_region(gpu_lib, reads)
    for g in [(0, 10, 1), (0, 10, 2), (30, 10, 1)]:
        totals, rows, ev = check(R, rs, cpu.WHOLE, g, n)
    assert totals[0] == sum(1 for i in range(n) if 60 - (i % 40) >= 30)
    R.close()


def test_the_long_read(gpu_lib):
    reads = long_read()
    assert reads["n_cigar"][0] == 82
    rs, R = cr.Restatement(reads), open_region(gpu_lib, reads)
    whole = [(R.beg, R.beg + R.npos)]
    totals, rows, ev = check(R, rs, whole, (0, 10, 1), "long read")
    assert len(rows) == 1 and rows[0, cr.W["side"]] == 0 and rows[0, cr.W["len_sum"]] == 37 and rows[0, cr.VOTE:].sum() == 32 and rows[0, cr.W["spanning"]] == 0
    check(R, rs, whole, (0, 38, 1), "long read, short clip")
    R.close()


def test_the_hot_row(gpu_lib):
    """3 000 reads clipped at one boundary with one string: one row takes every add."""
    s = [int(v) for v in np.random.default_rng(1).integers(0, 4, 40)]
    reads = cpu.reads_of([(100 + (i % 50), 0x10 if i % 2 else 0, [(cpu.M, 100 - (i % 50)), (cpu.S, 40)], [0] * (100 - (i % 50)) + s) for i in range(3000)])
    rs, R = cr.Restatement(reads), open_region(gpu_lib, reads)
    totals, rows, ev = check(R, rs, cpu.WHOLE, (0, 10, 3), "hot row")
    assert len(rows) == 1 and rows[0, cr.W["reads"]] == 3000 and rows[0, cr.VOTE:].reshape(32, 5).max(1).tolist() == [3000] * 32 and len(ev) == 3000
    assert cr.consensus(rows[0]) == (32, "".join("ACGT"[b] for b in s[:32]))
    R.close()


# ------------------------------------------------------------------------------------------------ the ABI
def raw_fn(lib):
    fn = lib.dll.uvcgpu_region_clip_sites
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return fn


SENTINEL = -123456789


def raw_call(lib, R, ranges, gate=(0, 10, 1), want_reads=1, site_cap=0, read_cap=0, n=None, null=()):
    """One call of the ABI with every output filled with a sentinel first -> rc, totals, rows, n_sites, events, n_reads, message"""
    arr, pairs = region._coverage_ranges(ranges)
    req = _ffi.UvcClipSitesRequest(gate[0], gate[1], gate[2], want_reads)
    totals = np.full(8, SENTINEL, np.int64)
    rows = np.full((max(abs(site_cap), 1), ROW), SENTINEL, np.int64)
    ev = np.full((max(abs(read_cap), 1), 4), SENTINEL, np.int32)
    ns, nr = C.c_int64(SENTINEL), C.c_int64(SENTINEL)
    p = lambda name, v: None if name in null else v                                           # noqa: E731
    rc = raw_fn(lib)(R.h, p("ranges", arr), len(pairs) if n is None else n, p("req", C.byref(req)), p("totals", totals.ctypes.data), p("sites", rows.ctypes.data), site_cap, p("n_sites", C.byref(ns)),
                     p("reads", ev.ctypes.data), read_cap, p("n_reads", C.byref(nr)))
    return rc, totals, rows, ns.value, ev, nr.value, lib.last_error()


def test_sizes_first(gpu_lib):
    reads, rs = clipped("umi_duplex_2kb_400x")
    R = open_region(gpu_lib, reads)
    whole = [(R.beg, R.beg + R.npos)]
    gate = (0, 10, 1)
    wt, wr, we = rs.run(whole, *gate)
    ns, nr = len(wr), len(we)
    assert ns > 256 and nr > ns
    # capacities 0 with NULL arrays; one row short on either array: the sizes and the totals, nothing else
    for kw in (dict(site_cap=0, read_cap=0, null=("sites", "reads")), dict(site_cap=ns - 1, read_cap=nr), dict(site_cap=ns, read_cap=nr - 1), dict(site_cap=0, read_cap=0)):
        rc, totals, rows, n_sites, ev, n_reads, msg = raw_call(gpu_lib, R, whole, gate, **kw)
        assert rc == ENOMEM and n_sites == ns and n_reads == nr and totals.tolist() == wt.tolist() and (rows == SENTINEL).all() and (ev == SENTINEL).all() and "clip_sites" in msg, (kw, rc, msg)
        assert str(ns if kw["site_cap"] < ns else nr) in msg
    # exact room
    rc, totals, rows, n_sites, ev, n_reads, msg = raw_call(gpu_lib, R, whole, gate, site_cap=ns, read_cap=nr)
    assert rc == 0 and n_sites == ns and n_reads == nr and totals.tolist() == wt.tolist() and np.array_equal(rows, wr) and np.array_equal(ev, we)
    rc2, t2, rows2, _, ev2, _, _ = raw_call(gpu_lib, R, whole, gate, site_cap=ns, read_cap=nr)   # a second identical call: the same bytes
    assert rc2 == 0 and rows2.tobytes() == rows.tobytes() and ev2.tobytes() == ev.tobytes() and t2.tobytes() == totals.tobytes()
    # more room than rows: the rows, and nothing behind them
    rc, _, rows3, n3, ev3, r3, _ = raw_call(gpu_lib, R, whole, gate, site_cap=ns + 3, read_cap=nr + 5)
    assert rc == 0 and n3 == ns and r3 == nr and np.array_equal(rows3[:ns], wr) and (rows3[ns:] == SENTINEL).all() and np.array_equal(ev3[:nr], we) and (ev3[nr:] == SENTINEL).all()
    # want_reads = 0 with no room for reads: the rows, *n_reads, no event row
    for kw in (dict(read_cap=0, null=("reads",)), dict(read_cap=2)):
        rc, totals, rows, n_sites, ev, n_reads, msg = raw_call(gpu_lib, R, whole, gate, want_reads=0, site_cap=ns, **kw)
        assert rc == 0 and n_sites == ns and n_reads == nr and np.array_equal(rows, wr) and (ev == SENTINEL).all(), (kw, rc, msg)
    R.close()


def test_refusals_window_device_columns_and_zero_reads(gpu_lib):
    reads = synth.generate_region(seed=33, region_len=3000, depth=80, clip_frac=0.3, indel_every=400)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, npos = R.beg, R.npos
    ok = [(beg + 100, beg + 1500), (beg + 1600, beg + npos)]
    rs = cr.Restatement(reads)

    def refused(what, word, **kw):
        rc, totals, rows, n_sites, ev, n_reads, msg = raw_call(gpu_lib, R, **kw)
        assert rc == EINVAL and word in msg and "clip_sites" in msg, (what, rc, msg)
        assert (totals == SENTINEL).all() and (rows == SENTINEL).all() and (ev == SENTINEL).all() and n_sites == SENTINEL and n_reads == SENTINEL, what

    refused("before set_reads", "set_reads", ranges=ok)
    assert "has no reads yet" in gpu_lib.last_error()
    R.set_reads(reads)
    assert len(rs.run(ok, 0, 10, 1)[1]) > 100
    check(R, rs, ok, (0, 10, 1), "before accumulate")
    for what, word, kw in [
        ("NULL ranges", "NULL", dict(ranges=ok, null=("ranges",))), ("NULL req", "NULL", dict(ranges=ok, null=("req",))), ("NULL totals", "NULL", dict(ranges=ok, null=("totals",))),
        ("NULL n_sites", "NULL", dict(ranges=ok, null=("n_sites",))), ("NULL n_reads", "NULL", dict(ranges=ok, null=("n_reads",))),
        ("no ranges", "n_ranges", dict(ranges=ok, n=0)), ("a negative count", "n_ranges", dict(ranges=ok, n=-2)),
        ("an empty range", "range 1", dict(ranges=[(beg, beg + 5), (beg + 9, beg + 9)])), ("a reversed range", "range 0", dict(ranges=[(beg + 9, beg + 5)])),
        ("in front of the region", "range 0", dict(ranges=[(beg - 1, beg + 5)])), ("behind the region", "range 1", dict(ranges=[(beg, beg + 5), (beg + 9, beg + npos + 1)])),
        ("overlapping ranges", "range 1", dict(ranges=[(beg, beg + 50), (beg + 49, beg + 60)])), ("unsorted ranges", "range 1", dict(ranges=[(beg + 100, beg + 150), (beg + 10, beg + 20)])),
        ("min_mapq -1", "min_mapq", dict(ranges=ok, gate=(-1, 10, 1))), ("min_mapq 256", "min_mapq", dict(ranges=ok, gate=(256, 10, 1))),
        ("min_clip 0", "min_clip", dict(ranges=ok, gate=(0, 0, 1))), ("min_reads 0", "min_reads", dict(ranges=ok, gate=(0, 10, 0))),
        ("want_reads -1", "want_reads", dict(ranges=ok, want_reads=-1)), ("want_reads 2", "want_reads", dict(ranges=ok, want_reads=2)),
        ("a negative site capacity", "site_capacity", dict(ranges=ok, site_cap=-1)), ("a negative read capacity", "read_capacity", dict(ranges=ok, read_cap=-1)),
        ("NULL sites with room", "sites is NULL", dict(ranges=ok, site_cap=10, null=("sites",))), ("NULL reads with room", "reads is NULL", dict(ranges=ok, read_cap=10, null=("reads",))),
    ]:
        refused(what, word, **kw)
    check(R, rs, ok, (0, 10, 2), "after the refusals")   # the handle is as usable as before
    # legal after accumulate, after a score with released planes, while a score stream is open
    R.accumulate()
    check(R, rs, ok, (30, 10, 1), "after accumulate")
    R.score(release_state=True)
    check(R, rs, ok, (0, 10, 1), "after a releasing score")
    R.accumulate()
    gen = R.score_stream(4096)
    next(gen)
    check(R, rs, ok, (0, 20, 2), "while a score stream is open")
    gen.close()
    # after a reset: refused until the next set_reads; zero reads: zero sites
    R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    refused("after a reset", "set_reads", ranges=ok)
    none = dict(reads, n_reads=0, n_fams=0)
    for k in ("pos", "mpos", "isize", "flag", "mapq", "nm", "l_qseq", "seq_off", "cigar_off", "n_cigar", "frag_id", "fam_id", "fam_strand", "bases", "quals", "cigars", "fam_dflag"):
        none[k] = reads[k][:0]
    R.set_reads(none)
    rc, totals, rows, n_sites, ev, n_reads, _ = raw_call(gpu_lib, R, ok, site_cap=4, read_cap=4)
    assert rc == 0 and n_sites == 0 and n_reads == 0 and not totals.any() and (rows == SENTINEL).all() and (ev == SENTINEL).all()
    R.close()


def test_set_reads_device_path(gpu_lib):
    reads = synth.generate_region(**dict(CASES["umi_duplex_2kb_400x"], clip_frac=0.2))
    cols = DeviceColumns(reads)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads_device((cols.soa, cols))
    rs = cr.Restatement(reads)
    host = open_region(gpu_lib, reads)
    for what, ranges in range_lists(R.beg, R.npos):
        for g in ((0, 10, 1), (20, 10, 2)):
            got = check(R, rs, ranges, g, "device columns")
            want = host.clip_sites(ranges, *g, want_reads=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    host.close()
    R.close()


# ------------------------------------------------------------------------------------------------ command line
GATE = (10, 10, 2)
OPTS = ["--clip-sites-min-mapq", "10", "--clip-sites-min-clip", "10", "--clip-sites-min-reads", "2"]


def clipped_panel(d, monkeypatch):
    """The panel of the coverage test with a quarter of its reads clipped by the generator."""
    gen = synth.generate_region
    monkeypatch.setattr(synth, "generate_region", lambda **kw: gen(**dict(kw, clip_frac=0.25)))
    try:
        return panel(d)
    finally:
        monkeypatch.undo()


def chain_report(gpu_lib, hb, hf, lines, clen, with_reads, path):
    """The report of the Python chain: every BED line its own region (uvc_amd.pipeline.call_region), Region.clip_sites over the positions the
    region owns, io.ClipSites."""
    n_sites = 0
    with uio.ClipSites(*GATE, with_reads) as st:
        for chrom, b, e, _ in lines:
            b, e = max(0, b), min(e, clen[chrom])
            res = pipeline.call_region(gpu_lib, hb, hf, chrom, b, e, keep_handle=True) if e > b else None
            if res is None:
                continue
            a, z = res["score_range"][0], min(res["score_range"][1], e)
            if z > a:
                totals, rows, ev = res["region"].clip_sites([(a, z)], *GATE, want_reads=True)
                st.add(hb.tid(chrom), chrom, rows, ev, res["reads"], [res["qnames"][int(i)] for i in res["order"]])
                n_sites += len(rows)
            res["region"].close()
        st.write(path)
    return open(path).read(), n_sites


def without_families(text):
    """The lines of the report without what a tile cut can move: the three family columns of S lines, the family rank of R lines and, with
    it, the order of the R lines of a site."""
    out, rl = [], []
    for l in text.splitlines() + ["#end"]:
        f = l.split("\t")
        if f[0] == "R":
            rl.append("\t".join(f[:9] + f[10:]))
            continue
        out += sorted(rl)
        rl = []
        out.append("\t".join(f[:13] + f[16:]) if f[0] == "S" else l)
    return out


def test_cli_clip_sites_report(tmp_path, gpu_lib, monkeypatch):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = clipped_panel(d, monkeypatch)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    want, n_sites = chain_report(gpu_lib, hb, hf, lines, clen, 1, o("chain.tsv"))
    kinds = [l.split("\t")[0] for l in want.splitlines()]
    print("sites of the chain:", n_sites, "R lines:", kinds.count("R"))
    assert n_sites >= kinds.count("S") >= 10 and kinds.count("R") >= 2 * kinds.count("S")   # (the long line of chrB overlaps its exons: their sites are reported twice and written once)
    assert {l.split("\t")[3] for l in want.splitlines() if l[0] == "S"} == {"L", "R"} and any(l.split("\t")[-1] not in (".", l.split("\t")[-1].upper()) for l in want.splitlines() if l[0] == "S")
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2")
    vcf_with = run_cli(bam, fa, o("s.vcf.gz"), "-R", bed, "-t", "2", "--clip-sites-out", o("s.tsv"), *OPTS, "--clip-sites-reads", "1")
    got = open(o("s.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100                  # the VCF is byte-identical to the run without the option
    # the S lines alone without --clip-sites-reads
    run_cli(bam, fa, o("n.vcf.gz"), "-R", bed, "-t", "4", "--clip-sites-out", o("n.tsv"), *OPTS)
    assert open(o("n.tsv")).read() == chain_report(gpu_lib, hb, hf, lines, clen, 0, o("chain0.tsv"))[0]
    assert [l for l in open(o("n.tsv")).read().splitlines() if l[0] == "S"] == [l for l in got.splitlines() if l[0] == "S"] and "\nR\t" not in open(o("n.tsv")).read()
    # however the contigs are cut: --tile 1000, --tile 7000 and no --tile are equal with the family columns left out
    cuts = []
    for extra in (["--tile", "1000", "-t", "1"], ["--tile", "7000", "-t", "4"], ["-t", "2"]):
        run_cli(bam, fa, o("t.vcf.gz"), "--clip-sites-out", o("t.tsv"), *OPTS, "--clip-sites-reads", "1", *extra)
        cuts.append(open(o("t.tsv")).read())
        print(extra, "S lines:", cuts[-1].count("\nS\t"), "with the family columns:", "equal" if cuts[-1] == cuts[0] else "different")
    assert cuts[0].count("\nS\t") > kinds.count("S")
    assert without_families(cuts[0]) == without_families(cuts[1]) == without_families(cuts[2])
