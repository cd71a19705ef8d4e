"""The alignments behind listed sites from the HIP library (uvcgpu_region_site_reads, Region.site_reads) and the report built from them
(uvc1-mi355x --site-reads-out).  Every number is an integer and is compared for equality:
  * rows and counts against the restatement of the definitions (tests/sitereads_restatement.py) for seven kinds of site list and four
    (min_mapq, alt_only) gates on the four synthetic inputs of the read-profile test, on the hand-made alignments of the CPU test and on
    one synthetic 20 kb read with forty InDels under the dense list of its span;
  * assertions on the restatement's own output that an unwired branch could not meet;
  * sizes first, the corrected qualities after correct_bq, the device-column path, the legality window and the refusals of the ABI;
  * the report of the command line against the Python chain, across --tile, -t, --score-mem-mb and --merge-regions, with the VCF and
    the other reports unchanged."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import sitereads_restatement as sr
import test_sitereads_cpu as cpu
from test_bq_correction import expected_quals
from test_gpu_coverage import panel, run_cli
from test_gpu_device_reads import DeviceColumns
from test_gpu_parity import CASES
from test_gpu_readprofile import INPUTS, long_read, open_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
EINVAL, ENOMEM = _ffi.ENUMS["UVCGPU_EINVAL"], _ffi.ENUMS["UVCGPU_ENOMEM"]
GATES = [(0, 0), (0, 1), (30, 0), (30, 1)]
DENSE_ON = ("tiny_600bp_5x", "umi_duplex_2kb_400x")
TINY_CANNOT = "tiny_600bp_5x"   # its 20 reads hold no N base and no InDel (see test_gpu_readprofile): kinds 4, 5 and the events stay empty


def site_lists(name, rs):
    beg, npos = rs.beg, rs.npos
    rng = np.random.default_rng(23)
    yield "one site", [beg + npos // 2]
    yield "the first and the last position", [beg, beg + npos - 1]
    if name in DENSE_ON:
        yield "every position", np.arange(beg, beg + npos)
    yield "a random 1 %", np.sort(rng.choice(np.arange(beg, beg + npos), max(2, npos // 100), replace=False))
    yield "64 random sites", np.sort(rng.choice(np.arange(beg, beg + npos), 64, replace=False))
    yield "65 consecutive sites", np.arange(beg + 250, beg + 315)
    uncovered = np.setdiff1d(np.arange(beg, beg + npos), rs.obs[:, 1])
    assert len(uncovered) >= 2 and uncovered[-1] == beg + npos - 1
    yield "sites no read covers", uncovered[np.linspace(0, len(uncovered) - 1, 7).astype(int)[[0, 2, 3, 5, 6]]]


def diff(got, want):
    if len(got) != len(want):
        return "lengths %d / %d" % (len(got), len(want))
    return [(int(i), got[i].tolist(), want[i].tolist()) for i in np.flatnonzero(got != want)[:4]]


def check(R, rs, sites, gate, what):
    rows, counts = R.site_reads(sites, *gate)
    w_rows, w_counts = rs.site_reads(sites, *gate)
    assert rows.dtype == region.SITE_READ and counts.dtype == np.int32 and counts.shape == (len(sites), 8)
    assert np.array_equal(counts, w_counts), (what, gate, diff(counts, w_counts))
    assert np.array_equal(rows, w_rows.astype(region.SITE_READ)), (what, gate, diff(rows, w_rows))
    return rows, counts


@pytest.mark.parametrize("name", list(INPUTS))
def test_rows_and_counts_equal_the_restatement(name, gpu_lib):
    reads = synth.generate_region(**INPUTS[name])
    rs = sr.Restatement(reads)
    beg, npos = rs.beg, rs.npos
    # ---- the restatement's own output over every position: every branch is wired and every gate bites
    dense = np.arange(beg, beg + npos)
    w = {g: rs.site_reads(dense, *g) for g in GATES}
    rows, counts = w[(0, 0)]
    print(name, "rows", {g: len(w[g][0]) for g in GATES}, "counts", counts.sum(0).tolist())
    assert (counts.sum(0)[:4] > 0).all()
    if name != TINY_CANNOT:
        assert (counts.sum(0) > 0).all(), "every kind 0..5 and both event columns"
        assert (rows["ins_len"] > 0).any() and (rows["del_len"] > 0).any() and (rows["ins_q"][rows["ins_len"] > 0] > 0).all() and (rows["ins_q"][rows["ins_len"] == 0] == -1).all()
    for mq in (0, 30):
        assert 0 < len(w[(mq, 1)][0]) < len(w[(mq, 0)][0]) and np.array_equal(w[(mq, 1)][1], w[(mq, 0)][1]), "alt_only drops rows and leaves the counts"
    assert len(w[(30, 0)][0]) < len(rows) and (w[(30, 0)][1] <= counts).all() and w[(30, 0)][1].sum() < counts.sum(), "the mapq gate drops rows"
    for k in range(6):
        assert np.array_equal(counts[:, k], np.bincount(rows["site"][(rows["obs"] & 0xFF) == k], minlength=npos))
    assert (rows["obs"] >> 8).max() > 20 and not rows["reserved"].any()
    # ---- the HIP library
    R = open_region(gpu_lib, reads)
    n_lists = 0
    for what, sites in site_lists(name, rs):
        for g in GATES:
            got_rows, got_counts = check(R, rs, sites, g, what)
            if what == "sites no read covers":
                assert len(got_rows) == 0 and not got_counts.any()
        n_lists += 1
    assert n_lists == (7 if name in DENSE_ON else 6)
    R.close()


def test_hand_made_alignments(gpu_lib):
    reads = cpu.hand_made_reads()
    rs, R = sr.Restatement(reads), open_region(gpu_lib, reads)
    B = cpu.BEG
    lists = [np.arange(B, B + cpu.REF_LEN + 1), [B + 14, B + 15], [B + 44, B + 46], [B + 74], [B + 150], [B + 324, B + 325], [B + 339, B + 340], [B + 352, B + 353], [B + 364],
             np.arange(B + 370, B + 377), np.arange(B + 380, B + 390), np.arange(B + 100, B + 340, 3)]
    for sites in lists:
        for g in GATES:
            check(R, rs, sites, g, list(sites)[:3])
    rows, counts = R.site_reads([B + 150, B + 324, B + 339, B + 382], 0, 0)   # inside an N, a dropped anchor, in front of pos, l_qseq 0
    assert len(rows) == 0 and not counts.any()
    R.close()


def test_one_long_read_with_forty_indels_under_the_dense_list(gpu_lib):
    reads = long_read()
    assert reads["l_qseq"][0] > 19000 and reads["n_cigar"][0] == 82
    rs, R = sr.Restatement(reads), open_region(gpu_lib, reads)
    span = rs.obs[rs.obs[:, 0] == 0][:, 1]
    dense = np.arange(span.min(), span.max() + 1)
    for g in ((0, 0), (0, 1)):
        rows, counts = check(R, rs, dense, g, "dense")
    rows, counts = R.site_reads(dense, 0, 0)
    own = rows[rows["read"] == 0]
    assert len(own) == len(dense) > 19000 and (own["ins_len"] > 0).sum() == 20 and (own["del_len"] > 0).sum() == 20 and ((own["obs"] & 0xFF) == 5).sum() == own["del_len"].sum()
    check(R, rs, dense[::7], (0, 1), "every seventh")
    R.close()


def raw_fn(lib):
    fn = lib.dll.uvcgpu_region_site_reads
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return fn


SENTINEL = -123456789


def raw_call(lib, R, sites, gate=(0, 0), capacity=0, n=None, null=()):
    """One call of the ABI with every output filled with a sentinel first -> rc, rows, counts, n_rows, message"""
    sites = np.ascontiguousarray(sites, np.int32)
    req = _ffi.UvcSiteReadsRequest(*gate)
    counts = np.full((max(len(sites), 1), 8), SENTINEL, np.int32)
    rows = np.full((max(abs(capacity), 1), 8), SENTINEL, np.int32)
    n_rows = C.c_int64(SENTINEL)
    rc = raw_fn(lib)(R.h, None if "sites" in null else sites.ctypes.data, len(sites) if n is None else n, None if "req" in null else C.byref(req),
                     None if "counts" in null else counts.ctypes.data, None if "rows" in null else rows.ctypes.data, capacity, None if "n_rows" in null else C.byref(n_rows))
    return rc, rows, counts, n_rows.value, lib.last_error()


def test_sizes_first(gpu_lib):
    reads = synth.generate_region(**INPUTS["umi_duplex_2kb_400x"])
    rs, R = sr.Restatement(reads), open_region(gpu_lib, reads)
    sites = np.arange(rs.beg + 300, rs.beg + 1500)
    for gate in ((0, 0), (0, 1)):
        w_rows, w_counts = rs.site_reads(sites, *gate)
        n = len(w_rows)
        assert n > 256   # more kept rows than one wave step, and than one block's four waves, ranks
        for cap in (0, n - 1):
            rc, rows, counts, n_rows, msg = raw_call(gpu_lib, R, sites, gate, cap)
            assert rc == ENOMEM and n_rows == n and np.array_equal(counts, w_counts) and (rows == SENTINEL).all() and "site_reads" in msg and str(n) in msg, (cap, rc, msg)
        rc, rows, counts, n_rows, msg = raw_call(gpu_lib, R, sites, gate, n)
        assert rc == 0 and n_rows == n and np.array_equal(counts, w_counts)
        assert np.array_equal(rows.view(region.SITE_READ).ravel(), w_rows.astype(region.SITE_READ))
        rc2, rows2, counts2, n2, _ = raw_call(gpu_lib, R, sites, gate, n)   # a second identical call: the same bytes
        assert rc2 == 0 and rows2.tobytes() == rows.tobytes() and counts2.tobytes() == counts.tobytes() and n2 == n
        rc3, rows3, _, n3, _ = raw_call(gpu_lib, R, sites, gate, n + 5)   # more room than rows: the rows, and nothing behind them
        assert rc3 == 0 and n3 == n and np.array_equal(rows3[:n], rows) and (rows3[n:] == SENTINEL).all()
    R.close()


def test_corrected_qualities_columns_window_and_refusals(gpu_lib):
    reads = synth.generate_region(seed=33, region_len=3000, depth=80, clip_frac=0.3, indel_every=400)
    p = region.default_params(gpu_lib)
    p.assay_sequencing_BQ_max, p.assay_sequencing_BQ_inc = 37, 2
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, npos = R.beg, R.npos
    ok = np.arange(beg + 200, beg + 2800, 13)

    def refused(what, word, **kw):
        rc, rows, counts, n_rows, msg = raw_call(gpu_lib, R, **kw)
        assert rc == EINVAL and word in msg and "site_reads" in msg, (what, rc, msg)
        assert (rows == SENTINEL).all() and (counts == SENTINEL).all() and n_rows == SENTINEL, what

    refused("before set_reads", "set_reads", sites=ok)
    assert "has no reads yet" in gpu_lib.last_error()
    R.set_reads(reads)
    before = sr.Restatement(reads)
    want = before.site_reads(ok, 0, 0)
    assert len(want[0]) > 5000
    check(R, before, ok, (0, 0), "before accumulate")
    for what, word, kw in [
        ("NULL sites", "NULL", dict(sites=ok, null=("sites",))), ("NULL req", "NULL", dict(sites=ok, null=("req",))),
        ("NULL counts", "NULL", dict(sites=ok, null=("counts",))), ("NULL n_rows", "NULL", dict(sites=ok, null=("n_rows",))),
        ("no sites", "n_sites", dict(sites=ok, n=0)), ("a negative count", "n_sites", dict(sites=ok, n=-3)),
        ("a site twice", "site 2", dict(sites=[beg + 5, beg + 9, beg + 9, beg + 20])), ("a site below its predecessor", "site 3", dict(sites=[beg + 5, beg + 9, beg + 12, beg + 11])),
        ("in front of the region", "site 0", dict(sites=[beg - 1, beg + 9])), ("behind the region", "site 1", dict(sites=[beg + 5, beg + npos])),
        ("min_mapq -1", "min_mapq", dict(sites=ok, gate=(-1, 0))), ("min_mapq 256", "min_mapq", dict(sites=ok, gate=(256, 0))),
        ("alt_only -1", "alt_only", dict(sites=ok, gate=(0, -1))), ("alt_only 2", "alt_only", dict(sites=ok, gate=(0, 2))),
        ("a negative capacity", "row_capacity", dict(sites=ok, capacity=-1)), ("NULL rows with room", "rows is NULL", dict(sites=ok, capacity=10, null=("rows",))),
    ]:
        refused(what, word, **kw)
        check(R, before, ok, (0, 1), what)   # the handle is as usable as before
    # the region's last position is a legal site
    assert raw_call(gpu_lib, R, [beg + npos - 1], (0, 0), 0)[0] == 0
    # the corrected qualities: the rows of the restatement over them, and not the rows before
    R.correct_bq()
    after = sr.Restatement(reads, quals=expected_quals(reads, 37, 2))
    rows, _ = check(R, after, ok, (0, 0), "after correct_bq")
    assert not np.array_equal(rows["obs"], want[0]["obs"]) and np.array_equal(rows["obs"] & 0xFF, want[0]["obs"] & 0xFF)
    # legal after accumulate, after a plain and a releasing score, while a score stream is open
    R.accumulate()
    check(R, after, ok, (30, 1), "after accumulate")
    R.score()
    check(R, after, ok, (0, 0), "after a score")
    R.score(release_state=True)
    check(R, after, ok, (0, 1), "after a releasing score")
    R.accumulate()
    gen = R.score_stream(4096)
    next(gen)
    check(R, after, ok, (0, 0), "while a score stream is open")
    gen.close()
    # after a reset: refused until the next set_reads; zero reads: zero rows and zero counts
    R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    refused("after a reset", "set_reads", sites=ok)
    none = dict(reads, n_reads=0, n_fams=0)
    for k in ("pos", "mpos", "isize", "flag", "mapq", "nm", "l_qseq", "seq_off", "cigar_off", "n_cigar", "frag_id", "fam_id", "fam_strand", "bases", "quals", "cigars", "fam_dflag"):
        none[k] = reads[k][:0]
    R.set_reads(none)
    rc, rows, counts, n_rows, _ = raw_call(gpu_lib, R, ok, (0, 0), 4)
    assert rc == 0 and n_rows == 0 and not counts.any() and (rows == SENTINEL).all()
    R.close()


def test_set_reads_device_path(gpu_lib):
    reads = synth.generate_region(**CASES["umi_duplex_2kb_400x"])
    cols = DeviceColumns(reads)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads_device((cols.soa, cols))
    rs = sr.Restatement(reads)
    for sites in (np.arange(R.beg + 500, R.beg + 700), [R.beg + 64, R.beg + 127, R.beg + 1500]):
        for g in ((0, 0), (20, 1)):
            check(R, rs, sites, g, "device columns")
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def listed_sites(d, lines, clen):
    """A BED file of sites over the panel: every base of two exons (one of chrA, one of chrB), every 37th position of the span with reads on
    both contigs (inside and outside the BED lines), two bases of the read-less chrC, one in the line beyond the reads and one near the end
    of chrB -> the path and per contig the zero-based positions."""
    exon_a, exon_b = [l for l in lines if l[0] == "chrA"][3], [l for l in lines if l[0] == "chrB"][2]
    bed = [(exon_a[0], exon_a[1], exon_a[2]), (exon_b[0], exon_b[1], exon_b[2])]
    bed += [(c, p, p + 1) for c in ("chrA", "chrB") for p in range(29990, 36100, 37)]
    bed += [("chrC", 150, 152), ("chrB", 38050, 38051), ("chrB", clen["chrB"] - 50, clen["chrB"] - 49)]
    path = os.path.join(d, "sites.bed")
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % q for q in bed))
    per = {}
    for c, b, e in bed:
        per.setdefault(c, set()).update(range(b, e))
    return path, {c: np.array(sorted(v)) for c, v in per.items()}


def chain_report(gpu_lib, hb, hf, lines, clen, per, gate, path):
    """The report of the Python chain: every BED line its own region (uvc_amd.pipeline.call_region), Region.site_reads over the listed sites
    among the positions the region owns, io.SiteReads."""
    with uio.SiteReads(region.SITE_READ_KINDS, region.READ_CLASSES, *gate) as st:
        for tid, (chrom, n) in enumerate(hb.refs):
            if chrom in per:
                st.add(tid, chrom, per[chrom], "".join(hf.fetch(chrom, int(p), int(p) + 1).upper() if p < n else "." for p in per[chrom]))
        n_rows = 0
        for chrom, b, e, _ in lines:
            b, e = max(0, b), min(e, clen[chrom])
            res = pipeline.call_region(gpu_lib, hb, hf, chrom, b, e, keep_handle=True) if e > b else None
            if res is None:
                continue
            a, z = res["score_range"][0], min(res["score_range"][1], e)
            sites = per[chrom][(per[chrom] >= a) & (per[chrom] < z)]
            if len(sites):
                rows, counts = res["region"].site_reads(sites, *gate)
                st.add(hb.tid(chrom), chrom, sites, None, counts, rows, res["reads"], [res["qnames"][int(i)] for i in res["order"]])
                n_rows += len(rows)
            res["region"].close()
        st.write(path)
    return open(path).read(), n_rows


def without_families(text):
    """The lines of the report without what a tile cut can move: the family column of R lines, the families* columns of A lines"""
    out = []
    for l in text.splitlines():
        f = l.split("\t")
        out.append("\t".join(f[:10] + f[11:]) if f[0] == "R" else "\t".join(f[:6]) if f[0] == "A" else l)
    return out


def test_cli_site_reads_report(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, lines, clen = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    hb, hf = uio.Bam(bam), uio.Fasta(fa)
    sites_bed, per = listed_sites(d, lines, clen)
    n_listed = sum(len(v) for v in per.values())
    opts = ["--site-reads-sites", sites_bed, "--site-reads-min-mapq", "10"]
    want, n_rows = chain_report(gpu_lib, hb, hf, lines, clen, per, (10, 1), o("chain.tsv"))
    kinds = [l.split("\t")[0] for l in want.splitlines()]
    assert kinds.count("S") == n_listed and n_rows == kinds.count("R") > 50 and kinds.count("A") > 20
    assert any(l.split("\t")[3].startswith("+") for l in want.splitlines() if l[0] == "A") and any(l.split("\t")[3].startswith("-") for l in want.splitlines() if l[0] == "A")
    assert sum(l.startswith("S\tchrC\t") and l.endswith("\t0" * 9) for l in want.splitlines()) == 2   # listed, owned by nobody: zeros
    others = ["--coverage-out", o("c.tsv"), "--error-profile-out", o("e.tsv"), "--family-stats-out", o("f.tsv"), "--callable-out", o("k.bed"), "--read-profile-out", o("r.tsv"),
              "--msi-out", o("m.tsv"), "--fragment-profile-out", o("g.tsv"), "--force-sites", sites_bed]
    names = ("c.tsv", "e.tsv", "f.tsv", "k.bed", "r.tsv", "m.tsv", "g.tsv")
    vcf_without = run_cli(bam, fa, o("plain.vcf.gz"), "-R", bed, "-t", "2", *others)
    reports = [open(o(n)).read() for n in names]
    vcf_with = run_cli(bam, fa, o("s.vcf.gz"), "-R", bed, "-t", "2", *others, "--site-reads-out", o("s.tsv"), *opts)
    got = open(o("s.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100                  # the VCF and the other seven reports do not see the option
    assert [open(o(n)).read() for n in names] == reports
    # the same bytes however many workers run and however the tiles are scored
    for extra in (["-t", "1"], ["-t", "4"], ["-t", "2", "--score-mem-mb", "16"]):
        run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "--site-reads-out", o("t.tsv"), *opts, *extra)
        assert open(o("t.tsv")).read() == got, extra
    # however the lines are cut: equal without the family columns; with them where no family of the input straddles a cut
    for extra in (["--tile", "1000", "-t", "1"], ["--tile", "7000", "-t", "4"]):
        run_cli(bam, fa, o("t.vcf.gz"), "-R", bed, "--site-reads-out", o("t.tsv"), *opts, *extra)
        cut = open(o("t.tsv")).read()
        assert without_families(cut) == without_families(got), extra
        print(extra, "with the family columns:", "equal" if cut == got else "different")
    # every read, not only the ALT ones: the S lines stay, the R lines grow; true / false as values
    run_cli(bam, fa, o("a.vcf.gz"), "-R", bed, "-t", "2", "--site-reads-out", o("a.tsv"), *opts, "--site-reads-alt-only", "false")
    every = open(o("a.tsv")).read()
    assert [l for l in every.splitlines() if l[0] == "S"] == [l for l in got.splitlines() if l[0] == "S"] and every.count("\nR\t") > 10 * got.count("\nR\t")
    assert every == chain_report(gpu_lib, hb, hf, lines, clen, per, (10, 0), o("chain0.tsv"))[0]
    # merged regions see the reads of the gaps between their lines: compared with itself across -t; .gz is the same text, block-gzipped
    for threads in ("1", "4"):
        run_cli(bam, fa, o("m%s.vcf.gz" % threads), "-R", bed, "-t", threads, "--merge-regions", "2000", "--site-reads-out", o("m%s.tsv.gz" % threads), *opts)
    m1 = gzip.open(o("m1.tsv.gz"), "rt").read()
    assert m1 == gzip.open(o("m4.tsv.gz"), "rt").read() and m1.startswith("##site_reads_min_mapq=10\n##site_reads_alt_only=1\n") and open(o("m1.tsv.gz"), "rb").read()[12:16] == b"BC\x02\x00"
