"""A score in bounded memory (uvcgpu_region_score_stream_begin / uvcgpu_score_stream_next / uvcgpu_score_stream_end): the chunks of a stream,
one after another, are the records of the one call -- every int32 field equal, germ_ref / germ_alt1 / germ_alt2 pointing at the same
(refpos, symbol) -- on the inputs of test_gpu_score_ranges crossed with the gates (default, -A, kept_only, force-output sites, tumor keys,
a ranges request), at chunk sizes that give at least four chunks; the chunks are whole positions, at most chunk_records records each, and
the ranges they report are consecutive, disjoint and add up to the request; the chunk texts concatenate to the one call's text with cuts
off the MGVCF block boundaries; the stated footprint bound holds and does not move from chunk to chunk; the handle refuses what cannot go
with an open stream and scores as before after it.  The same stream agrees with the oracle called once in the suite's tolerance classes.
uvc1-mi355x --score-mem-mb writes the files of the run without it, byte for byte."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_cli_params import resolved
from test_gpu_parity import CASES, compare_records, tumor_keys_from
from test_gpu_score_ranges import INPUTS, concat, panel, reads_of
from test_pipeline import make_files, make_tn_files
from util import run_region
from uvc_amd import _ffi, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
INDEX_FIELDS = ("germ_ref", "germ_alt1", "germ_alt2")
FOOTPRINT_CONST = 256 << 10          # include/uvcgpu.h: footprint <= chunk_records * bytes_per_record + 96 * positions + 3/2 staged arrays + 256 KiB
MIN_CHUNKS = 4


def zpos_of(rec):
    """zerobased_pos of every record: refpos of a LINK record, refpos + 1 of a BASE record (symbols 0..5)."""
    return rec["refpos"].astype(np.int64) + (rec["symbol"] <= 5)


def chunk_size(full):
    """A chunk size that cuts the records `full` (all records of the gated groups: what chunk_records counts) into at least MIN_CHUNKS + 1
    chunks -- a chunk is never fuller than chunk_records -- but not below what the fullest position needs."""
    n_all = len(full["refpos"])
    fullest = int(np.bincount(zpos_of(full) - int(zpos_of(full).min())).max()) if n_all else 1
    return max(n_all // (MIN_CHUNKS + 1), fullest)


def check_stream(R, want, full, request, ranges=None, c=None, **mode):
    """Runs the stream for `mode`, checks the chunk contract and returns the chunks.  `want`: the one call's records; `full`: all records of
    the gated groups (what chunk_records counts; = want unless kept_only); `request`: the (pos_beg, pos_end, base_at_pos_beg, region_beg) ranges the stream must cover."""
    n_all = len(full["refpos"])
    c = chunk_size(full) if c is None else c
    chunks = list(R.score_stream(c, ranges=ranges, **mode))
    sizes = [len(q[0]["refpos"]) for q in chunks]
    print(sorted(mode), "records", len(want["refpos"]), "of", n_all, "chunk_records", c, "chunks", len(chunks), "sizes", sizes[:8])
    assert len(chunks) >= MIN_CHUNKS, (sorted(mode), len(chunks), n_all, c)      # a one-chunk run must not pass silently
    assert max(sizes) <= c
    # covered: consecutive, disjoint, their union the request; a piece that continues a range says so and carries region_beg
    flat = [q for _, cov in chunks for q in cov]
    assert all(len(cov) >= 1 for _, cov in chunks)
    assert all(b[0] >= a[1] for a, b in zip(flat, flat[1:])), flat
    want_pos = np.concatenate([np.arange(a, b) for a, b, _, _ in request])
    assert np.array_equal(np.concatenate([np.arange(a, b) for a, b, _, _ in flat]), want_pos)
    begins = {a: (cb, d) for a, b, cb, d in request if b > a}
    for a, b, cb, d in flat:
        if a in begins:
            assert (cb, d) == begins[a], (a, cb, d, begins[a])
        else:
            assert cb == 1, (a, b, cb)
        assert d == next(dd for aa, bb, _, dd in request if aa <= a < bb)
    # no cut inside a position: the records of a chunk lie in its covered ranges (which are disjoint from every other chunk's)
    for rec, cov in chunks:
        z = zpos_of(rec)
        inside = np.zeros(len(z), bool)
        for a, b, _, _ in cov:
            inside |= (z >= a) & (z < b)
        assert inside.all(), (cov, z[~inside][:5])
    # the chunks, one after another, are the one call
    got = concat([q[0] for q in chunks])
    assert len(got["refpos"]) == len(want["refpos"]), (len(got["refpos"]), len(want["refpos"]))
    bad = [f for f in want if not np.array_equal(got[f], want[f])]
    assert not bad, (sorted(mode), bad[:6], [(int(np.argmax(got[f] != want[f])), int(got[f][np.argmax(got[f] != want[f])]), int(want[f][np.argmax(got[f] != want[f])])) for f in bad[:3]])
    # germ_*: chunk-relative indices, de-referenced inside their chunk, name the (refpos, symbol) the one call's index names
    at = 0
    for rec, _ in chunks:
        n = len(rec["refpos"])
        for f in INDEX_FIELDS:
            v, w = rec[f], want[f][at:at + n]
            assert ((v >= 0) == (w >= 0)).all() and (v < n).all()
            m = v >= 0
            assert np.array_equal(rec["refpos"][v[m]], want["refpos"][w[m]]) and np.array_equal(rec["symbol"][v[m]], want["symbol"][w[m]]), f
        at += n
    return chunks


@pytest.mark.parametrize("name", list(INPUTS))
def test_stream_equals_the_one_call(name, gpu_lib):
    reads = reads_of(name)
    R = run_region(gpu_lib, reads)
    beg, end = reads["beg"], reads["end"]
    lo, hi = beg + 1, end - 1
    rng = np.random.default_rng(len(name))
    sites = np.unique(rng.integers(lo, hi, 150))
    plain = [(beg + 1, end, 0, 0)]                                          # the default request: the whole region core
    for mode in (dict(), dict(all_out=True), dict(kept_only=True), dict(all_out=True, kept_only=True), dict(force_sites=sites), dict(force_sites=sites, kept_only=True)):
        full = R.score(**{k: v for k, v in mode.items() if k != "kept_only"})
        check_stream(R, R.score(**mode), full, plain, **mode)
    # a request of its own: not the whole core, with the base of its first position and a BED line's begin
    sub = dict(pos_beg=lo + 37, pos_end=hi - 41, base_at_pos_beg=True, region_beg=lo + 5)
    full = R.score(all_out=True, **sub)
    check_stream(R, full, full, [(lo + 37, hi - 41, 1, lo + 5)], all_out=True, **sub)
    # a ranges request: ranges that touch, a gap, an empty range, a one-position range
    mid = (lo + hi) // 2
    rg = [(lo + 10, mid - 300, 0, lo + 10), (mid - 300, mid, 1, lo + 10), (mid + 50, mid + 50, 0, 0), (mid + 60, mid + 61, 1, 0), (mid + 200, hi - 5, 0, mid + 200)]
    for mode in (dict(all_out=True), dict(), dict(all_out=True, kept_only=True), dict(force_sites=sites)):
        full = R.score_ranges(rg, **{k: v for k, v in mode.items() if k != "kept_only"})
        check_stream(R, R.score_ranges(rg, **mode), full, rg, ranges=rg, **mode)
    # the caller's InDel alleles
    full = R.score(all_out=True)
    indel = np.nonzero(np.isin(full["symbol"], (7, 8, 9, 10, 11, 12)) & (full["bDPa"] > 0))[0][::3]
    alleles = sorted(set((int(full["refpos"][i]), int(full["symbol"][i]), 7, 5, 1 + i % 3) for i in indel))
    if alleles:
        want = R.score(all_out=True, indel_alleles=alleles)
        check_stream(R, want, want, plain, all_out=True, indel_alleles=alleles)
    R.close()


@pytest.mark.parametrize("name", ["plain_300x", "umi_duplex"])
def test_stream_with_tumor_keys(name, gpu_lib):
    reads = reads_of(name)
    R0 = run_region(gpu_lib, reads)
    keys = tumor_keys_from(R0.score(all_out=False))
    R0.close()
    p = region.default_params(gpu_lib)
    p.tumor_vcf_is_provided = 1
    R = run_region(gpu_lib, reads, params=p)
    lo, hi = reads["beg"] + 1, reads["end"]
    want = R.score(tumor_keys=keys)
    assert (want["tkey"] >= 0).sum() > 20
    chunks = check_stream(R, want, want, [(lo, hi, 0, 0)], tumor_keys=keys)
    cols = ["0/1:%d" % i for i in range(len(keys))]
    ras = ["A\tAC" if k[1] in (10, 11, 12) else "AC\tA" if k[1] in (7, 8, 9) else "A\tC" for k in keys]
    text = "".join(R.vcf_records_ranges("chrT", rec, cov, tumor_keys=keys, tumor_sample_columns=cols, tumor_ref_alt=ras) for rec, cov in chunks)
    assert text == R.vcf_records("chrT", want, tumor_keys=keys, tumor_sample_columns=cols, tumor_ref_alt=ras)
    kept = R.score(tumor_keys=keys, kept_only=True)
    check_stream(R, kept, want, [(lo, hi, 0, 0)], tumor_keys=keys, kept_only=True)
    R.close()


def test_stream_against_the_oracle_called_once(oracle_lib, gpu_lib):
    """The comparison of test_ranges_records_match_the_oracle_called_once_per_range (compare_records of test_gpu_parity: depth / count fields
    exact, Phred-like within 1, x100 within 1 %), the oracle called ONCE, the stream's chunks joined."""
    reads = synth.generate_region(**CASES["config2shape_5kb_300x"])
    Ro, Rg = run_region(oracle_lib, reads), run_region(gpu_lib, reads)
    ro = Ro.score(all_out=True)
    chunks = list(Rg.score_stream(chunk_size(ro), all_out=True))
    assert len(chunks) >= MIN_CHUNKS
    rg = concat([q[0] for q in chunks])
    worst = compare_records(ro, rg)
    print(len(ro["refpos"]), len(chunks), {k: v for k, v in worst.items() if v})
    assert len(ro["refpos"]) > 1000
    Ro.close(); Rg.close()


def test_footprint(gpu_lib):
    reads = reads_of("plain_300x")
    R = run_region(gpu_lib, reads)
    bpr = R.score_stream_bytes_per_record()
    npos = reads["end"] - reads["beg"] + 1
    assert bpr >= 2 * 640
    full = R.score(all_out=True, kept_only=True)                            # a one-call score first: its record-sized buffers must not stay under a stream
    one_call = R.score_stream_footprint()
    c0 = chunk_size(R.score(all_out=True))
    for c in (c0, c0 // 3, c0):
        bound = c * bpr + 96 * npos + FOOTPRINT_CONST
        seen = []
        for rec, cov in R.score_stream(c, all_out=True, kept_only=True):
            seen.append(R.score_stream_footprint())
        print("chunk_records", c, "chunks", len(seen), "footprint", seen[0], "bound", bound, "one call", one_call, "bytes per record", bpr)
        assert len(seen) >= MIN_CHUNKS
        assert len(set(seen)) == 1, seen                                    # nothing is allocated per chunk
        assert 0 < seen[0] <= bound, (seen[0], bound)
        assert seen[0] < one_call                                           # (the one call holds rows for every record of the request)
        again = [R.score_stream_footprint() for _ in R.score_stream(c, all_out=True, kept_only=True)]
        assert again == seen                                                # kept across streams with the same chunk_records
    assert len(full["refpos"]) > 0
    R.close()


def test_text_concatenates_with_cuts_off_the_block_boundaries(gpu_lib):
    """MGVCF blocks open at multiples of 1000 and at region_beg, never at a range's begin: the chunk texts, each written from (chunk, covered),
    are the one call's text although no cut falls on a multiple of 1000.  outvar_flag has the MGVCF and the ADDITIONAL_INDEL_CANDIDATE lines
    on; this input writes block lines in every mode and, measured, no candidate line (no long repeat track, no clipped reads): the count
    is printed, not asserted."""
    name = "plain_300x"
    reads = reads_of(name)
    p = region.default_params(gpu_lib)
    p.outvar_flag |= 0x18                                                   # OUTVAR_MGVCF and ADDITIONAL_INDEL_CANDIDATE lines (the default has them; said here)
    R = run_region(gpu_lib, reads, params=p)
    lo, hi = reads["beg"] + 1, reads["end"] - 1
    n_text = n_cand = n_block = 0
    for mode, req in ((dict(), dict()), (dict(all_out=True), dict()), (dict(force_sites=list(range(lo + 3, hi, 97))), dict()),
                      (dict(all_out=True), dict(pos_beg=lo + 450, pos_end=hi - 300, base_at_pos_beg=True, region_beg=lo + 450))):
        want = R.score(**mode, **req)
        text = R.vcf_records("chrS", want, **req)
        n_block += text.count("<NON_REF>")
        n_cand += text.count("<ADDITIONAL_INDEL_CANDIDATE>")
        done = False
        for c in [chunk_size(want) + k for k in (0, 7, 13, 29, 57)]:
            chunks = list(R.score_stream(c, **mode, **req))
            cuts = [cov[0][0] for _, cov in chunks[1:]]
            if len(chunks) < MIN_CHUNKS or any(z % 1000 == 0 for z in cuts):
                continue
            got = "".join(R.vcf_records_ranges("chrS", rec, cov) for rec, cov in chunks)
            assert got == text, (sorted(mode), c, cuts)
            done = True
            n_text += len(got)
            break
        assert done, sorted(mode)
    print(name, "text bytes", n_text, "block lines", n_block, "candidate lines", n_cand)
    assert n_text > 0 and n_block > 0
    R.close()


def test_state(gpu_lib):
    reads = reads_of("plain_300x")
    R = run_region(gpu_lib, reads)
    E = _ffi.ENUMS
    before = R.score(all_out=True)
    c = chunk_size(before)
    g = R.score_stream(c, all_out=True)
    first = next(g)
    for what, call in (("score", lambda: R.score()), ("score_ranges", lambda: R.score_ranges([(reads["beg"] + 5, reads["beg"] + 50)])), ("accumulate", R.accumulate),
                       ("reset", lambda: R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])), ("set_reads", lambda: R.set_reads(reads)),
                       ("a second stream", lambda: next(R.score_stream(c)))):
        with pytest.raises(region.UvcError) as ei:
            call()
        assert ei.value.code == E["UVCGPU_ESTATE"] and "stream" in str(ei.value), (what, ei.value)
    planes = R.fetch("FRAG")                                                # reading the planes is no business of the stream
    second = next(g)
    assert len(first[0]["refpos"]) > 0 and second[1][0][0] == first[1][-1][1]
    g.close()                                                               # end mid-way
    after = R.score(all_out=True)
    assert all(np.array_equal(after[f], before[f]) for f in before)
    assert all(np.array_equal(R.score(kept_only=True)[f], v) for f, v in R.score(kept_only=True).items())
    assert np.array_equal(R.fetch("FRAG"), planes)
    # a position that alone is more than a chunk: refused with its name, nothing opened, the handle as before
    with pytest.raises(region.UvcError) as ei:
        next(R.score_stream(8, all_out=True))
    assert ei.value.code == E["UVCGPU_ENOMEM"], ei.value
    m = re.search(r"zerobased_pos (\d+) alone has (\d+) records", str(ei.value))
    assert m and reads["beg"] < int(m.group(1)) < reads["end"] and int(m.group(2)) > 8, ei.value
    assert int(m.group(2)) == int((zpos_of(before) == int(m.group(1))).sum())
    assert all(np.array_equal(R.score(all_out=True)[f], before[f]) for f in before)
    # chunk_records as small as the fullest position needs: still the one call (no artificial minimum)
    need = int(np.bincount(zpos_of(before) - reads["beg"]).max())
    tiny = concat([q[0] for q in R.score_stream(need, all_out=True, pos_beg=reads["beg"] + 100, pos_end=reads["beg"] + 160)])
    want = R.score(all_out=True, pos_beg=reads["beg"] + 100, pos_end=reads["beg"] + 160)
    assert all(np.array_equal(tiny[f], want[f]) for f in want)
    # release_state: the planes stay while chunks are outstanding and go behind the last chunk's kernels
    g = R.score_stream(c, all_out=True, release_state=True)
    parts = [next(g)[0]]
    assert np.array_equal(R.fetch("FRAG"), planes)                          # at least four chunks: the last one is not queued yet
    parts += [q[0] for q in g]
    got = concat(parts)
    assert all(np.array_equal(got[f], before[f]) for f in before)
    with pytest.raises(region.UvcError) as ei:
        R.score()
    assert ei.value.code == E["UVCGPU_ESTATE"] and "released" in str(ei.value)
    with pytest.raises(region.UvcError):
        R.fetch("FRAG")
    R.accumulate()
    again = R.score(all_out=True)
    assert all(np.array_equal(again[f], before[f]) for f in before)
    # ended before the last chunk was queued: the planes are kept
    g = R.score_stream(c, all_out=True, release_state=True)
    next(g); g.close()
    assert all(np.array_equal(R.score(all_out=True)[f], before[f]) for f in before)
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def cli(args, timeout=600):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def payload(path):
    """Everything of a VCF but the two header lines that state the time and the command line of the run."""
    return [l for l in gzip.open(path, "rt").read().splitlines() if not l.startswith(("##fileDate=", "##variantCallerCommand="))]


def chunks_per_tile(stderr, which=None):
    m = re.findall(r"--score-mem-mb \d+(?:, (tumor|normal))?: (?:\d+ records per chunk, )?(\d+) chunks in (\d+) scored tiles", stderr)
    assert m, stderr[-2000:]
    return {k or "all": int(a) / max(int(b), 1) for k, a, b in m}[which or "all"]


MB = 1          # the smallest budget the option takes: about 170 records per chunk, dozens of chunks per 2 kb -A tile


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("scorestream")
    reads = make_files(d, 1)
    b0, b1 = reads["beg"], reads["beg"] + 6000
    return dict(d=d, bam=str(d / "u1.bam"), fa=str(d / "u1.fa"), b0=b0, b1=b1, common=[str(d / "u1.bam"), "-f", str(d / "u1.fa"), "-s", "S1", "--targets", "chrT:%d-%d" % (b0 + 1, b1), "--tile", 2000])


def test_cli_all_out_threads_and_shards(files):
    f = files
    o = lambda n: str(f["d"] / n)                                           # noqa: E731
    cli(f["common"] + ["-o", o("a.vcf.gz"), "-A", "-t", "1"])
    want = payload(o("a.vcf.gz"))
    for tag, extra in (("t1", ["-t", "1"]), ("t2", ["-t", "2"])):
        err = cli(f["common"] + ["-o", o(tag + ".vcf.gz"), "-A", "--score-mem-mb", MB, "--timing"] + extra)
        assert chunks_per_tile(err) >= MIN_CHUNKS, err
        assert payload(o(tag + ".vcf.gz")) == want, tag
    cli(f["common"] + ["-o", o("zero.vcf.gz"), "-A", "-t", "1", "--score-mem-mb", "0"])
    assert payload(o("zero.vcf.gz")) == want
    # the default gate as well (few records: one chunk may do), and two shards joined
    cli(f["common"] + ["-o", o("d.vcf.gz"), "-t", "2"])
    cli(f["common"] + ["-o", o("ds.vcf.gz"), "-t", "2", "--score-mem-mb", MB])
    assert payload(o("ds.vcf.gz")) == payload(o("d.vcf.gz"))
    assert len(want) > 2 * len(payload(o("d.vcf.gz")))                      # -A wrote what the default gate does not (as test_gpu_force_sites states it)
    outs = []
    for i in range(2):
        cli(f["common"] + ["-o", o("sh%d.vcf.gz" % i), "-A", "--shard", "%d/2" % i, "--score-mem-mb", MB])
        outs.append(o("sh%d.vcf.gz" % i))
    cli(["--concat", o("joined.vcf.gz")] + outs)
    assert [l for l in payload(o("joined.vcf.gz")) if not l.startswith("##")] == [l for l in want if not l.startswith("##")]


def test_cli_force_sites(files):
    f = files
    o = lambda n: str(f["d"] / n)                                           # noqa: E731
    sites = sorted(set(np.random.default_rng(3).integers(f["b0"] + 1, f["b1"], 400).tolist()))
    bed = f["d"] / "s.bed"
    bed.write_text("".join("chrT\t%d\t%d\n" % (x - 1, x) for x in sites))
    cli(f["common"] + ["-o", o("fs.vcf.gz"), "-t", "2", "--force-sites", bed])
    err = cli(f["common"] + ["-o", o("fss.vcf.gz"), "-t", "2", "--force-sites", bed, "--score-mem-mb", MB, "--timing"])
    assert chunks_per_tile(err) >= MIN_CHUNKS, err
    assert payload(o("fss.vcf.gz")) == payload(o("fs.vcf.gz"))
    records = lambda path: [l for l in payload(path) if not l.startswith("#")]   # noqa: E731
    cli(f["common"] + ["-o", o("fs_default.vcf.gz"), "-t", "2"])
    assert len(records(o("fs.vcf.gz"))) > len(records(o("fs_default.vcf.gz")))  # the sites added lines


def test_cli_merge_regions(tmp_path):
    d = str(tmp_path)
    bam, fa, bed, lines, contigs = panel(d)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    common = [bam, "-f", fa, "-s", "S", "-t", "2", "-R", bed, "-A"]
    for N in (0, 300, 5000):
        cli(common + ["-o", o("m%d.vcf.gz" % N), "--merge-regions", N])
        err = cli(common + ["-o", o("s%d.vcf.gz" % N), "--merge-regions", N, "--score-mem-mb", MB, "--timing"])
        assert chunks_per_tile(err) >= MIN_CHUNKS, (N, err)
        assert payload(o("s%d.vcf.gz" % N)) == payload(o("m%d.vcf.gz" % N)), N
    assert any(not l.startswith("#") for l in payload(o("m300.vcf.gz")))


def test_cli_pair_mode(tmp_path):
    rd = make_tn_files(tmp_path)
    tb, nb, fa = str(tmp_path / "tumor.bam"), str(tmp_path / "normal.bam"), str(tmp_path / "tn.fa")
    o = lambda n: str(tmp_path / n)                                         # noqa: E731
    assert rd["tumor"]["beg"] > 0
    base = [tb, "--normal-bam", nb, "-f", fa, "-s", "TUM,NOR", "--tile", 2000, "-t", "2", "-A"]
    cli(base + ["-o", o("n.vcf.gz"), "--tumor-output", o("t.vcf.gz")])
    err = cli(base + ["-o", o("ns.vcf.gz"), "--tumor-output", o("ts.vcf.gz"), "--score-mem-mb", MB, "--timing"])
    print(err[-600:])
    assert chunks_per_tile(err, "tumor") >= MIN_CHUNKS, err
    assert chunks_per_tile(err, "normal") >= 1, err                          # (the normal sample scores the tumor's positions only)
    assert payload(o("ts.vcf.gz")) == payload(o("t.vcf.gz"))                # both output files
    assert payload(o("ns.vcf.gz")) == payload(o("n.vcf.gz"))
    assert any(not l.startswith("#") for l in payload(o("t.vcf.gz"))) and any(not l.startswith("#") for l in payload(o("n.vcf.gz")))


def test_python_call_region_writes_the_command_line_text(files, gpu_lib):
    f = files
    o = lambda n: str(f["d"] / n)                                           # noqa: E731
    args = ["--targets", "chrT:%d-%d" % (f["b0"] + 1, f["b1"]), "--tile", 2000, "-A"]
    cli(f["common"] + ["-o", o("cli_py.vcf.gz"), "-A", "-t", "1", "--score-mem-mb", MB])
    p, g = resolved(f["bam"], args)
    kw = dict(sample="S1", tile=2000, params=p, group_params=g, molecule_tag=g.molecule_tag, disable_duplex=g.disable_duplex, all_out=True)
    body = lambda path: [l for l in gzip.open(path, "rt").read().splitlines() if not l.startswith("##")]   # noqa: E731
    for tag, mb in (("stream", MB), ("one", 0)):
        pipeline.write_vcf(region.gpu_lib(), f["bam"], f["fa"], "chrT", f["b0"], f["b1"], o("py_%s.vcf.gz" % tag), score_mem_mb=mb, **kw)
        assert body(o("py_%s.vcf.gz" % tag)) == body(o("cli_py.vcf.gz")), tag
    # the BED-batch call
    d = str(f["d"] / "panel")
    os.makedirs(d)
    bam, fa, bed, lines, contigs = panel(d)
    from uvc_amd import io as uio
    pieces = uio.plan_bed_batches([contigs.index(c) for c, _, _ in lines], [b for _, b, _ in lines], [e for _, _, e in lines], 300, 1000000)
    assert pipeline.call_bed_batches(gpu_lib, bam, fa, pieces, all_out=True, score_mem_mb=MB) == pipeline.call_bed_batches(gpu_lib, bam, fa, pieces, all_out=True)
