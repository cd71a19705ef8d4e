"""The microsatellite tally of ranges of the accumulated region (uvcgpu_region_msi, Region.msi) and the file built from it (uvc1-mi355x
--msi-out).  Every number is an integer and every word of every row is compared for equality: the rows of the HIP library against the numpy
restatement (msi_restatement.py) over what the ORACLE's handle gives through the public calls -- its STR planes, its depth planes, its InDel
allele rows.  The input (msi_inputs.py) is a 6 kb reference with planted repeats and reads whose CIGARs carry every class of InDel the tally
distinguishes, in a plain arm and a duplex-UMI arm; the test asserts on the restatement's own output that every class occurs, so an input
that stops covering one fails instead of passing vacuously."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bamwriter
import msi_inputs as mi
import msi_restatement as mr
from test_gpu_coverage import EXE, run_cli
from util import run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

E = _ffi.ENUMS
EINVAL, ENOMEM = E["UVCGPU_EINVAL"], E["UVCGPU_ENOMEM"]
ROW = E["UVC_MSI_ROW"]
DEFAULT, HOMOPOLYMERS, EVERY_HEAD = (10, 5, 6), (10, 5, 1), (1, 1, 6)
_cache = {}


def planes_of(R, reads):
    """what the restatement reads, from a handle's public calls: STR planes, the four measures bDP cDP12 cDP2 dDP1 per position, allele rows"""
    base = slice(E["UVC_BASE_A"], E["UVC_BASE_NN"] + 1)
    frag, fam, dup = R.fetch("FRAG"), R.fetch("FAM"), R.fetch("DUPLEX")
    m4 = np.stack([frag[:, E["UVC_FRAG_bDP"], base].sum((0, 1), dtype=np.int64), fam[:, E["UVC_FAM_cDP12"], base].sum((0, 1), dtype=np.int64),
                   fam[:, E["UVC_FAM_cDP2"], base].sum((0, 1), dtype=np.int64), dup[E["UVC_DUPLEX_dDP1"], base].sum(0, dtype=np.int64)])
    rtr = R.fetch("RTR")
    for a in (m4, rtr):
        a.setflags(write=False)
    return dict(reads=reads, beg=R.beg, npos=R.npos, rtr=rtr, m4=m4, alleles=R.indel_alleles(), refseq=reads["refseq"])


def oracle_arm(arm, oracle_lib):
    """the reads of an arm and what the oracle's handle gives for them; computed once"""
    if arm not in _cache:
        reads = mi.build(arm)
        Ro = run_region(oracle_lib, reads)
        _cache[arm] = planes_of(Ro, reads)
        Ro.close()
    return _cache[arm]


def want_of(ref, ranges, req):
    return mr.tally(ref["rtr"], ref["beg"], ranges, ref["m4"], ref["alleles"], ref["refseq"], *req)


def check(Rg, ref, ranges, req, what):
    want, classes = want_of(ref, ranges, req)
    got = Rg.msi(ranges, *req)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:8]])
    return want, classes


def level(rows, lv):
    return rows[:, mr.HIST + lv * mr.NBIN:mr.HIST + (lv + 1) * mr.NBIN]


@pytest.mark.parametrize("arm", ["plain", "duplex"])
def test_every_word_equals_the_restatement(arm, oracle_lib, gpu_lib):
    ref = oracle_arm(arm, oracle_lib)
    beg, npos = ref["beg"], ref["npos"]
    whole = [(beg, beg + npos)]
    # ---- the input covers what it is meant to cover (asserted on the restatement alone) ----
    want, classes = want_of(ref, whole, DEFAULT)
    print(arm, "loci", want[:, 1:4].tolist(), classes)
    for k in ("no_locus", "unit_del", "unit_ins", "tail", "del_past_end", "non_multiple", "wrong_bases", "behind_last_unit"):
        assert classes[k] > 0, (arm, k, classes)
    heads = {int(p) - beg: (int(tl), int(ul), int(fl)) for p, tl, ul, fl in want[:, 1:5]}
    for at, unit, copies in mi.PLANTS:
        if copies * len(unit) >= 10 and copies >= 5:
            assert heads.get(at) == (copies * len(unit), len(unit), 1 if at in (0, mi.N - 16) else 0), (at, unit, heads.get(at))
    assert 1600 not in heads                                                                   # (CA)4: below min_units
    assert heads[1900][0] + 1900 == 1916 and 1012 < 1024 < 1012 + heads[1012][0] and 2038 < 2048 < 2038 + heads[2038][0]   # back to back; across the block seams
    assert not want[want[:, 4] == 1, 5:].any() and (want[want[:, 4] == 0, 5] > 0).all()          # EDGE rows are zeros, the others have fragments on them
    a20 = want[[int(p) - beg == 300 for p in want[:, 1]]][0]
    assert a20[mr.HIST + 0] > 0 and a20[mr.HIST + 4] > 0 and a20[mr.HIST + 5] > 0 and a20[mr.HIST + 6] > 0 and a20[mr.HIST + mr.OTHER] > 0   # -7 (tail), -2, -1, +1 units, OTHER
    for lv in range(4):                                                                        # all four levels count in the duplex arm, two in the plain one
        assert (level(want, lv).sum() > 0) == (arm == "duplex" or lv < 2), (arm, lv)
        assert (want[want[:, 4] == 0, mr.DEPTH + lv] > 0).all() == (arm == "duplex" or lv < 2), (arm, lv)
    # ---- range lists x requests ----
    r150 = mi.ranges_150(beg)
    assert len(r150) == 40 and r150[-1][1] <= beg + npos and r150[20][0] < beg + 3140 < r150[20][1] < beg + 3164
    Rg = run_region(gpu_lib, ref["reads"])
    for req in (DEFAULT, HOMOPOLYMERS, EVERY_HEAD):
        w1, c1 = check(Rg, ref, whole, req, ("whole", req))
        w2, c2 = check(Rg, ref, r150, req, ("40 x 150", req))
        assert np.array_equal(w1[:, 1:], w2[:, 1:])                                             # the same loci (the region's last position is never a head); only the range differs
        assert (w2[:, 0] == (w2[:, 1] - beg) // 150).all()                                      # a locus belongs to the range of its head
    assert [int(p) - beg for p in want_of(ref, whole, HOMOPOLYMERS)[0][:, 1]] == [300, 2038]
    n_every = len(want_of(ref, whole, EVERY_HEAD)[0])
    assert n_every > npos // 2, n_every                                                         # nearly every head a locus: the compaction's stress case
    # a few odd lists: single positions on and beside heads, ranges that begin and end inside tracts, the last position alone
    check(Rg, ref, [(beg + 299, beg + 300), (beg + 300, beg + 301), (beg + 301, beg + 302), (beg + 610, beg + 1013), (beg + 1023, beg + 1025), (beg + 2038, beg + 2039), (beg + npos - 1, beg + npos)], DEFAULT, "odd")
    check(Rg, ref, [(beg + k, beg + k + 1) for k in range(1850, 2150)], EVERY_HEAD, "300 single positions")
    # a range that holds no locus: legal, zero rows
    empty = [(beg + 400, beg + 590)]
    assert len(want_of(ref, empty, DEFAULT)[0]) == 0 and Rg.msi(empty).shape == (0, ROW)
    # two calls on one handle give equal bytes, whatever ran in between
    first = Rg.msi(whole, *EVERY_HEAD).tobytes()
    Rg.msi(empty)
    Rg.score()
    assert Rg.msi(whole, *EVERY_HEAD).tobytes() == first
    Rg.close()


def raw_fn(lib):
    fn = lib.dll.uvcgpu_region_msi
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return fn


def test_sizes_first_and_a_handle_reused_for_a_shorter_region(oracle_lib, gpu_lib):
    ref = oracle_arm("duplex", oracle_lib)
    Rg = run_region(gpu_lib, ref["reads"])
    fn = raw_fn(gpu_lib)
    beg, npos = ref["beg"], ref["npos"]
    ranges = [(beg + 7, beg + 900), (beg + 900, beg + npos)]
    want, _ = want_of(ref, ranges, DEFAULT)
    assert len(want) >= 10
    arr = (_ffi.UvcCoverageRange * 2)(*[_ffi.UvcCoverageRange(*q) for q in ranges])
    req = _ffi.UvcMsiRequest(*DEFAULT)
    n = C.c_int64(-1)
    assert fn(Rg.h, arr, 2, C.byref(req), None, 0, C.byref(n)) == ENOMEM and n.value == len(want)          # capacity 0: the size alone
    canary = np.full((len(want) + 4, ROW), 0x5A5A5A5A, np.int32)
    buf = canary.copy()
    n.value = -1
    assert fn(Rg.h, arr, 2, C.byref(req), buf.ctypes.data, 0, C.byref(n)) == ENOMEM and n.value == len(want) and np.array_equal(buf, canary)
    n.value = -1
    assert fn(Rg.h, arr, 2, C.byref(req), buf.ctypes.data, len(want) - 1, C.byref(n)) == ENOMEM and n.value == len(want) and np.array_equal(buf, canary)
    n.value = -1
    assert fn(Rg.h, arr, 2, C.byref(req), buf.ctypes.data, len(want), C.byref(n)) == 0 and n.value == len(want)   # the exact capacity
    assert np.array_equal(buf[:len(want)], want) and np.array_equal(buf[len(want):], canary[len(want):])
    again = canary.copy()
    assert fn(Rg.h, arr, 2, C.byref(req), again.ctypes.data, len(want) + 4, C.byref(n)) == 0 and again.tobytes() == buf.tobytes()
    # the stress request first (the buffers grow), then the handle goes to a shorter region with other reads
    check(Rg, ref, ranges, EVERY_HEAD, "every head")
    reads = synth.generate_region(seed=3, region_len=1500, depth=40, indel_every=150, variant_inset=100)
    Ro = run_region(oracle_lib, reads)
    short = planes_of(Ro, reads)
    Ro.close()
    Rg.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Rg.set_reads(reads)
    Rg.accumulate()
    for req3 in (EVERY_HEAD, (4, 2, 6), DEFAULT):
        w, classes = check(Rg, short, [(short["beg"], short["beg"] + short["npos"])], req3, ("reused", req3))
    w, classes = want_of(short, [(short["beg"], short["beg"] + short["npos"])], EVERY_HEAD)
    assert len(w) > 500 and w[:, mr.HIST:mr.HIST + 52].sum() > 0, (len(w), classes)
    Rg.close()


def test_refusals(oracle_lib, gpu_lib):
    ref = oracle_arm("plain", oracle_lib)
    reads = ref["reads"]
    fn = raw_fn(gpu_lib)
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    beg, end = R.beg, R.beg + R.npos
    sentinel = -123456789

    def call(ranges, req=DEFAULT, n=None, cap=None, null=()):
        arr = (_ffi.UvcCoverageRange * max(len(ranges), 1))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])
        q = _ffi.UvcMsiRequest(*req)
        out = np.full((64, ROW), sentinel, np.int32)
        n_loci = C.c_int64(sentinel)
        rc = fn(R.h, None if "ranges" in null else arr, len(ranges) if n is None else n, None if "req" in null else C.byref(q), None if "loci" in null else out.ctypes.data,
                64 if cap is None else cap, None if "n_loci" in null else C.byref(n_loci))
        return rc, (out == sentinel).all() and n_loci.value == sentinel, gpu_lib.last_error()

    ok = [(beg + 5, beg + 1000), (beg + 1000, beg + 1001), (beg + 1200, end)]
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "accumulate" in msg and untouched
    R.set_reads(reads)
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "accumulate" in msg and untouched
    R.accumulate()
    want, _ = want_of(ref, ok, DEFAULT)
    assert len(want) >= 8 and np.array_equal(R.msi(ok), want)
    bad_calls = [
        ("unsorted", dict(ranges=[(beg + 200, beg + 250), (beg + 10, beg + 50)]), "range 1"),
        ("overlapping", dict(ranges=[(beg + 10, beg + 50), (beg + 49, beg + 60)]), "range 1"),
        ("empty", dict(ranges=[(beg + 10, beg + 50), (beg + 60, beg + 60)]), "range 1"),
        ("reversed", dict(ranges=[(beg + 50, beg + 10)]), "range 0"),
        ("in front of the region", dict(ranges=[(beg - 1, beg + 10)]), "range 0"),
        ("behind the region", dict(ranges=[(beg + 10, beg + 20), (end - 3, end + 1)]), "range 1"),
        ("no ranges", dict(ranges=ok, n=0), "n_ranges"),
        ("NULL ranges", dict(ranges=ok, null=("ranges",)), "NULL"),
        ("min_tracklen 0", dict(ranges=ok, req=(0, 5, 6)), "min_tracklen"),
        ("min_units 0", dict(ranges=ok, req=(10, 0, 6)), "min_units"),
        ("max_unitlen 0", dict(ranges=ok, req=(10, 5, 0)), "max_unitlen"),
        ("a negative field", dict(ranges=ok, req=(10, -3, 6)), "min_units"),
        ("NULL req", dict(ranges=ok, null=("req",)), "NULL"),
        ("NULL n_loci", dict(ranges=ok, null=("n_loci",)), "NULL"),
        ("negative capacity", dict(ranges=ok, cap=-1), "locus_capacity"),
        ("NULL loci with room", dict(ranges=ok, null=("loci",), cap=5), "loci is NULL"),
    ]
    for what, kw, word in bad_calls:
        rc, untouched, msg = call(**kw)
        assert rc == EINVAL and word in msg, (what, rc, msg)
        assert untouched, what
        assert np.array_equal(R.msi(ok), want), what                             # the handle is as usable as before
    R.score()
    assert np.array_equal(R.msi(ok), want)                                       # a plain score keeps the planes and the allele rows
    R.score(release_state=True)
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "release" in msg and untouched
    R.set_reads(reads)
    R.accumulate()
    assert np.array_equal(R.msi(ok), want)
    gen = R.score_stream(4096)
    next(gen)
    rc, untouched, msg = call(ok)
    assert rc == EINVAL and "stream" in msg and untouched
    gen.close()
    assert np.array_equal(R.msi(ok), want)
    R.close()


# ------------------------------------------------------------------------------------------------ command line
def test_cli_msi_out(tmp_path, gpu_lib):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    o = lambda n: os.path.join(d, n)                                        # noqa: E731
    reads = mi.build("plain")
    shifted = dict(reads, pos=reads["pos"] - mi.BEG)                        # the region as a contig of its own
    rng = np.random.default_rng(4)
    seq = reads["refseq"] + "".join("ACGT"[i] for i in rng.integers(0, 4, 300))
    bamwriter.write_bam(o("m.bam"), [("chrM1", len(seq))], bamwriter.records_from_reads(shifted, tid=0))
    bamwriter.write_fasta(o("m.fa"), [("chrM1", seq)])
    lines = [("chrM1", 250, 700, "first"), ("chrM1", 850, 2100, "second target"), ("chrM1", 3100, 3200, None), ("chrM1", 5900, 6200, "the end")]
    with open(o("m.bed"), "w") as f:
        f.write("".join(("%s\t%d\t%d" % l[:3]) + ("\t%s\n" % l[3] if l[3] else "\n") for l in lines))
    hb, hf = uio.Bam(o("m.bam")), uio.Fasta(o("m.fa"))
    req, min_depth, permille = (8, 4, 4), 55, 100
    opts = ["--msi-min-tract", "8", "--msi-min-units", "4", "--msi-max-unit", "4", "--msi-min-depth", "55", "--msi-unstable-permille", "100"]
    # (a) the file equals the Python chain: each line its own region, its loci through the store of the reader library
    store = uio.Msi(*req, min_depth, permille)
    targets, per_target = [], []
    for chrom, b, e, name in lines:
        t = store.add_target(chrom, b, e, name)
        res = pipeline.call_region(gpu_lib, hb, hf, chrom, b, e, keep_handle=True)
        lo, hi = max(res["score_range"][0], b), min(res["score_range"][1], e)
        rows = res["region"].msi([(lo, hi)], *req)
        res["region"].close()
        units = [hf.fetch(chrom, int(r[1]), int(r[1]) + int(r[3])).upper() for r in rows]
        store.add([t], rows, units)
        targets.append((chrom, b, e, name))
        per_target.append(list(zip(rows, units)))
    store.write(o("chain.tsv"))
    store.close()
    want = open(o("chain.tsv")).read()
    assert want == mr.report_text(targets, per_target, *req, min_depth, permille)
    body = [l.split("\t") for l in want.splitlines() if not l.startswith("#")]
    assert [int(l[1]) for l in body if l[6] == "first"][:2] == [300, 600] and len(body) >= 8 and sum(int(l[9]) > 0 for l in body) >= 5, body   # loci with shifted fragments
    assert "#summary\tb\tassessable\t%d\tunstable\t%d" % (sum(l[7] == "." and int(l[8]) >= 55 for l in body), sum(l[7] == "." and int(l[8]) >= 55 and 1000 * int(l[9]) >= 100 * int(l[8]) for l in body)) in want
    vcf_without = run_cli(o("m.bam"), o("m.fa"), o("plain.vcf.gz"), "-R", o("m.bed"), "-t", "2")
    vcf_with = run_cli(o("m.bam"), o("m.fa"), o("w.vcf.gz"), "-R", o("m.bed"), "-t", "2", "--msi-out", o("m.tsv"), *opts)
    got = open(o("m.tsv")).read()
    assert got == want, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:3]
    assert vcf_with == vcf_without and len(vcf_with) > 100                  # the VCF does not know about the tally
    # (b) beside --callable-out (the two share their targets), block-gzipped, one worker; (c) merged regions give the same loci here: no
    # tract of this panel touches the end of a line's region
    vcf = run_cli(o("m.bam"), o("m.fa"), o("c.vcf.gz"), "-R", o("m.bed"), "-t", "1", "--msi-out", o("z.tsv.gz"), "--callable-out", o("c.bed"), *opts)
    run_cli(o("m.bam"), o("m.fa"), o("c0.vcf.gz"), "-R", o("m.bed"), "-t", "1", "--callable-out", o("c0.bed"))
    assert vcf == vcf_without and gzip.open(o("z.tsv.gz"), "rt").read() == got and open(o("c.bed")).read() == open(o("c0.bed")).read()
    # (d) without a BED file and with the defaults: one target per contig, the planted loci of the whole reference
    run_cli(o("m.bam"), o("m.fa"), o("d.vcf.gz"), "-t", "2", "--tile", "100000", "--msi-out", o("d.tsv"))
    dl = [l.split("\t") for l in open(o("d.tsv")).read().splitlines()]
    assert dl[5:10] == [["#min_tract", "10"], ["#min_units", "5"], ["#max_unit", "6"], ["#min_depth", "30"], ["#unstable_permille", "200"]]
    at = {int(l[1]): l for l in dl if l[0] == "chrM1"}
    for p, unit, copies in mi.PLANTS:
        if copies >= 5 and 0 < p < mi.N - 16:
            assert at[p][2:6] == [str(p + len(unit) * copies), unit, str(len(unit)), str(copies)] and at[p][7] == ".", at.get(p)
