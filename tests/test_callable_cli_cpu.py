"""The callable-region BED without a device: --callable-out, --callable-min-depth and --callable-max-aDP are CLI options, their refusals come
before any file or device is opened, malformed criteria are refused, the bit table of include/uvc_callable.def is the header's enum, the
Python mirror and the library's names alike, the store of the reader library (uvcio_callable_*) sorts, fills and joins the runs that tiles
report and writes the text, and the numpy restatement gives the runs of a hand-built input that are written out here."""
import ctypes as C
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

import callable_restatement as cr
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--callable-out", "c.bed"]
PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_three_options_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--callable-out", '""'), ("--callable-min-depth", "cDP12=20"), ("--callable-max-aDP", "0")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


def test_the_bits_are_the_table_of_the_def_file_everywhere():
    E = _ffi.ENUMS
    names = [l.split("(")[1].split(")")[0].strip() for l in open(os.path.join(_ffi.ROOT, "include", "uvc_callable.def")) if l.startswith("UVC_CALLBIT(")]
    assert names == cr.BITS == region.CALLABLE_BITS == _ffi.CALLABLE_BITS and E["UVC_NCALLBIT"] == 8
    assert [E["UVC_CALL_" + n] for n in names] == list(range(8))
    assert names[:6] == ["LOW_" + m for m in region.COVERAGE_MEASURES] and cr.MEASURES == region.COVERAGE_MEASURES
    assert (cr.EXCESS, cr.NOCOV) == (E["UVC_CALL_EXCESS_aDP"], E["UVC_CALL_NO_COVERAGE"]) == (6, 7)
    assert C.sizeof(_ffi.UvcCallableRun) == 16 == region.CALLABLE_RUN.itemsize == cr.RUN.itemsize and C.sizeof(_ffi.UvcCallableRequest) == 28
    assert [n for n, _ in _ffi.UvcCallableRun._fields_] == list(region.CALLABLE_RUN.names) == list(cr.RUN.names)
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_callable_bit_name.restype, dll.uvcgpu_callable_bit_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_callable_bit_name(i).decode() for i in range(8)] == names
    assert dll.uvcgpu_callable_bit_name(-1) is None and dll.uvcgpu_callable_bit_name(8) is None
    assert hasattr(dll, "uvcgpu_region_callable")


@pytest.mark.parametrize("args,both", [
    (PAIR + ["-R", "p.bed"] + OUT, ("--callable-out", "--normal-bam")),
    (PAIR + ["--callable-max-aDP", "5"], ("--callable-max-aDP", "--normal-bam")),
    (PAIR + ["--callable-min-depth", "aDP=5"], ("--callable-min-depth", "--normal-bam")),
    (BASE + ["-R", "p.bed"] + OUT + ["--shard", "1/2"], ("--callable-out", "--shard")),
    (BASE + ["--callable-out=c.bed", "--shard=0/3"], ("--callable-out", "--shard")),
    (BASE + OUT + ["--repeat", "2"], ("--callable-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT, ("--callable-out", "/only-print-vcf-header/")),
    (BASE + ["--callable-min-depth", "aDP=5"], ("--callable-min-depth", "--callable-out")),
    (BASE + ["--callable-max-aDP", "500"], ("--callable-max-aDP", "--callable-out")),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("bad", ["cDP12=20,cDP12=30", "xDP=5", "cDP12", "cDP12=", "=5", "cDP12=-1", "cDP12=2.5", "cDP12=true", "cDP12=1e3", "aDP=1,,bDP=2", "aDP=1,", "", "aDP=1 ,bDP=2", "adp=5",
                                 "aDP=3000000000"])
def test_malformed_criteria_are_refused(tmp_path, bad):
    r = run(BASE + OUT + ["--callable-min-depth=" + bad], tmp_path)
    assert r.returncode == 2 and "--callable-min-depth" in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("bad", ["-5", "true", "1.5", "x", "", "1,2", "3e10"])
def test_malformed_max_adp_is_refused(tmp_path, bad):
    r = run(BASE + OUT + ["--callable-max-aDP=" + bad], tmp_path)
    assert r.returncode == 2 and "--callable-max-aDP" in r.stderr, (bad, r.stderr)
    r = run(BASE + ["--callable-out="], tmp_path)
    assert r.returncode == 2 and "--callable-out" in r.stderr
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The other reports and what they allow are not refused, with or without a BED file: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c.tsv", "--error-profile-out", "e.tsv", "--family-stats-out", "f.tsv", "--merge-regions", "2000", "--score-mem-mb", "64",
                          "--devices", "0", "-t", "2", "-A", "--force-sites", "s.bed", "--shard", "0/1", "--repeat", "1", "--callable-min-depth", "aDP=0,dDP1=3,cDP2=10", "--callable-max-aDP", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--callable" not in r.stderr, r.stderr
    r = run(BASE + ["--callable-out", "c.bed.gz", "--callable-max-aDP=900", "--tumor-vcf", "t.vcf.gz", "--tile", "1000", "--devices", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--callable" not in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ the store
MIN_DEPTH = [0, 0, 0, 20, 5, 0]
FILL = 1 << 7 | 1 << 3 | 1 << 4          # the mask of depth 0 under MIN_DEPTH
TARGETS = [("chr1", 100, 200, "exon 1"), ("chr1", 200, 260, None), ("chr2", 5, 50, "never visited"), ("chr2", 60, 90, "middle only"), ("chr2", 95, 95, "empty")]


def new_store():
    s = uio.Callable(cr.MEASURES, MIN_DEPTH, 300, cr.BITS)
    assert [s.add_target(*t) for t in TARGETS] == [0, 1, 2, 3, 4]
    return s


def runs(rows):
    r = np.zeros(len(rows), cr.RUN)
    for i, row in enumerate(rows):
        r[i] = row
    return r


# one call = (target of each range, its runs): exon 1 arrives in three pieces, the first and the last with equal masks (0) either side of
# the seams at 130 and 170; the second target begins at 200 with the mask exon 1 ends on; "middle only" is reported over [70, 80) alone
CALLS = [
    ([0], runs([(0, 100, 120, 0), (0, 120, 130, 8)])),
    ([0, 1], runs([(0, 170, 200, 0), (1, 200, 230, 0), (1, 230, 260, 64)])),
    ([0], runs([(0, 130, 150, 8), (0, 150, 170, 0)])),
    ([3], runs([(0, 70, 75, 16), (0, 75, 80, FILL)])),
]
WANT = ("##callable_regions=1\n#min_depth\taDP=0,bDP=0,cDP1=0,cDP12=20,cDP2=5,dDP1=0\n#max_aDP\t300\n#chrom\tbeg\tend\tclass\ttarget\n"
        "chr1\t100\t120\tCALLABLE\texon 1\n"
        "chr1\t120\t150\tLOW_cDP12\texon 1\n"                               # joined over the seam at 130
        "chr1\t150\t200\tCALLABLE\texon 1\n"                                # joined over the seam at 170 ...
        "chr1\t200\t230\tCALLABLE\t.\n"                                     # ... and not over the target border at 200
        "chr1\t230\t260\tEXCESS_aDP\t.\n"
        "chr2\t5\t50\tLOW_cDP12,LOW_cDP2,NO_COVERAGE\tnever visited\n"
        "chr2\t60\t70\tLOW_cDP12,LOW_cDP2,NO_COVERAGE\tmiddle only\n"
        "chr2\t70\t75\tLOW_cDP2\tmiddle only\n"
        "chr2\t75\t90\tLOW_cDP12,LOW_cDP2,NO_COVERAGE\tmiddle only\n"       # a reported run of the fill mask joins the fill behind it
        "#summary\tpositions\t235\n#summary\tCALLABLE\t100\n"
        "#summary\tLOW_aDP\t0\n#summary\tLOW_bDP\t0\n#summary\tLOW_cDP1\t0\n#summary\tLOW_cDP12\t100\n#summary\tLOW_cDP2\t75\n#summary\tLOW_dDP1\t0\n"
        "#summary\tEXCESS_aDP\t30\n#summary\tNO_COVERAGE\t70\n")


def test_the_text_of_hand_written_pieces(tmp_path):
    s = new_store()
    for tor, r in CALLS:
        s.add_runs(tor, r)
    assert s.n_runs() == 9
    plain, gz = tmp_path / "c.bed", tmp_path / "c.bed.gz"
    s.write(plain); s.write(gz)
    s.close()
    text = plain.read_text()
    assert text == WANT
    assert gzip.open(gz, "rt").read() == text
    assert open(gz, "rb").read()[12:16] == b"BC\x02\x00"                    # block-gzipped: the BGZF extra field
    per_target = [[], [], [], [], []]
    for tor, r in CALLS:
        for q in r:
            per_target[tor[q["range"]]].append((q["pos_beg"], q["pos_end"], q["mask"]))
    assert text == cr.report_text(TARGETS, per_target, MIN_DEPTH, 300)


def test_pieces_in_shuffled_order_from_several_threads_write_the_same_bytes(tmp_path):
    rng = np.random.default_rng(11)
    single = [([tor[q["range"]]], runs([(0, q["pos_beg"], q["pos_end"], q["mask"])])) for tor, r in CALLS for q in r]   # every run its own call
    one, many = new_store(), new_store()
    for tor, r in CALLS:
        one.add_runs(tor, r)
    order = rng.permutation(len(single)).tolist()
    th = [threading.Thread(target=lambda k=k: [many.add_runs(*single[i]) for i in order[k::4]]) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    one.write(tmp_path / "one.bed"); many.write(tmp_path / "many.bed")
    assert (tmp_path / "one.bed").read_bytes() == (tmp_path / "many.bed").read_bytes() == WANT.encode()
    one.close(); many.close()


def test_the_store_refuses_what_cannot_be_right(tmp_path):
    s = new_store()
    for what, tor, r, word in (("outside its target", [0], runs([(0, 90, 110, 0)]), "outside target 0"), ("empty", [1], runs([(0, 210, 210, 0)]), "empty"),
                               ("no such target", [9], runs([(0, 1, 2, 0)]), "does not exist"), ("no such range", [0], runs([(1, 100, 110, 0)]), "range 1")):
        with pytest.raises(IOError, match=word):
            s.add_runs(tor, r)
    assert s.n_runs() == 0
    s.add_runs([0], runs([(0, 100, 150, 0)]))
    s.add_runs([0], runs([(0, 140, 160, 8)]))
    with pytest.raises(IOError, match="overlap"):
        s.write(tmp_path / "c.bed")
    for path in (tmp_path / "no_such_dir" / "c.bed", tmp_path / "no_such_dir" / "c.bed.gz"):
        with pytest.raises(IOError, match="cannot create|overlap"):
            s.write(path)
    s.close()
    e = new_store()
    for path in (tmp_path / "no_such_dir" / "c.bed", tmp_path / "no_such_dir" / "c.bed.gz"):
        with pytest.raises(IOError, match="cannot create"):
            e.write(path)
    e.close()


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_on_forty_hand_built_positions():
    m = np.zeros((6, 40), np.int64)
    m[0] = [0] * 3 + [5] * 7 + [30] * 10 + [90] * 5 + [30] * 10 + [0] * 5      # aDP
    m[1] = m[0]
    m[2] = m[0] // 2
    m[3] = [0] * 3 + [2] * 7 + [10] * 4 + [25] * 16 + [10] * 5 + [0] * 5       # cDP12
    m[4] = [0] * 18 + [6] * 4 + [0] * 18                                       # cDP2
    md, mx = cr.request({"cDP12": 20, "cDP2": 5}, 80)
    assert (md, mx) == ([0, 0, 0, 20, 5, 0], 80)
    mask = cr.masks_of(m, md, mx)
    L12, L2, X, N = 8, 16, 64, 128
    assert mask.tolist() == [N | L12 | L2] * 3 + [L12 | L2] * 11 + [L2] * 4 + [0] * 2 + [X] * 2 + [X | L2] * 3 + [L2] * 5 + [L12 | L2] * 5 + [N | L12 | L2] * 5
    got = cr.runs_of(m, 1000, [(1000, 1040)], md, mx)
    assert got.tolist() == [(0, 1000, 1003, N | L12 | L2), (0, 1003, 1014, L12 | L2), (0, 1014, 1018, L2), (0, 1018, 1020, 0), (0, 1020, 1022, X), (0, 1022, 1025, X | L2),
                            (0, 1025, 1030, L2), (0, 1030, 1035, L12 | L2), (0, 1035, 1040, N | L12 | L2)]
    # runs never cross a range border: two ranges that touch inside the stretch of equal masks, a single position, a gap
    got = cr.runs_of(m, 1000, [(1001, 1008), (1008, 1016), (1019, 1020), (1036, 1040)], md, mx)
    assert got.tolist() == [(0, 1001, 1003, N | L12 | L2), (0, 1003, 1008, L12 | L2), (1, 1008, 1014, L12 | L2), (1, 1014, 1016, L2), (2, 1019, 1020, 0), (3, 1036, 1040, N | L12 | L2)]
    # the all-zero request: only NO_COVERAGE can be set
    got = cr.runs_of(m, 0, [(0, 40)], *cr.request())
    assert got.tolist() == [(0, 0, 3, N), (0, 3, 35, 0), (0, 35, 40, N)]
    assert cr.class_of(0) == "CALLABLE" and cr.class_of(N | L12 | X) == "LOW_cDP12,EXCESS_aDP,NO_COVERAGE" and cr.depth0_mask(md) == (N | L12 | L2)
    assert cr.fill_join(10, 30, [(20, 25, 0), (12, 20, 0), (25, 28, N | L12 | L2)], md) == [(10, 12, N | L12 | L2), (12, 25, 0), (25, 30, N | L12 | L2)]
