"""The UMI family report without a device: --family-stats-out and --family-stats-window are CLI options, their refusals come before any file
or device is opened, malformed values are refused, the row layout is the table of include/uvc_famstats.def in the header, the Python mirror
and the library alike, the store of the reader library (uvcio_famstats_*) sums the pieces that tiles report and writes the text, and the
numpy restatement gives the rows of a hand-built input that are written out here."""
import ctypes as C
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

import famstats_restatement as fr
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--family-stats-out", "f.tsv"]
WIN = ["--family-stats-window", "1000"]
ROW = _ffi.ENUMS["UVC_FAMSTAT_ROW"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_two_options_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--family-stats-out", '""'), ("--family-stats-window", "0")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


def test_the_row_is_the_table_of_the_def_file_everywhere():
    E = _ffi.ENUMS
    table = [l.split("(")[1].rstrip(")\n").replace(" ", "").split(",") for l in open(os.path.join(_ffi.ROOT, "include", "uvc_famstats.def")) if l.startswith("UVC_FAMSTAT(")]
    names = [t[0] for t in table]
    assert names == ["target_" + c for c in fr.COUNTERS] + fr.FIRST_NAMES + ["reserved", "size", "strands"]
    assert region.FAMILY_STATS == names and E["UVC_NFAMSTAT"] == len(names) == 14
    assert [E["UVC_FAMSTAT_" + n] for n in names] == list(range(14))
    first, words = [int(t[1]) for t in table], [int(t[2]) for t in table]
    assert first == [sum(words[:k]) for k in range(14)] and sum(words) == ROW == E["UVC_FAMSTAT_ROW"] == 365
    assert (E["UVC_FAMSTAT_TARGET"], E["UVC_FAMSTAT_FIRST"], E["UVC_FAMSTAT_SIZE"], E["UVC_FAMSTAT_NSIZE"], E["UVC_FAMSTAT_STRANDS"], E["UVC_FAMSTAT_STRAND_CAP"]) == (0, 4, 12, 64, 76, 16)
    assert (fr.TARGET, fr.FIRST, fr.FLAGS, fr.SIZE, fr.NSIZE, fr.STRANDS, fr.CAP, fr.ROW) == (0, 4, first[names.index("families_umi")], 12, 64, 76, 16, 365)
    assert fr.CONTINUES == E["UVC_FAMRANGE_CONTINUES"] == 1 and C.sizeof(_ffi.UvcFamilyRange) == 16
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_family_stat_name.restype, dll.uvcgpu_family_stat_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_family_stat_name(i).decode() for i in range(14)] == names
    assert dll.uvcgpu_family_stat_name(-1) is None and dll.uvcgpu_family_stat_name(14) is None
    assert hasattr(dll, "uvcgpu_region_family_stats")


PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]


@pytest.mark.parametrize("args,both", [
    (PAIR + OUT + WIN, ("--family-stats-out", "--normal-bam")),
    (PAIR + WIN, ("--family-stats-window", "--normal-bam")),
    (BASE + OUT + WIN + ["--shard", "1/2"], ("--family-stats-out", "--shard")),
    (BASE + ["--family-stats-out=f.tsv", "--family-stats-window=500", "--shard=0/3"], ("--family-stats-out", "--shard")),
    (BASE + OUT + WIN + ["--repeat", "2"], ("--family-stats-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT + WIN, ("--family-stats-out", "/only-print-vcf-header/")),
    (BASE + WIN, ("--family-stats-window", "--family-stats-out")),
    (BASE + OUT, ("--family-stats-out", "--family-stats-window")),                       # no BED file: windows are required
    (BASE + OUT + ["-R", "p.bed"] + WIN, ("--family-stats-window", "-R")),
    (BASE + OUT + ["--bed-in-fname", "p.bed"] + WIN, ("--family-stats-window", "--bed-in-fname")),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("bad", ["0", "-5", "true", "false", "1.5", "x", "", "1,2", "3e10"])
def test_malformed_values_are_refused(tmp_path, bad):
    r = run(BASE + OUT + ["--family-stats-window=" + bad], tmp_path)
    assert r.returncode == 2 and "--family-stats-window" in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []
    r = run(BASE + ["--family-stats-out=", "--family-stats-window", "100"], tmp_path)
    assert r.returncode == 2 and "--family-stats-out" in r.stderr
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The other reports and what they allow are not refused: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c.tsv", "--error-profile-out", "e.tsv", "--merge-regions", "2000", "--score-mem-mb", "64", "--devices", "0", "-t", "2", "-A",
                          "--force-sites", "s.bed", "--shard", "0/1", "--repeat", "1"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--family-stats" not in r.stderr, r.stderr
    r = run(BASE + ["--family-stats-out", "f.tsv.gz", "--family-stats-window=500", "--tumor-vcf", "t.vcf.gz", "--tile", "1000", "--devices", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--family-stats" not in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ the store
def random_rows(rng, n):
    return np.where(rng.random((n, ROW)) < 0.3, rng.integers(0, 1 << 40, (n, ROW)), 0)


TARGETS = [("chr1", 100, 200, "exon 1"), ("chr1", 300, 400, None), ("chr2", 5, 50, "x"), ("chr2", 60, 70, "never visited")]


def expect_text(pieces):
    """(target, row) pieces -> the restatement's text of their sums"""
    per = np.zeros((len(TARGETS), 4), np.int64)
    total = np.zeros(ROW, np.int64)
    for t, row in pieces:
        per[t] += row[:4]
        total += row
    return fr.report_text(TARGETS, per, total)


def test_pieces_from_several_threads_write_the_bytes_of_their_sum(tmp_path):
    rng = np.random.default_rng(5)
    rows = random_rows(rng, 24)
    pieces = [(int(rng.integers(0, 3)), r) for r in rows]
    one, many = uio.FamilyStats(), uio.FamilyStats()
    for s in (one, many):
        assert [s.add_target(*t) for t in TARGETS] == [0, 1, 2, 3]
    for t in range(3):   # one piece per target: the sum of its pieces
        one.add_piece(t, sum((r for q, r in pieces if q == t), np.zeros(ROW, np.int64)))
    order = rng.permutation(len(pieces)).tolist()
    th = [threading.Thread(target=lambda k=k: [many.add_piece(*pieces[i]) for i in order[k::4]]) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    one.write(tmp_path / "one.tsv"); many.write(tmp_path / "many.tsv")
    assert (tmp_path / "one.tsv").read_bytes() == (tmp_path / "many.tsv").read_bytes()
    assert (tmp_path / "one.tsv").read_text() == expect_text(pieces)
    with pytest.raises(IOError, match="does not exist"):
        one.add_piece(4, rows[0])
    assert uio.dll().uvcio_famstats_add_piece(one.h, 0, None) != 0
    one.close(); many.close()


def test_the_text_of_a_hand_built_input(tmp_path):
    a, b = np.zeros(ROW, np.int64), np.zeros(ROW, np.int64)
    a[0:4] = [10, 25, 50, 4]                 # TARGET of "exon 1", first piece
    a[4:12] = [8, 20, 40, 3, 5, 3, 1, 999]   # FIRST counters, flags, and a reserved word the report does not show
    a[fr.SIZE + 0], a[fr.SIZE + 2], a[fr.SIZE + 63] = 4, 3, 1
    a[fr.STRANDS + 1 * 17 + 0], a[fr.STRANDS + 2 * 17 + 1], a[fr.STRANDS + 16 * 17 + 16] = 4, 3, 1
    b[0:4] = [2, 9000000000, 4, 0]           # a later piece of the same target
    b[4:8] = [2, 4, 4, 1]
    b[fr.SIZE + 1] = 2
    b[fr.STRANDS + 1 * 17 + 1], b[fr.STRANDS + 0 * 17 + 16] = 1, 1
    s = uio.FamilyStats()
    for t in TARGETS:
        s.add_target(*t)
    s.add_piece(0, a); s.add_piece(0, b); s.add_piece(2, b)
    plain, gz = tmp_path / "f.tsv", tmp_path / "f.tsv.gz"
    s.write(plain); s.write(gz)
    s.close()
    want = ("##family_stats=1\n##summary and histograms: every family that overlaps a target, counted once; target lines: every family that overlaps the target\n"
            "#summary\nfamilies\t12\nfragments\t28\nalignments\t48\nfamilies_both_strands\t5\nfamilies_umi\t5\nfamilies_duplex_tag\t3\nfamilies_amplicon\t1\n"
            "duplication_permille\t571\nmean_family_size_x1000\t2333\nboth_strands_permille\t416\n"
            "#family_size\tfamilies\n1\t4\n2\t4\n3\t3\n" + "".join("%d\t0\n" % k for k in range(4, 64)) + "64+\t1\n"
            "#strand0_size\tstrand1_size\tfamilies\n0\t16+\t2\n1\t0\t4\n1\t1\t2\n2\t1\t3\n16+\t16+\t1\n"
            "#chrom\tbeg\tend\tname\tfamilies\tfragments\talignments\tfamilies_both_strands\tmean_family_size_x1000\tboth_strands_permille\n"
            "chr1\t100\t200\texon 1\t12\t9000000025\t54\t4\t750000002083\t333\n"
            "chr1\t300\t400\t.\t0\t0\t0\t0\t0\t0\n"
            "chr2\t5\t50\tx\t2\t9000000000\t4\t0\t4500000000000\t0\n"
            "chr2\t60\t70\tnever visited\t0\t0\t0\t0\t0\t0\n")
    text = plain.read_text()
    assert text == want
    assert gzip.open(gz, "rt").read() == text
    assert open(gz, "rb").read()[12:16] == b"BC\x02\x00"                    # block-gzipped: the BGZF extra field
    assert text == expect_text([(0, a), (0, b), (2, b)])


def test_write_fails_with_a_message_where_the_file_cannot_be_made(tmp_path):
    s = uio.FamilyStats()
    for path in (tmp_path / "no_such_dir" / "f.tsv", tmp_path / "no_such_dir" / "f.tsv.gz"):
        with pytest.raises(IOError, match="cannot create"):
            s.write(path)
    s.close()


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_on_six_hand_built_families():
    """Six families over positions 0..400, CIGARs with clips, an insertion, a deletion and a skip; the rows are written out."""
    M, I, D, N, S = 0, 1, 2, 3, 4
    alns = [  # (fam, strand, frag, pos, cigar)
        (0, 0, 0, 100, [(50, M)]),                                   # family 0: one fragment of two alignments on strand 0 ...
        (0, 0, 0, 180, [(5, S), (45, M)]),                           #   ... -> [100, 225)
        (0, 1, 1, 120, [(20, M), (3, I), (27, M)]),                  #   and one fragment on strand 1: [120, 167): a = 1, b = 1, n = 3, dflag 3
        (1, 0, 2, 200, [(50, M)]),                                   # family 1: two fragments on strand 0: [200, 260), dflag 1
        (1, 0, 3, 205, [(25, M), (5, D), (25, M)]),
        (2, 1, 4, 260, [(40, M)]),                                   # family 2: strand 1 only: [260, 300), dflag 0
        (3, 0, 5, 50, [(10, M), (300, N), (10, M)]),                 # family 3: a skip: [50, 370), dflag 4
        (4, 0, 6, 300, [(30, M)]),                                   # family 4: [300, 330)
    ] + [(5, k % 2, 7 + k, 340 + k % 3, [(20, M)]) for k in range(40)]   # family 5: 20 + 20 fragments: [340, 362), dflag 3
    reads = dict(pos=np.array([a[3] for a in alns]), n_cigar=np.array([len(a[4]) for a in alns]), cigars=np.array([(ln << 4) | op for a in alns for ln, op in a[4]], np.uint32),
                 fam_id=np.array([a[0] for a in alns]), fam_strand=np.array([a[1] for a in alns]), frag_id=np.array([a[2] for a in alns]), fam_dflag=np.array([3, 1, 0, 4, 0, 3], np.uint8))
    f = fr.families(reads)
    assert f["a"].tolist() == [1, 2, 0, 1, 1, 20] and f["b"].tolist() == [1, 0, 1, 0, 0, 20] and f["n"].tolist() == [3, 2, 1, 1, 1, 40]
    assert f["lo"].tolist() == [100, 200, 260, 50, 300, 340] and f["hi"].tolist() == [225, 260, 300, 370, 330, 362]
    ranges = [(100, 200, 60, 0), (200, 260, 200, 1), (260, 300, 260, 0), (330, 340, 300, 0), (362, 400, 340, 0)]
    got = fr.rows(f, ranges)

    def row(target, first, flags=(0, 0, 0), size=(), strands=()):
        r = np.zeros(ROW, np.int64)
        r[0:4], r[4:8], r[8:11] = target, first, flags
        for k, v in size:
            r[fr.SIZE + k - 1] = v
        for a, b, v in strands:
            r[fr.STRANDS + a * 17 + b] = v
        return r
    want = np.stack([
        row((2, 3, 4, 1), (1, 2, 3, 1), (1, 1, 0), [(2, 1)], [(1, 1, 1)]),     # families 0 and 3; 3 begins in front of prev_end 60
        row((1, 2, 2, 0), (1, 2, 2, 0), (1, 0, 0), [(2, 1)], [(2, 0, 1)]),     # CONTINUES: 0 and 3 begin in front of 200; family 1 begins at it
        row((2, 2, 2, 0), (1, 1, 1, 0), (0, 0, 0), [(1, 1)], [(0, 1, 1)]),     # families 2 and 3 (hi of family 1 == 260: no overlap); 3 is not first
        row((1, 1, 1, 0), (0, 0, 0, 0)),                                         # family 3 alone (family 4 ends at 330, family 5 begins at 340)
        row((1, 1, 1, 0), (0, 0, 0, 0)),                                         # family 3 alone (hi of family 5 == 362)
    ])
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    whole = fr.rows(f, [(0, 400, 0, 0)])[0]
    assert np.array_equal(whole, row((6, 47, 48, 2), (6, 47, 48, 2), (3, 2, 1), [(1, 3), (2, 2), (40, 1)], [(1, 1, 1), (2, 0, 1), (0, 1, 1), (1, 0, 2), (16, 16, 1)]))
    assert fr.summary_lines(whole)[-3:] == ["duplication_permille\t872", "mean_family_size_x1000\t7833", "both_strands_permille\t333"]
