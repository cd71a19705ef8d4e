"""The fragment profile without a device: --fragment-profile-out and its sub-options are CLI options with their defaults in --help, their
refusals come before any file or device is opened, malformed values are refused, the row layout is the table of
include/uvc_fragprofile.def in the header, the Python mirror and the library alike, the store of the reader library
(uvcio_fragprofile_*) sums what tiles report and writes the text, and the numpy restatement gives the rows of a hand-made input that are
written out here."""
import ctypes as C
import gzip
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import fragprofile_restatement as fp
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--fragment-profile-out", "f.tsv"]
WIN = ["--fragment-profile-window", "1000"]
SUBS = {"--fragment-profile-window": "1000", "--fragment-profile-min-mapq": "20", "--fragment-profile-short": "90-140", "--fragment-profile-long": "141-250"}
ROW, TROW = _ffi.ENUMS["UVC_FRAGPROF_ROW"], _ffi.ENUMS["UVC_FRAGPROF_TARGET_ROW"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_options_as_cli_with_their_defaults(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--fragment-profile-out", '""'), ("--fragment-profile-window", "0"), ("--fragment-profile-min-mapq", "0"), ("--fragment-profile-short", "100-150"),
                      ("--fragment-profile-long", "151-220")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


def test_the_row_is_the_table_of_the_def_file_everywhere():
    E = _ffi.ENUMS
    table = [l.split("(")[1].rstrip(")\n").replace(" ", "").split(",") for l in open(os.path.join(_ffi.ROOT, "include", "uvc_fragprofile.def")) if l.startswith("UVC_FRAGPROF(")]
    names = [t[0] for t in table]
    assert names == fp.TARGET_NAMES + ["reserved", "families_both_strands", "ends", "ends_off_region", "ends_no_ref", "reserved2", "LEN", "FAMLEN", "MOTIF"]
    assert region.FRAGMENT_PROFILE == names and E["UVC_NFRAGPROF"] == len(names) == 16
    assert [E["UVC_FRAGPROF_" + n] for n in names] == list(range(16))
    first, words = [int(t[1]) for t in table], [int(t[2]) for t in table]
    assert first == [sum(words[:k]) for k in range(16)] and sum(words) == ROW == fp.ROW == 2320
    at = dict(zip(names, zip(first, words)))
    assert at["LEN"] == (fp.LEN, fp.NLEN) == (E["UVC_FRAGPROF_LEN_BINS"], E["UVC_FRAGPROF_NLEN"]) == (16, 1024)
    assert at["FAMLEN"] == (fp.FAMLEN, fp.NLEN) == (E["UVC_FRAGPROF_FAMLEN_BINS"], 1024) and at["MOTIF"] == (fp.MOTIF, fp.NMOTIF) == (E["UVC_FRAGPROF_MOTIF_BINS"], E["UVC_FRAGPROF_NMOTIF"]) == (2064, 256)
    assert (TROW, E["UVC_FRAGPROF_NCOUNTER"]) == (fp.TARGET_ROW, fp.NCOUNTER) == (8, 16)
    assert [at[n][0] for n in fp.SUMMARY_NAMES] == fp.SUMMARY_WORDS and [at[n][0] for n in fp.TARGET_NAMES] == list(range(7))
    assert (fp.PAIRS, fp.OTHERS, fp.SINGLES, fp.LEN_SUM, fp.SHORT, fp.LONG, fp.FAMILIES, fp.RESERVED) == tuple(range(8))
    assert (fp.FAMILIES_BOTH, fp.ENDS, fp.ENDS_OFF, fp.ENDS_NO_REF) == tuple(at[n][0] for n in ("families_both_strands", "ends", "ends_off_region", "ends_no_ref"))
    assert fp.CONTINUES == E["UVC_FAMRANGE_CONTINUES"] == 1 and C.sizeof(_ffi.UvcFragmentProfileRequest) == 20
    assert (E["UVC_BASE_A"], E["UVC_BASE_C"], E["UVC_BASE_G"], E["UVC_BASE_T"]) == tuple(fp.motif_code(c) for c in "ACGT") == (0, 1, 2, 3) and fp.motif_code("N") < 0
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_fragment_profile_name.restype, dll.uvcgpu_fragment_profile_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_fragment_profile_name(i).decode() for i in range(16)] == names
    assert dll.uvcgpu_fragment_profile_name(-1) is None and dll.uvcgpu_fragment_profile_name(16) is None
    assert hasattr(dll, "uvcgpu_region_fragment_profile")


def test_the_new_symbols_are_declared_where_the_symbol_checks_look():
    """tests/test_capi_symbols.py takes its lists from the headers: the new entry points are in them, so those checks cover them"""
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(_ffi.ROOT, "include", name)).read(), flags=re.S)   # noqa: E731
    gpu = set(re.findall(r"\b(uvcgpu_[a-z_0-9]+)\s*\(", strip("uvcgpu.h")))
    assert {"uvcgpu_region_fragment_profile", "uvcgpu_fragment_profile_name"} <= gpu
    io_names = set(re.findall(r"\b(uvcio_[a-z_0-9]+)\s*\(", strip("uvcio.h")))
    want = {"uvcio_fragprofile_" + f for f in ("open", "add_target", "add_piece", "add_profile", "write", "close")}
    assert want <= io_names and all(hasattr(uio.dll(), n) for n in want)


PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]


@pytest.mark.parametrize("args,both", [
    (PAIR + OUT + WIN, ("--fragment-profile-out", "--normal-bam", "writes no fragment profile")),
    (PAIR + WIN, ("--fragment-profile-window", "--normal-bam", "writes no fragment profile")),
    (PAIR + ["--fragment-profile-short", "1-2"], ("--fragment-profile-short", "--normal-bam", "writes no fragment profile")),
    (BASE + OUT + WIN + ["--shard", "1/2"], ("--fragment-profile-out", "--shard")),
    (BASE + ["--fragment-profile-out=f.tsv", "--fragment-profile-window=500", "--shard=0/3"], ("--fragment-profile-out", "--shard")),
    (BASE + OUT + WIN + ["--repeat", "2"], ("--fragment-profile-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT + WIN, ("--fragment-profile-out", "/only-print-vcf-header/")),
    (BASE + OUT, ("--fragment-profile-out", "--fragment-profile-window")),                       # no BED file: windows are required
    (BASE + OUT + ["-R", "p.bed"] + WIN, ("--fragment-profile-window", "-R")),
    (BASE + OUT + ["--bed-in-fname", "p.bed"] + WIN, ("--fragment-profile-window", "--bed-in-fname")),
] + [(BASE + [sub, v], (sub, "needs --fragment-profile-out")) for sub, v in SUBS.items()])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_the_refusals_have_the_frames_of_the_family_report(tmp_path):
    """the same sentences as --family-stats-out gives, with this report's names in them"""
    for tail in (["--shard", "1/2"], ["--repeat", "2"]):
        a = run(BASE + OUT + WIN + tail, tmp_path).stderr
        b = run(BASE + ["--family-stats-out", "f.tsv", "--family-stats-window", "1000"] + tail, tmp_path).stderr
        assert a and a == b.replace("--family-stats", "--fragment-profile"), (a, b)
    a, b = run(BASE + OUT, tmp_path).stderr, run(BASE + ["--family-stats-out", "f.tsv"], tmp_path).stderr
    assert a and a == b.replace("--family-stats", "--fragment-profile")
    a, b = run(BASE + WIN, tmp_path).stderr, run(BASE + ["--family-stats-window", "1000"], tmp_path).stderr
    assert a and a == b.replace("--family-stats", "--fragment-profile")
    a, b = run(PAIR + OUT + WIN, tmp_path).stderr, run(PAIR + ["--family-stats-out", "f.tsv"], tmp_path).stderr
    assert a and a == b.replace("--family-stats", "--fragment-profile").replace("family report", "fragment profile")


@pytest.mark.parametrize("opt,bad", [("--fragment-profile-window", b) for b in ("0", "-5", "true", "1.5", "x", "", "1,2", "3e10")]
                         + [("--fragment-profile-min-mapq", b) for b in ("-1", "256", "x", "", "1.5", "true")]
                         + [(o, b) for o in ("--fragment-profile-short", "--fragment-profile-long") for b in ("150", "150-100", "-5-10", "a-b", "100-", "-100", "", "1e2-200", "100-150-200", "100 - 150")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + (WIN if opt != "--fragment-profile-window" else []) + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (opt, bad, r.stderr)
    assert "cannot open" not in r.stderr and os.listdir(tmp_path) == []


def test_good_values_and_allowed_companions_get_past_the_option_checks(tmp_path):
    """A-B values at their edges and the other reports are not refused: the run fails on the missing BAM."""
    for short, long in (("0-0", "0-2000000000"), ("100-100", "5-5"), ("7-9", "8-8")):
        r = run(BASE + OUT + WIN + ["--fragment-profile-short", short, "--fragment-profile-long=" + long, "--fragment-profile-min-mapq", "255", "--devices", "0"], tmp_path)
        assert r.returncode == 2 and "in.bam" in r.stderr and "--fragment-profile" not in r.stderr, r.stderr
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c.tsv", "--family-stats-out", "s.tsv", "--read-profile-out", "r.tsv", "--merge-regions", "2000", "--score-mem-mb", "64", "--devices", "0",
                          "-t", "2", "--shard", "0/1", "--repeat", "1"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--fragment-profile" not in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ the store
TARGETS = [("chr1", 100, 200, "exon 1"), ("chr1", 300, 400, None), ("chr2", 5, 50, "x"), ("chr2", 60, 70, "never visited")]


def test_pieces_from_several_threads_write_the_bytes_of_their_sum(tmp_path):
    rng = np.random.default_rng(5)
    rows = np.where(rng.random((24, TROW)) < 0.6, rng.integers(0, 1 << 40, (24, TROW)), 0)
    profs = np.where(rng.random((7, ROW)) < 0.3, rng.integers(0, 1 << 40, (7, ROW)), 0)
    pieces = [(int(rng.integers(0, 3)), r) for r in rows]
    req = dict(min_mapq=20, short=(90, 140), long=(141, 250))
    one, many = uio.FragmentProfile(**req), uio.FragmentProfile(**req)
    for s in (one, many):
        assert [s.add_target(*t) for t in TARGETS] == [0, 1, 2, 3]
    per = np.zeros((4, TROW), np.int64)
    for t, r in pieces:
        per[t] += r
    for t in range(3):
        one.add_piece(t, per[t])
    one.add_profile(profs.sum(0))
    order = rng.permutation(len(pieces)).tolist()
    th = [threading.Thread(target=lambda k=k: [many.add_piece(*pieces[i]) for i in order[k::4]] + [many.add_profile(p) for p in profs[k::4]]) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    one.write(tmp_path / "one.tsv"); many.write(tmp_path / "many.tsv")
    assert (tmp_path / "one.tsv").read_bytes() == (tmp_path / "many.tsv").read_bytes()
    assert (tmp_path / "one.tsv").read_text() == fp.report_text(TARGETS, per, profs.sum(0), 20, (90, 140), (141, 250))
    with pytest.raises(IOError, match="does not exist"):
        one.add_piece(4, rows[0])
    assert uio.dll().uvcio_fragprofile_add_piece(one.h, 0, None) != 0 and uio.dll().uvcio_fragprofile_add_profile(one.h, None) != 0
    with pytest.raises(ValueError):
        one.add_piece(0, np.zeros(7, np.int64))
    with pytest.raises(ValueError):
        one.add_profile(np.zeros(ROW + 1, np.int64))
    one.close(); many.close()


def test_the_text_of_hand_made_rows(tmp_path):
    prof = np.zeros(ROW, np.int64)
    prof[:12] = [10, 2, 3, 9000000000, 4, 5, 6, 999, 1, 17, 2, 1]   # word 7 is reserved: the report does not show it
    prof[12:16] = 77                                                 # nor the reserved words behind the counters
    prof[fp.LEN + 0], prof[fp.LEN + 167], prof[fp.LEN + 1023] = 1, 8, 1
    prof[fp.FAMLEN + 167], prof[fp.FAMLEN + 1022] = 5, 1
    prof[fp.MOTIF + 0], prof[fp.MOTIF + 27], prof[fp.MOTIF + 228], prof[fp.MOTIF + 255] = 3, 9, 4, 1
    a = np.array([4, 1, 2, 9000000000, 1, 2, 3, 555])
    b = np.array([1, 0, 0, 160, 0, 1, 1, 0])
    s = uio.FragmentProfile()
    for t in TARGETS:
        s.add_target(*t)
    s.add_piece(0, a); s.add_piece(0, b); s.add_piece(2, b); s.add_profile(prof)
    plain, gz = tmp_path / "f.tsv", tmp_path / "f.tsv.gz"
    s.write(plain); s.write(gz)
    s.close()
    text = plain.read_text()
    lines = text.splitlines()
    assert lines[:5] == ["##fragment_profile=1", "##fragment_profile_min_mapq=0", "##fragment_profile_short=100-150", "##fragment_profile_long=151-220",
                         "##summary, lengths and end motifs: every fragment and family that overlaps a target, counted once; target lines: every fragment and family that overlaps the target"]
    assert lines[5:17] == ["#summary", "pairs\t10", "others\t2", "singles\t3", "len_sum\t9000000000", "short\t4", "long\t5", "families\t6", "families_both_strands\t1", "ends\t17",
                           "ends_off_region\t2", "ends_no_ref\t1"]
    assert lines[17] == "#length\tfragments\tfamilies" and lines[18] == "0\t1\t0" and lines[18 + 167] == "167\t8\t5" and lines[18 + 1022] == "1022\t0\t1" and lines[18 + 1023] == "1023+\t1\t0"
    assert lines[18 + 1024] == "#end_motif\tcount" and len(lines) == 18 + 1024 + 1 + 256 + 1 + 4
    motifs = lines[18 + 1025:18 + 1025 + 256]
    assert motifs[0] == "AAAA\t3" and motifs[27] == "ACGT\t9" and motifs[228] == "TGCA\t4" and motifs[255] == "TTTT\t1" and motifs[1] == "AAAC\t0" and motifs[64] == "CAAA\t0"
    assert lines[-5:] == ["#chrom\tbeg\tend\tname\tpairs\tothers\tsingles\tlen_sum\tshort\tlong\tfamilies",
                          "chr1\t100\t200\texon 1\t5\t1\t2\t9000000160\t1\t3\t4",
                          "chr1\t300\t400\t.\t0\t0\t0\t0\t0\t0\t0",
                          "chr2\t5\t50\tx\t1\t0\t0\t160\t0\t1\t1",
                          "chr2\t60\t70\tnever visited\t0\t0\t0\t0\t0\t0\t0"]
    assert text.endswith("\n") and not re.search(r"[^\t\n]\.\d", text.split("#summary")[1].replace("\t.\t", "\t")), "integers only"
    assert gzip.open(gz, "rt").read() == text
    assert open(gz, "rb").read()[12:16] == b"BC\x02\x00"                    # block-gzipped: the BGZF extra field
    per = np.zeros((4, TROW), np.int64)
    per[0], per[2] = a + b, b
    assert text == fp.report_text(TARGETS, per, prof)


def test_write_fails_with_a_message_where_the_file_cannot_be_made(tmp_path):
    s = uio.FragmentProfile()
    for path in (tmp_path / "no_such_dir" / "f.tsv", tmp_path / "no_such_dir" / "f.tsv.gz"):
        with pytest.raises(IOError, match="cannot create"):
            s.write(path)
    s.close()


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_on_hand_made_fragments():
    """Seven fragments in four families over a reference of 40 bases, region [1000, 1040]; the rows are written out."""
    M, I, D, N, S = 0, 1, 2, 3, 4
    ref = "ACGTACGTAAAACCCCGGGGTTTTACGNTACGTTGCAACGT"[:40]
    alns = [  # (fam, strand, frag, pos, cigar, flag, mapq)
        (0, 0, 0, 1000, [(8, M)], 0, 60),                      # family 0 strand 0: pair [1000, 1020): L 20 ...
        (0, 0, 0, 1010, [(2, S), (4, M), (2, D), (4, M)], 16, 60),
        (0, 1, 1, 1004, [(6, M)], 0, 60),                      # ... strand 1: pair [1004, 1024) -> template [1000, 1024), both strands
        (0, 1, 1, 1014, [(5, M), (3, I), (5, M)], 16, 60),
        (1, 0, 2, 1020, [(6, M)], 16, 60),                     # family 1: everted [1020, 1036): other
        (1, 0, 2, 1030, [(6, M)], 0, 60),
        (1, 0, 3, 1002, [(6, M)], 0, 60),                      #   and a single [1002, 1008) -> not sized
        (2, 0, 4, 1024, [(4, M), (6, N), (4, M)], 0, 60),      # family 2: pair [1024, 1040), L 16: the N at 27 in its left motif, its right end at the last reference base
        (2, 0, 4, 1036, [(4, M)], 16, 60),
        (2, 0, 5, 1024, [(4, M)], 0, 10),                      #   a fragment below the mapping quality: nothing
        (3, 0, 6, 996, [(10, M)], 0, 60),                      # family 3: pair [996, 1012): begins in front of the region, L 16
        (3, 0, 6, 1008, [(4, M)], 16, 60),
        (3, 0, 6, 1030, [(8, M)], 16 | 0x800, 60),             #   its supplementary alignment does not count
    ]
    reads = dict(pos=np.array([a[3] for a in alns]), n_cigar=np.array([len(a[4]) for a in alns]), cigars=np.array([(ln << 4) | op for a in alns for ln, op in a[4]], np.uint32),
                 fam_id=np.array([a[0] for a in alns]), fam_strand=np.array([a[1] for a in alns]), frag_id=np.array([a[2] for a in alns]), flag=np.array([a[5] for a in alns]),
                 mapq=np.array([a[6] for a in alns]))
    f = fp.fragments(reads, 20)
    assert f["kind"].tolist() == [0, 0, 1, 2, 0, -1, 0] and (f["lo"] - 1000)[[0, 1, 2, 3, 4, 6]].tolist() == [0, 4, 20, 2, 24, -4] and (f["hi"] - 1000)[[0, 1, 2, 3, 4, 6]].tolist() == [20, 24, 36, 8, 40, 12]
    assert f["L"].tolist() == [20, 20, 16, 6, 16, 0, 16]
    fam = fp.families(f)
    assert fam["fam"].tolist() == [0, 2, 3] and (fam["tlo"] - 1000).tolist() == [0, 24, -4] and fam["TL"].tolist() == [24, 16, 16] and fam["both"].tolist() == [True, False, False]
    ranges = [(1000, 1004, 0, 0), (1004, 1010, 1004, 1), (1012, 1024, 1010, 0), (1030, 1041, 1024, 0)]
    rows, prof = fp.rows_and_profile(f, fam, ranges, 1000, ref, short=(16, 16), long=(17, 20))
    assert rows.tolist() == [[2, 0, 1, 36, 1, 1, 2, 0],     # fragments 0, 6 and the single; families 0 and 3
                             [1, 0, 0, 20, 0, 1, 0, 0],     # CONTINUES: only fragment 1 begins at or behind 1004; family 0 begins in front of it
                             [2, 1, 0, 40, 0, 2, 1, 0],     # fragments 0, 1 and the everted one; family 0 (family 3 ends at 1012)
                             [1, 1, 0, 16, 1, 0, 1, 0]]     # the pair over the N, the everted one; family 2
    want = np.zeros(fp.ROW, np.int64)
    want[:12] = [4, 1, 1, 72, 2, 2, 3, 0, 1, 5, 2, 1]
    want[fp.LEN + 20], want[fp.LEN + 16] = 2, 2
    want[fp.FAMLEN + 24], want[fp.FAMLEN + 16] = 1, 2
    for m in ("ACGT", "CCCC", "ACGT", "AAAA", "CGTT"):      # left of 0, right of 0 (GGGG reversed and complemented), left of 1, right of 1 (ref[20:24] TTTT), right of 4 (ref[36:40] AACG)
        want[fp.MOTIF + sum("ACGT".index(c) << (6 - 2 * k) for k, c in enumerate(m))] += 1
    # fragment 6: its left end lies in front of the region (off), its right end reads ref[8:12] = AAAA -> TTTT
    want[fp.MOTIF + 255] += 1
    want[fp.ENDS], want[fp.ENDS_OFF], want[fp.ENDS_NO_REF] = 6, 1, 1
    assert prof.tolist() == want.tolist(), np.flatnonzero(prof != want).tolist()
