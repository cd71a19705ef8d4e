"""The microsatellite tally without a device: the numpy restatement (msi_restatement.py) against a hand-worked answer, the row layout of
include/uvc_msi.def in the header's enums, the Python mirror and the library's names alike, the store of the reader library (uvcio_msi_*)
and the text it writes, and the --msi-out options of the command line with their refusals, which come before any file or device."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import msi_restatement as mr
from uvc_amd import _ffi, io as uio

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--msi-out", "m.tsv"]
PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]
SUB = [("--msi-min-tract", "10"), ("--msi-min-units", "5"), ("--msi-max-unit", "6"), ("--msi-min-depth", "30"), ("--msi-unstable-permille", "200")]
E = _ffi.ENUMS


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def hand_input():
    """(CA)12 at region positions 10..33 between two 10-base flanks: the STR planes as accumulate would leave them (every flank base its own
    track of one unit), four depths with one dip inside the tract each, and the reference text"""
    beg, h, tl = 5000, 10, 24
    refseq = "GTTGACTGAT" + "CA" * 12 + "GGTTAGCTTA"
    npos = len(refseq) + 1
    rtr = np.zeros((7, npos), np.int32)
    rtr[0] = np.arange(npos); rtr[1] = 1; rtr[2] = 1
    rtr[0, h:h + tl], rtr[1, h:h + tl], rtr[2, h:h + tl] = h, tl, 2
    rtr[:, npos - 1] = rtr[:, npos - 2]                                             # the last position has no base: it repeats the one before it
    m4 = np.array([[50] * npos, [40] * npos, [12] * npos, [6] * npos])
    m4[0, 20], m4[1, 33], m4[2, 10], m4[3, 15] = 48, 37, 11, 5                      # the minima, inside the tract
    m4[:, 34] = 1                                                                   # the first base behind it does not count
    return beg, h, tl, refseq, rtr, m4


def allele(beg, x, symbol, ln, seq, counts, strand=0):
    return dict(refpos=beg + x, symbol=symbol, strand=strand, len=ln, seq=seq, bAD1=counts[0], cAD1=counts[1], c2AD=counts[2], c2dAD=counts[3])


def test_the_restatement_gives_the_hand_worked_bins():
    beg, h, tl, refseq, rtr, m4 = hand_input()
    D3P, D2, I3P = E["UVC_LINK_D3P"], E["UVC_LINK_D2"], E["UVC_LINK_I3P"]
    alleles = [allele(beg, 14, D2, 2, None, (5, 4, 3, 1)),                            # one unit deleted
               allele(beg, 16, I3P, 4, "CACA", (3, 2, 1, 0)),                         # two units inserted, in phase
               allele(beg, 18, D3P, 3, None, (2, 2, 0, 0))]                           # three bases: no whole number of units
    rows, classes = mr.tally(rtr, beg, [(beg, beg + rtr.shape[1])], m4, alleles, refseq)
    want = np.zeros((1, 64), np.int32)
    want[0, :9] = [0, beg + 10, 24, 2, 0, 48, 37, 11, 5]
    #                 -6 -5 -4 -3 -2 -1 +1 +2 +3 +4 +5 +6 OTHER
    want[0, 9:22] = [0, 0, 0, 0, 0, 5, 0, 3, 0, 0, 0, 0, 2]                           # fragments
    want[0, 22:35] = [0, 0, 0, 0, 0, 4, 0, 2, 0, 0, 0, 0, 2]                          # families
    want[0, 35:48] = [0, 0, 0, 0, 0, 3, 0, 1, 0, 0, 0, 0, 0]                          # consensus families
    want[0, 48:61] = [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]                          # duplex families
    assert np.array_equal(rows, want), rows.tolist()
    assert classes == dict(no_locus=0, edge=0, unit_del=1, unit_ins=1, tail=0, del_past_end=0, non_multiple=1, wrong_bases=0, behind_last_unit=0)
    # the other rules, one allele each: out of phase, the wrong bases, behind the last unit, past the end, the tail, both strands, plain sequence
    more = [(allele(beg, 17, I3P, 4, "ACAC", (1, 1, 1, 1)), 9 + 7),                   # q - h odd: the unit read from its second base
            (allele(beg, 17, I3P, 4, "CACA", (1, 1, 1, 1)), 9 + 12),                  # the same bases at an odd offset do not continue the tract
            (allele(beg, 34, E["UVC_LINK_I2"], 2, "CA", (1, 1, 1, 1)), 9 + 6),        # q = h + tracklen: behind the last unit
            (allele(beg, 34, E["UVC_LINK_I2"], 2, "AC", (1, 1, 1, 1)), 9 + 12),
            (allele(beg, 32, D3P, 4, None, (1, 1, 1, 1)), 9 + 12),                    # two units, the second outside the tract
            (allele(beg, 12, D3P, 16, None, (1, 1, 1, 1)), 9 + 0)]                    # eight units: the -6 bin
    for al, word in more:
        rows, _ = mr.tally(rtr, beg, [(beg, beg + rtr.shape[1])], m4, [al], refseq)
        assert rows[0, word] == 1 and rows[0, 9:61].sum() == 4, (al, rows[0, 9:22].tolist())
    rows, classes = mr.tally(rtr, beg, [(beg, beg + rtr.shape[1])], m4, [allele(beg, 14, D2, 2, None, (5, 4, 3, 1)), allele(beg, 14, D2, 2, None, (2, 2, 2, 2), strand=1), allele(beg, 4, D2, 2, None, (9, 9, 9, 9))], refseq)
    assert rows[0, 9 + 5] == 7 and rows[0, 48 + 5] == 3 and rows[0, 9:61].sum() == 7 + 6 + 5 + 3 and classes["no_locus"] == 1
    # requests, ranges and EDGE
    assert len(mr.loci_of(rtr, beg, [(beg, beg + 45)], max_unitlen=1)) == 0 and len(mr.loci_of(rtr, beg, [(beg, beg + 45)], min_units=13)) == 0
    assert len(mr.loci_of(rtr, beg, [(beg, beg + 10), (beg + 11, beg + 45)])) == 0                       # the head lies in no range
    assert mr.loci_of(rtr, beg, [(beg + 2, beg + 10), (beg + 10, beg + 11)])[0, :5].tolist() == [1, beg + 10, 24, 2, 0]   # the tract may leave the range
    every = mr.loci_of(rtr, beg, [(beg, beg + 45)], 1, 1, 6)
    assert len(every) == 21 and every[0, 4] == 1 and every[-1, 4] == 1 and every[1:-1, 4].sum() == 0     # position 44 repeats position 43: no head
    cut = rtr[:, :35].copy()                                                                            # the region ends on the tract's last base + 1
    rows, classes = mr.tally(cut, beg, [(beg, beg + 35)], m4[:, :35], alleles, refseq[:34])
    assert rows[0, 4] == 1 and not rows[0, 5:].any() and classes["edge"] == 3
    assert [mr.bin_of(s) for s in (-9, -6, -1, 1, 6, 7)] == [0, 0, 5, 6, 11, 11]


def test_the_row_is_the_table_of_the_def_file_everywhere():
    rows = [l.split("(")[1].split(")")[0].replace(" ", "").split(",") for l in open(os.path.join(_ffi.ROOT, "include", "uvc_msi.def")) if l.startswith("UVC_MSI(")]
    assert [(n, int(f), int(w)) for n, f, w in rows] == _ffi.MSI_SECTIONS
    assert [E["UVC_MSI_" + n] for n, _, _ in _ffi.MSI_SECTIONS] == list(range(E["UVC_NMSI"]))
    assert (mr.ROW, mr.DEPTH, mr.HIST, mr.NLEVEL, mr.NBIN, mr.OTHER, mr.MAXSHIFT, mr.EDGE) == tuple(E["UVC_MSI_" + k] for k in ("ROW", "DEPTH", "HIST", "NLEVEL", "NBIN", "OTHER", "MAXSHIFT", "EDGE"))
    assert mr.DEL_SYMBOLS == (E["UVC_LINK_D3P"], E["UVC_LINK_D2"], E["UVC_LINK_D1"]) and mr.INS_SYMBOLS == (E["UVC_LINK_I3P"], E["UVC_LINK_I2"], E["UVC_LINK_I1"])
    assert C.sizeof(_ffi.UvcMsiRequest) == 12
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_msi_section_name.restype, dll.uvcgpu_msi_section_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_msi_section_name(i).decode() for i in range(E["UVC_NMSI"])] == [n for n, _, _ in _ffi.MSI_SECTIONS]
    assert dll.uvcgpu_msi_section_name(-1) is None and dll.uvcgpu_msi_section_name(E["UVC_NMSI"]) is None
    assert hasattr(dll, "uvcgpu_region_msi")


# ------------------------------------------------------------------------------------------------ the store and the writer
def locus(rng_, pos, tl, ul, flags=0, depth=(0, 0, 0, 0), bins=()):
    r = np.zeros(64, np.int32)
    r[:5] = rng_, pos, tl, ul, flags
    r[5:9] = depth
    for lv, b, v in bins:
        r[9 + 13 * lv + b] = v
    return r


TARGETS = [("chr1", 100, 400, "exon 1"), ("chr2", 0, 90, None)]
# chr1: (CA)12 with a fifth of its fragments shifted, A x 15 with too little duplex depth; chr2: a tract cut by the region (EDGE)
LOCI = [(locus(0, 300, 15, 1, 0, (100, 40, 30, 29), [(0, 5, 19), (0, 12, 7), (1, 5, 8), (2, 5, 6), (3, 6, 6)]), "A"),
        (locus(0, 120, 24, 2, 0, (60, 50, 40, 30), [(0, 5, 8), (0, 0, 2), (0, 11, 2), (1, 4, 9), (1, 12, 3), (2, 5, 7), (3, 5, 5)]), "CA"),
        (locus(0, 0, 12, 3, 1), "AAG")]


def test_the_store_sorts_counts_and_writes(tmp_path):
    with uio.Msi(10, 5, 6, 30, 200) as s:
        assert [s.add_target(*t) for t in TARGETS] == [0, 1]
        # two calls, the loci of chr1 against their order in the file; range 0 of a call is the target named
        s.add([0], np.array([LOCI[0][0]]), [LOCI[0][1]])
        s.add([1], np.array([LOCI[2][0]]), [LOCI[2][1]])
        s.add([0], np.array([LOCI[1][0]]), [LOCI[1][1]])
        assert s.n_loci() == 3
        with pytest.raises(Exception):
            s.add([0], np.array([locus(0, 400, 12, 2)]), ["CA"])                     # begins outside its target
        with pytest.raises(Exception):
            s.add([0], np.array([locus(1, 120, 12, 2)]), ["CA"])                     # names a range the call does not have
        assert s.n_loci() == 3
        s.write(str(tmp_path / "m.tsv"))
        s.write(str(tmp_path / "m.tsv.gz"))
    text = open(tmp_path / "m.tsv").read()
    assert text == mr.report_text(TARGETS, [[LOCI[0], LOCI[1]], [LOCI[2]]], 10, 5, 6, 30, 200)
    lines = text.splitlines()
    assert lines[0] == "##msi_loci=1" and "NOT an MSI call" in lines[1] and "germline" in "".join(lines[1:5])
    assert lines[5:10] == ["#min_tract\t10", "#min_units\t5", "#max_unit\t6", "#min_depth\t30", "#unstable_permille\t200"]
    assert lines[10].split("\t")[:11] == ["#chrom", "beg", "end", "unit", "unitlen", "units", "target", "flags", "b_depth", "b_shifted", "b_other"] and len(lines[10].split("\t")) == 8 + 4 * 15
    assert lines[10].split("\t")[11:23] == ["b_m6", "b_m5", "b_m4", "b_m3", "b_m2", "b_m1", "b_p1", "b_p2", "b_p3", "b_p4", "b_p5", "b_p6"]
    ca = "chr1\t120\t144\tCA\t2\t12\texon 1\t.\t60\t12\t0\t2\t0\t0\t0\t0\t8\t0\t0\t0\t0\t0\t2\t50\t9\t3\t0\t0\t0\t0\t9\t0\t0\t0\t0\t0\t0\t0\t40\t7\t0" + "\t0" * 5 + "\t7" + "\t0" * 6 + "\t30\t5\t0" + "\t0" * 5 + "\t5" + "\t0" * 6
    assert lines[11] == ca
    assert lines[12].split("\t")[:11] == ["chr1", "300", "315", "A", "1", "15", "exon 1", ".", "100", "19", "7"]
    assert lines[13] == "chr2\t0\t12\tAAG\t3\t4\t.\tEDGE" + "\t0" * 60
    # assessable: depth >= 30 without EDGE; unstable: 1000 * shifted >= 200 * depth.  b: 12/60 = 200 is in, 19/100 is out; c: 9/50 is out,
    # 8/40 is in; c2: 7/40 is out, 6/30 is in; d: the A tract has depth 29 and is not assessable, 5/30 is out
    assert lines[14:] == ["#summary\tloci\t3", "#summary\tloci_EDGE\t1", "#summary\tb\tassessable\t2\tunstable\t1", "#summary\tc\tassessable\t2\tunstable\t1",
                          "#summary\tc2\tassessable\t2\tunstable\t1", "#summary\td\tassessable\t1\tunstable\t0"]
    assert gzip.open(tmp_path / "m.tsv.gz", "rt").read() == text and open(tmp_path / "m.tsv.gz", "rb").read()[12:16] == b"BC\x02\x00"
    assert subprocess.run(["gzip", "-dc", str(tmp_path / "m.tsv.gz")], capture_output=True, text=True).stdout == text
    with uio.Msi(12, 3, 4, 100, 0) as s:                                             # another request; a store without loci still writes its head
        s.add_target("chrX", 5, 50)
        s.write(str(tmp_path / "e.tsv"))
    assert open(tmp_path / "e.tsv").read() == mr.report_text([("chrX", 5, 50, None)], [[]], 12, 3, 4, 100, 0)


# ------------------------------------------------------------------------------------------------ the command line
def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_six_options_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in [("--msi-out", '""')] + SUB:
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


@pytest.mark.parametrize("args,both", [
    (PAIR + ["-R", "p.bed"] + OUT, ("--msi-out", "--normal-bam")),
    (BASE + ["-R", "p.bed"] + OUT + ["--shard", "1/2"], ("--msi-out", "--shard")),
    (BASE + ["--msi-out=m.tsv", "--shard=0/3"], ("--msi-out", "--shard")),
    (BASE + OUT + ["--repeat", "2"], ("--msi-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT, ("--msi-out", "/only-print-vcf-header/")),
    (BASE + ["--msi-out="], ("--msi-out", "path")),
] + [(PAIR + [o, v], (o, "--normal-bam")) for o, v in SUB] + [(BASE + [o, v], (o, "--msi-out")) for o, v in SUB])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


# (0 thousandths is a value of --msi-unstable-permille: every assessable locus counts)
@pytest.mark.parametrize("opt,bad", [(o, b) for o, _ in SUB for b in ["0", "-5", "true", "1.5", "x", "", "1,2", "3e10"] if (o, b) != ("--msi-unstable-permille", "0")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The other reports and what they allow are not refused, with or without a BED file: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c.tsv", "--callable-out", "c.bed", "--error-profile-out", "e.tsv", "--merge-regions", "2000", "--score-mem-mb", "64", "--devices", "0",
                          "-t", "2", "--shard", "0/1", "--repeat", "1", "--msi-min-tract", "12", "--msi-min-units", "3", "--msi-max-unit", "4", "--msi-min-depth", "100", "--msi-unstable-permille", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--msi" not in r.stderr, r.stderr
    r = run(BASE + ["--msi-out", "m.tsv.gz", "--tumor-vcf", "t.vcf.gz", "--tile", "1000", "--devices", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--msi" not in r.stderr, r.stderr
