"""The read profile without a device: the restatement of the definitions (tests/readprofile_restatement.py) on hand-made reads with every
expected word written out, the identities of a row, the store of the reader library (uvcio_readprofile_*), and the command line options
with their refusals, which come before any file or device is opened."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import readprofile_restatement as rr
from test_bq_correction import make_reads
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--read-profile-out", "r.tsv"]
GATE_OPTS = ["--read-profile-min-mapq", "--read-profile-min-depth", "--read-profile-max-alt-permille"]
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
BEG, REF_LEN = 1_000_000, 400


def hand_made(specs, mapq=None, ref_edit=None):
    """make_reads of the BQ-correction test (one read per spec: offset, flag, cigar, bases, quals) with bases given as offsets against
    the reference: None = the reference base, k = (reference + k) % 4, "N" = N; aligned bases only, the others are plain codes."""
    r = make_reads(specs, beg=BEG, ref_len=REF_LEN)
    if mapq is not None:
        r["mapq"] = np.array(mapq, np.uint8)
    if ref_edit:
        s = list(r["refseq"])
        for at, ch in ref_edit.items():
            s[at] = ch
        r["refseq"] = "".join(s)
    return r


def ref_codes(n=REF_LEN):
    return [int(v) for v in np.random.default_rng(0).integers(0, 4, n)]   # the reference string of make_reads


REF = ref_codes()


def row_of(words):
    row = np.zeros(rr.ROW, np.int64)
    for k, v in words.items():
        row[k] = v
    return row


def q_(c, qb, k):
    return rr.Q_BINS + (c * 64 + qb) * 2 + k


def cyc_(c, cb, kind):
    return rr.CYC_BINS + (c * 256 + cb) * 5 + kind


def sub_(c, ref, read):
    return rr.SUB_BINS + c * 16 + ref * 4 + read


def add(words, key, v=1):
    words[key] = words.get(key, 0) + v


WHOLE = [(BEG, BEG + REF_LEN + 1)]


def test_soft_clips_hard_clip_and_the_cycle_direction_of_a_reverse_read_2():
    # read 0: forward R1 at offset 10, 2S 4M 3S; matches everywhere but the third aligned base
    b0 = [0, 0] + [REF[10], REF[11], (REF[12] + 1) % 4, REF[13]] + [3, 3, 3]
    # read 1: reverse R2 (flag 0x90) at offset 50, 2H 1S 3M 2H: l_qseq 4, the cycles run down from 3
    b1 = [2] + [REF[50], REF[51], REF[52]]
    r = hand_made([(10, 0x0, [(S, 2), (M, 4), (S, 3)], b0, [30, 30, 31, 32, 33, 34, 2, 2, 2]),
                   (50, 0x90, [(H, 2), (S, 1), (M, 3), (H, 2)], b1, [70, 40, 41, 63])])
    got = rr.Restatement(r).row(WHOLE, 0, 1, 1000)
    w = {}
    for k, (q, mis) in enumerate([(31, 0), (32, 0), (33, 1), (34, 0)]):      # read 0: query 2..5 = cycles 2..5
        add(w, q_(0, q, mis)); add(w, cyc_(0, 2 + k, mis))
        add(w, sub_(0, REF[10 + k], b0[2 + k]))
    for cyc in (0, 1, 6, 7, 8):                                               # its clips: the leading one anchored at pos, the trailing one at the last aligned position
        add(w, cyc_(0, cyc, 4))
    for k, q in enumerate([40, 41, 63]):                                      # read 1, class 3: query 1..3 = cycles 2, 1, 0; quality 63 is the last bin
        add(w, q_(3, q, 0)); add(w, cyc_(3, 2 - k, 0)); add(w, sub_(3, REF[50 + k], REF[50 + k]))
    add(w, cyc_(3, 3, 4))                                                     # its one soft-clipped base at cycle 3; the hard clips count nowhere
    w[rr.C["bases_clean"]] = 7
    w[rr.C["positions_no_ref"]], w[rr.C["positions_low_depth"]], w[rr.C["positions_clean"]] = 1, REF_LEN - 7, 7
    assert np.array_equal(got, row_of(w)), [(int(i), int(got[i]), int(row_of(w)[i])) for i in np.flatnonzero(got != row_of(w))]
    rr.check_identities(got, REF_LEN + 1)
    # quality 70 of the clipped base is nowhere: clips have no quality bin


def test_insertion_behind_a_clip_deletion_skip_and_anchors_outside_the_range():
    # forward R2 (0x80) at offset 100: 1S 2I 3M 2D 2M 5N 1M 1I 1M, l_qseq 11
    aligned = [100, 101, 102, 105, 106, 112, 113]
    b = [1] + [2, 2] + [REF[p] for p in aligned[:3]] + [REF[105], REF[106]] + [REF[112]] + [0] + [REF[113]]
    cg = [(S, 1), (I, 2), (M, 3), (D, 2), (M, 2), (N, 5), (M, 1), (I, 1), (M, 1)]
    r = hand_made([(100, 0x80, cg, b, [20] * 11)])
    rs = rr.Restatement(r)
    got = rs.row(WHOLE, 0, 1, 1000)
    w = {}
    for cyc, p in zip([3, 4, 5, 6, 7, 8, 10], aligned):
        add(w, q_(2, 20, 0)); add(w, cyc_(2, cyc, 0)); add(w, sub_(2, REF[p], REF[p]))
    add(w, cyc_(2, 0, 4))            # the clip: anchor max(pos, pos - 1) = 100
    add(w, cyc_(2, 1, 2)); add(w, cyc_(2, 2, 2))   # the insertion in front of the first aligned base: anchor 100 as well
    add(w, cyc_(2, 5, 3))            # the deletion at 103: one event at the cycle of the query base in front of it (query 5)
    add(w, cyc_(2, 9, 2))            # the second insertion (query 9): anchor 112
    w[rr.C["bases_clean"]] = 7
    w[rr.C["positions_no_ref"]], w[rr.C["positions_low_depth"]], w[rr.C["positions_clean"]] = 1, REF_LEN - 7, 7
    assert np.array_equal(got, row_of(w)), [(int(i), int(got[i]), int(row_of(w)[i])) for i in np.flatnonzero(got != row_of(w))]
    # a range from 101 on: the clip and the first insertion (anchor 100) and the base at 100 are outside; the deletion's anchor 103 is outside
    # [104, 113) too, the second insertion's anchor 112 inside
    part = rs.row([(BEG + 104, BEG + 113)], 0, 1, 1000)
    w = {}
    for cyc, p in zip([6, 7, 8], [105, 106, 112]):
        add(w, q_(2, 20, 0)); add(w, cyc_(2, cyc, 0)); add(w, sub_(2, REF[p], REF[p]))
    add(w, cyc_(2, 9, 2))
    w[rr.C["bases_clean"]] = 3
    w[rr.C["positions_low_depth"]], w[rr.C["positions_clean"]] = 6, 3
    assert np.array_equal(part, row_of(w)), [(int(i), int(part[i]), int(row_of(w)[i])) for i in np.flatnonzero(part != row_of(w))]
    rr.check_identities(part, 9)
    # rows of disjoint position sets add
    assert np.array_equal(rs.row([(BEG, BEG + 104)], 0, 1, 1000) + part + rs.row([(BEG + 113, BEG + REF_LEN + 1)], 0, 1, 1000), got)


def test_n_base_reference_n_low_mapq_and_the_gates():
    # three forward R1 reads over offsets 200..203; read 1 has an N base at 201 and a mismatch at 202; read 2 has mapq 5; the reference has an N at 203
    same = [REF[200], REF[201], REF[202], REF[203]]
    r = hand_made([(200, 0, [(M, 4)], same, [30] * 4), (200, 0, [(M, 4)], [same[0], 4, (same[2] + 2) % 4, same[3]], [10, 11, 12, 13]), (200, 0x10, [(M, 4)], same, [40] * 4)],
                  mapq=[60, 60, 5], ref_edit={203: "N"})
    rs = rr.Restatement(r)
    st, Dp, Xp = rs.status(10, 2, 500)
    assert Dp[200:204].tolist() == [2, 1, 2, 2] and Xp[200:203].tolist() == [0, 0, 1]   # (X under the reference N decides nothing)
    assert st[200:204].tolist() == [rr.CLEAN, rr.LOW_DEPTH, rr.CLEAN, rr.NO_REF] and st[REF_LEN] == rr.NO_REF
    got = rs.row([(BEG + 200, BEG + 204)], 10, 2, 500)
    w = {rr.C["bases_low_mapq"]: 4, rr.C["bases_no_ref"]: 2, rr.C["bases_n"]: 1, rr.C["bases_low_depth"]: 1, rr.C["bases_clean"]: 4,
         rr.C["positions_clean"]: 2, rr.C["positions_low_depth"]: 1, rr.C["positions_no_ref"]: 1}
    add(w, q_(0, 30, 0), 2); add(w, cyc_(0, 0, 0)); add(w, cyc_(0, 2, 0))                      # read 0 at 200 and 202
    add(w, q_(0, 10, 0)); add(w, cyc_(0, 0, 0)); add(w, q_(0, 12, 1)); add(w, cyc_(0, 2, 1))  # read 1: a match at 200, the mismatch at 202
    add(w, sub_(0, same[0], same[0]), 2); add(w, sub_(0, same[2], same[2])); add(w, sub_(0, same[2], (same[2] + 2) % 4))
    assert np.array_equal(got, row_of(w)), [(int(i), int(got[i]), int(row_of(w)[i])) for i in np.flatnonzero(got != row_of(w))]
    rr.check_identities(got, 4)
    # one mismatch of two bases is 500 permille: not above 500, but above 499 -> high_alt; the N base comes before the depth test
    got = rs.row([(BEG + 200, BEG + 204)], 10, 1, 499)
    assert got[rr.C["positions_high_alt"]] == 1 and got[rr.C["bases_high_alt"]] == 2 and got[rr.C["bases_n"]] == 1 and got[rr.C["bases_clean"]] == 3
    # with every alignment counted the reverse read's bases are class 1 and its cycles run down
    got = rs.row([(BEG + 200, BEG + 201)], 0, 1, 1000)
    assert got[q_(1, 40, 0)] == 1 and got[cyc_(1, 3, 0)] == 1 and got[rr.C["bases_low_mapq"]] == 0 and got[rr.C["bases_clean"]] == 3


def test_long_reads_meet_in_the_last_cycle_bin():
    b = [REF[k] for k in range(300)]
    r = hand_made([(0, 0, [(M, 300)], b, [25] * 300), (0, 0x10, [(M, 300)], b, [25] * 300)])
    got = rr.Restatement(r).row(WHOLE, 0, 1, 1000)
    cyc = rr.sections(got)[1]
    assert cyc[0, :255, 0].tolist() == [1] * 255 and cyc[0, 255, 0] == 45 and cyc[1, 255, 0] == 45 and cyc[1, :255, 0].tolist() == [1] * 255
    rr.check_identities(got, REF_LEN + 1)


# ------------------------------------------------------------------------------------------------ layout and names
def test_the_row_is_the_table_of_the_issue():
    E = _ffi.ENUMS
    assert E["UVC_READPROF_ROW"] == 5712 == rr.ROW
    assert [(n, f, w) for n, f, w in _ffi.READPROF_SECTIONS[:3]] == [("Q", 0, 512), ("CYC", 512, 5120), ("SUB", 5632, 64)]
    assert [n for n, _, _ in _ffi.READPROF_SECTIONS[3:13]] == rr.COUNTER_NAMES and _ffi.READPROF_SECTIONS[13] == ("reserved", 5706, 6)
    assert [f for _, f, _ in _ffi.READPROF_SECTIONS[3:13]] == [rr.C[n] for n in rr.COUNTER_NAMES]
    assert region.READ_CLASSES == rr.CLASSES
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_read_class_name.restype, dll.uvcgpu_read_class_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_read_class_name(i).decode() for i in range(4)] == region.READ_CLASSES
    assert dll.uvcgpu_read_class_name(-1) is None and dll.uvcgpu_read_class_name(4) is None
    assert C.sizeof(_ffi.UvcReadProfileRequest) == 12


# ------------------------------------------------------------------------------------------------ the store
def test_store_sums_rows_and_writes_fixed_text(tmp_path):
    row = np.zeros(rr.ROW, np.int64)
    row[q_(0, 30, 0)], row[q_(0, 30, 1)], row[q_(0, 2, 0)], row[q_(3, 63, 1)] = 9000000000, 7, 5, 1
    row[cyc_(2, 255, 4)], row[cyc_(2, 0, 0)], row[cyc_(1, 17, 3)] = 4, 6, 2
    row[sub_(1, 2, 3)], row[sub_(0, 0, 0)] = 11, 13
    row[rr.COUNTERS:rr.COUNTERS + 10] = np.arange(1, 11)
    with uio.ReadProfile(region.READ_CLASSES, 3, 25, 75) as s:
        s.add(row)
        s.add(row)
        with pytest.raises(ValueError):
            s.add(row[:100])
        plain, gz = tmp_path / "r.tsv", tmp_path / "r.tsv.gz"
        s.write(plain)
        s.write(gz)
        with pytest.raises(Exception, match="cannot create"):
            s.write(tmp_path / "no_such_dir" / "r.tsv")
    want = ("##read_profile_min_mapq=3\n##read_profile_min_depth=25\n##read_profile_max_alt_permille=75\n"
            "##empirical_quality=-10*log10((mismatch+1)/(match+mismatch+2))\n#counter\tcount\n"
            + "".join("%s\t%d\n" % (n, 2 * (k + 1)) for k, n in enumerate(rr.COUNTER_NAMES))
            + "#class\tquality\tmatch\tmismatch\nR1_fwd\t2\t10\t0\nR1_fwd\t30\t18000000000\t14\nR2_rev\t63\t0\t2\n"
            + "#class\tcycle\tmatch\tmismatch\tins\tdel\tclip\nR1_rev\t17\t0\t0\t0\t4\t0\nR2_fwd\t0\t12\t0\t0\t0\t0\nR2_fwd\t255\t0\t0\t0\t0\t8\n"
            + "#class\tref\tread\tcount\nR1_fwd\tA\tA\t26\nR1_rev\tG\tT\t22\n")
    text = plain.read_text()
    assert text == want                                                       # doubled; classes, qualities and cycles ascend; zero bins are left out
    assert gzip.open(gz, "rt").read() == text and open(gz, "rb").read()[12:16] == b"BC\x02\x00"
    assert text == rr.report_text(2 * row, 3, 25, 75)


# ------------------------------------------------------------------------------------------------ command line
def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_four_options_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--read-profile-out", '""'), ("--read-profile-min-mapq", "0"), ("--read-profile-min-depth", "20"), ("--read-profile-max-alt-permille", "50")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]


@pytest.mark.parametrize("args,both", [
    (PAIR + OUT, ("--read-profile-out", "--normal-bam")),
    (PAIR + ["--read-profile-min-mapq", "5"], ("--read-profile-min-mapq", "--normal-bam")),
    (BASE + OUT + ["--shard", "1/2"], ("--read-profile-out", "--shard")),
    (BASE + ["--read-profile-out=r.tsv", "--shard=0/3"], ("--read-profile-out", "--shard")),
    (BASE + OUT + ["--repeat", "2"], ("--read-profile-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT, ("--read-profile-out", "/only-print-vcf-header/")),
] + [(BASE + [g, "5"], (g, "--read-profile-out")) for g in GATE_OPTS])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("opt,bad", [("--read-profile-min-mapq", b) for b in ("-1", "256", "true", "1.5", "x", "")]
                         + [("--read-profile-min-depth", b) for b in ("0", "-5", "true", "1.5", "x", "", "1,2", "3e10")]
                         + [("--read-profile-max-alt-permille", b) for b in ("-1", "1001", "false", "0.5", "x", "", "5%")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The other four reports and what they allow are not refused: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c.tsv", "--error-profile-out", "e.tsv", "--family-stats-out", "f.tsv", "--callable-out", "k.bed", "--merge-regions", "2000",
                          "--score-mem-mb", "64", "--devices", "0", "-t", "2", "--shard", "0/1", "--repeat", "1", "--read-profile-min-mapq", "20", "--read-profile-min-depth", "1",
                          "--read-profile-max-alt-permille", "1000"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--read-profile" not in r.stderr, r.stderr
    r = run(BASE + ["--read-profile-out="], tmp_path)
    assert r.returncode == 2 and "--read-profile-out" in r.stderr
