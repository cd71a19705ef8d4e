"""The background error profile without a device: --error-profile-out, --error-profile-min-depth and --error-profile-max-alt-permille are CLI
options, their refusals come before any file or device is opened, malformed values are refused, the levels are the table of
include/uvc_errprofile.def, and the store of the reader library (uvcio_errprofile_*) sums the profiles that tiles report and writes the text."""
import ctypes as C
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

import errprofile_restatement as er
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
NLEVEL, ROW = _ffi.ENUMS["UVC_NERRLEVEL"], _ffi.ENUMS["UVC_ERR_ROW"]
OUT = ["--error-profile-out", "e.tsv"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_three_options_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--error-profile-out", '""'), ("--error-profile-min-depth", "20"), ("--error-profile-max-alt-permille", "50")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


def test_the_levels_and_the_row_are_the_table_of_the_issue():
    E = _ffi.ENUMS
    assert region.ERROR_LEVELS == ["bDP", "cDP1", "cDP12", "cDP2", "dDP1"] and NLEVEL == 5 and ROW == 712
    assert [E["UVC_ERRLEVEL_" + n] for n in region.ERROR_LEVELS] == [0, 1, 2, 3, 4]
    assert (er.BASE_BINS, er.LINK_BINS, er.COUNTERS) == (0, 256, 704)
    assert [E["UVC_ERRC_" + n] for n in er.COUNTER_NAMES] == list(range(7)) and E["UVC_ERRC_reserved"] == 7
    table = [l.split("(")[1].rstrip(")\n").replace(" ", "").split(",") for l in open(os.path.join(_ffi.ROOT, "include", "uvc_errprofile.def")) if l.startswith("UVC_ERRLEVEL(")]
    assert table == [[n, g, p] for n, (g, p) in zip(region.ERROR_LEVELS, er.LEVEL_PLANES)]
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_error_level_name.restype, dll.uvcgpu_error_level_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_error_level_name(i).decode() for i in range(NLEVEL)] == region.ERROR_LEVELS
    assert dll.uvcgpu_error_level_name(-1) is None and dll.uvcgpu_error_level_name(NLEVEL) is None


@pytest.mark.parametrize("args,both", [
    (["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"] + OUT, ("--error-profile-out", "--normal-bam")),
    (["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz", "--error-profile-min-depth", "5"], ("--error-profile-min-depth", "--normal-bam")),
    (BASE + OUT + ["--shard", "1/2"], ("--error-profile-out", "--shard")),
    (BASE + ["--error-profile-out=e.tsv", "--shard=0/3"], ("--error-profile-out", "--shard")),
    (BASE + OUT + ["--repeat", "2"], ("--error-profile-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT, ("--error-profile-out", "/only-print-vcf-header/")),
    (BASE + ["--error-profile-min-depth", "5"], ("--error-profile-min-depth", "--error-profile-out")),
    (BASE + ["--error-profile-max-alt-permille", "5"], ("--error-profile-max-alt-permille", "--error-profile-out")),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """--coverage-out and what it allows are not refused: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c.tsv", "--merge-regions", "2000", "--score-mem-mb", "64", "--devices", "0", "-t", "2", "-A", "--force-sites", "s.bed",
                          "--shard", "0/1", "--repeat", "1", "--error-profile-min-depth", "1", "--error-profile-max-alt-permille", "1000"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--error-profile" not in r.stderr, r.stderr
    r = run(BASE + ["--error-profile-out", "e.tsv.gz", "--error-profile-max-alt-permille=0", "--tumor-vcf", "t.vcf.gz", "--tile", "1000", "--devices", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--error-profile" not in r.stderr, r.stderr


@pytest.mark.parametrize("opt,bad", [("--error-profile-min-depth", b) for b in ("0", "-5", "true", "1.5", "x", "", "1,2", "3e10")]
                         + [("--error-profile-max-alt-permille", b) for b in ("-1", "1001", "false", "0.5", "x", "", "5%")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []
    r = run(BASE + ["--error-profile-out="], tmp_path)
    assert r.returncode == 2 and "--error-profile-out" in r.stderr


# ------------------------------------------------------------------------------------------------ the store
class Store:
    def __init__(self, min_depth, permille, levels=region.ERROR_LEVELS):
        d = uio.dll()
        d.uvcio_errprofile_open.restype, d.uvcio_errprofile_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32]
        d.uvcio_errprofile_add.restype, d.uvcio_errprofile_add.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
        d.uvcio_errprofile_write.restype, d.uvcio_errprofile_write.argtypes = C.c_int, [C.c_void_p, C.c_char_p]
        d.uvcio_errprofile_close.restype, d.uvcio_errprofile_close.argtypes = None, [C.c_void_p]
        self.d, self.h = d, C.c_void_p()
        names = (C.c_char_p * len(levels))(*[m.encode() for m in levels])
        assert d.uvcio_errprofile_open(C.byref(self.h), names, len(levels), min_depth, permille) == 0

    def add(self, p):
        p = np.ascontiguousarray(p, dtype=np.int64)
        assert p.shape == (NLEVEL, ROW)
        return self.d.uvcio_errprofile_add(self.h, p.ctypes.data)

    def write(self, path):
        return self.d.uvcio_errprofile_write(self.h, str(path).encode())

    def close(self):
        self.d.uvcio_errprofile_close(self.h)


def test_pieces_from_several_threads_add_to_the_bytes_of_their_sum(tmp_path):
    rng = np.random.default_rng(5)
    pieces = [np.where(rng.random((NLEVEL, ROW)) < 0.3, rng.integers(0, 1 << 40, (NLEVEL, ROW)), 0) for _ in range(24)]
    one, many = Store(20, 50), Store(20, 50)
    assert one.add(sum(pieces)) == 0
    order = rng.permutation(len(pieces)).tolist()
    th = [threading.Thread(target=lambda k=k: [many.add(pieces[i]) for i in order[k::4]]) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert one.write(tmp_path / "one.tsv") == 0 and many.write(tmp_path / "many.tsv") == 0
    assert (tmp_path / "one.tsv").read_bytes() == (tmp_path / "many.tsv").read_bytes()
    assert (tmp_path / "one.tsv").read_text() == er.report_text(region.ERROR_LEVELS, sum(pieces), 20, 50)
    assert one.d.uvcio_errprofile_add(one.h, None) != 0
    one.close()
    many.close()


def test_the_text_of_a_hand_built_profile(tmp_path):
    p = np.zeros((NLEVEL, ROW), np.int64)
    acg, tta = 16 * 0 + 4 * 1 + 2, 16 * 3 + 4 * 3 + 0
    p[0, er.BASE_BINS + acg * 4:er.BASE_BINS + acg * 4 + 4] = [3, 9000000000, 0, 7]       # bDP, A[C]G: ref C; C>A 3, C>T 7
    p[4, er.LINK_BINS + tta * 7:er.LINK_BINS + tta * 7 + 7] = [500, 0, 0, 2, 0, 0, 1]     # dDP1, T[T]A: one D1 twice, one I1
    p[0, er.COUNTERS:er.COUNTERS + 7] = [11, 12, 13, 14, 15, 16, 17]
    p[1:, er.C["no_context"]] = 17
    s = Store(3, 250)
    assert s.add(p) == 0
    plain, gz = tmp_path / "e.tsv", tmp_path / "e.tsv.gz"
    assert s.write(plain) == 0 and s.write(gz) == 0
    s.close()
    counters = "".join("%s\t%s\t%d\n" % (lv, c, (v if lv == "bDP" else (17 if c == "no_context" else 0)))
                       for lv in region.ERROR_LEVELS for c, v in zip(er.COUNTER_NAMES, [11, 12, 13, 14, 15, 16, 17]))
    want = ("##error_profile_min_depth=3\n##error_profile_max_alt_permille=250\n#level\tcounter\tcount\n" + counters
            + "#level\tkind\tcontext\tsymbol\tcount\tref_count\n"
            + "bDP\tBASE\tACG\tA\t3\t9000000000\nbDP\tBASE\tACG\tC\t9000000000\t9000000000\nbDP\tBASE\tACG\tG\t0\t9000000000\nbDP\tBASE\tACG\tT\t7\t9000000000\n"
            + "".join("dDP1\tLINK\tTTA\t%s\t%d\t500\n" % (k, v) for k, v in zip(["M", "D3P", "D2", "D1", "I3P", "I2", "I1"], [500, 0, 0, 2, 0, 0, 1])))
    text = plain.read_text()
    assert text == want
    assert gzip.open(gz, "rt").read() == text
    assert open(gz, "rb").read()[12:16] == b"BC\x02\x00"                    # block-gzipped: the BGZF extra field
    assert text == er.report_text(region.ERROR_LEVELS, p, 3, 250)


def test_write_fails_with_a_message_where_the_file_cannot_be_made(tmp_path):
    s = Store(20, 50)
    assert s.write(tmp_path / "no_such_dir" / "e.tsv") != 0 and "cannot create" in uio.dll().uvcio_last_error().decode()
    assert s.write(tmp_path / "no_such_dir" / "e.tsv.gz") != 0 and "cannot create" in uio.dll().uvcio_last_error().decode()
    s.close()
