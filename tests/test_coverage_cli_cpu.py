"""The per-target coverage report without a device: --coverage-out, --coverage-thresholds and --coverage-window are CLI options, their
refusals come before any file or device is opened, malformed threshold lists are refused, and the report store of the reader library
(uvcio_coverage_*) merges the pieces that tiles report for a target and writes the rows in target order."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
NCOV, ROW = _ffi.ENUMS["UVC_NCOV"], _ffi.ENUMS["UVC_COV_ROW"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_three_options_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--coverage-out", '""'), ("--coverage-thresholds", "1,20,100,500"), ("--coverage-window", "0")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


def test_the_measures_are_the_table_of_the_issue():
    assert region.COVERAGE_MEASURES == ["aDP", "bDP", "cDP1", "cDP12", "cDP2", "dDP1"] and NCOV == 6 and ROW == 11
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_coverage_measure_name.restype, dll.uvcgpu_coverage_measure_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_coverage_measure_name(i).decode() for i in range(NCOV)] == region.COVERAGE_MEASURES
    assert dll.uvcgpu_coverage_measure_name(-1) is None and dll.uvcgpu_coverage_measure_name(NCOV) is None


@pytest.mark.parametrize("args,both", [
    (["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz", "-R", "p.bed", "--coverage-out", "c.tsv"], ("--coverage-out", "--normal-bam")),
    (BASE + ["-R", "p.bed", "--coverage-out", "c.tsv", "--shard", "1/2"], ("--coverage-out", "--shard")),
    (BASE + ["-R", "p.bed", "--coverage-out=c.tsv", "--shard=0/3"], ("--coverage-out", "--shard")),
    (BASE + ["-R", "p.bed", "--coverage-out", "c.tsv", "--repeat", "2"], ("--coverage-out", "--repeat")),
    (["/only-print-vcf-header/", "--coverage-out", "c.tsv", "--coverage-window", "1000"], ("--coverage-out", "/only-print-vcf-header/")),
    (BASE + ["--coverage-thresholds", "1,5"], ("--coverage-thresholds", "--coverage-out")),
    (BASE + ["--coverage-window", "1000"], ("--coverage-window", "--coverage-out")),
    (BASE + ["--coverage-out", "c.tsv"], ("--coverage-out", "--coverage-window")),                       # no BED file: windows are required
    (BASE + ["--coverage-out", "c.tsv", "-R", "p.bed", "--coverage-window", "1000"], ("--coverage-window", "-R")),
    (BASE + ["--coverage-out", "c.tsv", "--bed-in-fname", "p.bed", "--coverage-window", "1000"], ("--coverage-window", "--bed-in-fname")),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """--tumor-vcf, --force-sites, --merge-regions, --score-mem-mb, --devices, -t and -A are not refused: the run fails on the missing BAM."""
    r = run(BASE + ["-R", "p.bed", "--coverage-out", "c.tsv", "--merge-regions", "2000", "--score-mem-mb", "64", "--devices", "0", "-t", "2", "-A", "--force-sites", "s.bed",
                    "--shard", "0/1", "--repeat", "1", "--coverage-thresholds", "0,1,2,3,4,5,6,7"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--coverage" not in r.stderr, r.stderr
    r = run(BASE + ["--coverage-window", "500", "--coverage-out", "c.tsv.gz", "--tumor-vcf", "t.vcf.gz", "--devices", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--coverage" not in r.stderr, r.stderr


@pytest.mark.parametrize("bad", ["1,2,3,4,5,6,7,8,9", "100,20,1", "1,20,20", "-1,5", "1,,2", "true", "1,true", "", "1,2.5", "1, 2", "a", "1,2,"])
def test_malformed_threshold_lists_are_refused(tmp_path, bad):
    r = run(BASE + ["-R", "p.bed", "--coverage-out", "c.tsv", "--coverage-thresholds=" + bad], tmp_path)
    assert r.returncode == 2 and "--coverage-thresholds" in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("bad", ["0", "-5", "true", "1.5", "x", ""])
def test_malformed_windows_are_refused(tmp_path, bad):
    r = run(BASE + ["--coverage-out", "c.tsv", "--coverage-window=" + bad], tmp_path)
    assert r.returncode == 2 and "--coverage-window" in r.stderr, (bad, r.stderr)


# ------------------------------------------------------------------------------------------------ the report store
class Report:
    def __init__(self, thresholds, measures=region.COVERAGE_MEASURES):
        d = uio.dll()
        d.uvcio_coverage_open.restype, d.uvcio_coverage_open.argtypes = C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int32, C.c_void_p, C.c_int32]
        d.uvcio_coverage_add_target.restype, d.uvcio_coverage_add_target.argtypes = C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int64]
        d.uvcio_coverage_add_piece.restype, d.uvcio_coverage_add_piece.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        d.uvcio_coverage_write.restype, d.uvcio_coverage_write.argtypes = C.c_int, [C.c_void_p, C.c_char_p]
        d.uvcio_coverage_close.restype, d.uvcio_coverage_close.argtypes = None, [C.c_void_p]
        self.d, self.h = d, C.c_void_p()
        names = (C.c_char_p * len(measures))(*[m.encode() for m in measures])
        thr = np.ascontiguousarray(thresholds, dtype=np.int32)
        assert d.uvcio_coverage_open(C.byref(self.h), names, len(measures), thr.ctypes.data, len(thr)) == 0

    def target(self, chrom, beg, end, name, length):
        return self.d.uvcio_coverage_add_target(self.h, chrom.encode(), beg, end, name.encode() if name is not None else None, length)

    def piece(self, target, length, row):
        row = np.ascontiguousarray(row, dtype=np.int64)
        assert row.shape == (NCOV, ROW)
        return self.d.uvcio_coverage_add_piece(self.h, target, length, row.ctypes.data)

    def write(self, path):
        rc = self.d.uvcio_coverage_write(self.h, str(path).encode())
        return rc

    def close(self):
        self.d.uvcio_coverage_close(self.h)


def row_of(depths, thresholds):
    """What uvcgpu_region_coverage returns for one range whose per-position depths of every measure are `depths` [NCOV][len]."""
    depths = np.asarray(depths, dtype=np.int64)
    row = np.zeros((NCOV, ROW), np.int64)
    row[:, 0], row[:, 1], row[:, 2] = depths.sum(1), depths.min(1), depths.max(1)
    for k, t in enumerate(thresholds):
        row[:, 3 + k] = (depths >= t).sum(1)
    return row


def test_pieces_merge_to_the_rows_of_the_whole_target(tmp_path):
    rng = np.random.default_rng(3)
    thr = [0, 1, 20, 100]
    rep = Report(thr)
    depth = {"t0": rng.integers(0, 150, (NCOV, 700)), "t1": rng.integers(5, 30, (NCOV, 40)), "t2": rng.integers(1, 9, (NCOV, 10))}
    assert rep.target("chr1", 100, 800, "exonA", 700) == 0
    assert rep.target("chr2", 5, 45, None, 40) == 1
    assert rep.target("chr2", 50, 60, "", 10) == 2
    assert rep.target("chrM", 16000, 17000, "past_the_end", 569) == 3        # nothing is ever reported for it
    assert rep.target("chrM", 0, 0, "empty", 0) == 4
    # t0 in four pieces, reported out of order as workers finish; t1 whole; t2 only partly covered (its other positions count as depth 0)
    cuts = [(300, 700), (0, 1), (1, 120), (120, 300)]
    for a, b in cuts:
        assert rep.piece(0, b - a, row_of(depth["t0"][:, a:b], thr)) == 0
    assert rep.piece(1, 40, row_of(depth["t1"], thr)) == 0
    assert rep.piece(2, 6, row_of(depth["t2"][:, 2:8], thr)) == 0
    # refused: a piece that would make the pieces longer than the target, a target that does not exist, an empty piece
    assert rep.piece(1, 1, row_of(depth["t1"][:, :1], thr)) != 0 and "target 1" in uio.dll().uvcio_last_error().decode()
    assert rep.piece(9, 1, row_of(depth["t1"][:, :1], thr)) != 0
    assert rep.piece(0, 0, row_of(depth["t1"][:, :1], thr)) != 0
    plain, gz = tmp_path / "c.tsv", tmp_path / "c.tsv.gz"
    assert rep.write(plain) == 0 and rep.write(gz) == 0
    rep.close()
    text = plain.read_text()
    assert gzip.open(gz, "rt").read() == text
    assert open(gz, "rb").read()[12:16] == b"BC\x02\x00"                    # block-gzipped: the BGZF extra field
    lines = text.splitlines()
    head = ["#chrom", "beg", "end", "name", "len"] + [m + s for m in region.COVERAGE_MEASURES for s in ["_sum", "_min", "_max"] + ["_ge%d" % t for t in thr]]
    assert lines[0].split("\t") == head and len(lines) == 6

    def want(chrom, beg, end, name, length, depths):
        d = np.zeros((NCOV, length), np.int64)
        d[:, :depths.shape[1]] = depths                                     # unreported positions: depth 0
        r = row_of(d, thr) if length else np.zeros((NCOV, ROW), np.int64)
        return [chrom, str(beg), str(end), name, str(length)] + [str(v) for v in r[:, :3 + len(thr)].reshape(-1)]
    assert lines[1].split("\t") == want("chr1", 100, 800, "exonA", 700, depth["t0"])
    assert lines[2].split("\t") == want("chr2", 5, 45, ".", 40, depth["t1"])
    assert lines[3].split("\t") == want("chr2", 50, 60, ".", 10, depth["t2"][:, 2:8])
    assert lines[4].split("\t") == want("chrM", 16000, 17000, "past_the_end", 569, np.zeros((NCOV, 0), np.int64))
    assert lines[5].split("\t") == want("chrM", 0, 0, "empty", 0, np.zeros((NCOV, 0), np.int64))
    assert all(f.lstrip("-").isdigit() for l in lines[1:] for f in l.split("\t")[4:])


def test_write_fails_with_a_message_where_the_file_cannot_be_made(tmp_path):
    rep = Report([1])
    assert rep.write(tmp_path / "no_such_dir" / "c.tsv") != 0 and "cannot create" in uio.dll().uvcio_last_error().decode()
    assert rep.write(tmp_path / "no_such_dir" / "c.tsv.gz") != 0 and "cannot create" in uio.dll().uvcio_last_error().decode()
    rep.close()
