"""The streamed score without a device: the five entry points are exported and the ctypes mirror matches the header, --score-mem-mb is a
[CLI] option whose refusals come before any file or device is opened, the per-record footprint is stated by the library (no device
needed: a layout constant), and the oracle binding knows nothing of streams (it is called once and compared with the concatenation)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from uvc_amd import _ffi, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
SYMBOLS = ("uvcgpu_region_score_stream_begin", "uvcgpu_score_stream_next", "uvcgpu_score_stream_end", "uvcgpu_score_stream_bytes_per_record", "uvcgpu_score_stream_footprint")


def run(args, cwd=None):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=cwd)


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(_ffi.ROOT, "include", "uvcgpu.h")).read(), flags=re.S)


def test_the_five_symbols_are_exported_and_declared():
    dll = C.CDLL(_ffi.gpu_library_path())
    hdr = header()
    for name in SYMBOLS:
        assert hasattr(dll, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    # the declarations, argument by argument
    flat = " ".join(hdr.split())
    assert "typedef struct uvcgpu_score_stream uvcgpu_score_stream_t;" in flat
    assert ("int uvcgpu_region_score_stream_begin(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, "
            "int64_t chunk_records, uvcgpu_score_stream_t **out);") in flat
    assert "int uvcgpu_score_stream_next(uvcgpu_score_stream_t *s, UvcScoreOut *chunk, UvcScoreRange *covered, int64_t *n_covered);" in flat
    assert "int uvcgpu_score_stream_end(uvcgpu_score_stream_t *s);" in flat
    assert "int64_t uvcgpu_score_stream_bytes_per_record(void);" in flat
    assert "int64_t uvcgpu_score_stream_footprint(const uvcgpu_region_t *r);" in flat


def test_the_ctypes_mirror_matches_the_header():
    # the structs a stream hands over are the ones of the one call, unchanged: the chunk is a UvcScoreOut, the covered ranges UvcScoreRange
    assert C.sizeof(_ffi.UvcScoreOut) == 24 and [f[0] for f in _ffi.UvcScoreOut._fields_] == ["capacity", "n_records", "fields"]
    assert C.sizeof(_ffi.UvcScoreRange) == 16
    assert C.sizeof(_ffi.UvcScoreRequest) == 96
    # the end-of-stream code is distinct from success and from every error
    E = _ffi.ENUMS
    assert E["UVCGPU_STREAM_END"] == 1
    assert E["UVCGPU_STREAM_END"] not in [v for k, v in E.items() if k.startswith("UVCGPU_E")] and E["UVCGPU_ESTATE"] == -5 and E["UVCGPU_ENOMEM"] == -6
    # the Python generator binds the three calls with the header's argument lists
    src = open(os.path.join(_ffi.ROOT, "uvc_amd", "region.py")).read()
    assert '"region_score_stream_begin", C.c_int, [C.c_void_p, C.POINTER(_ffi.UvcScoreRequest), C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]' in src
    assert '"score_stream_next", C.c_int, [C.c_void_p, C.POINTER(_ffi.UvcScoreOut), C.c_void_p, C.POINTER(C.c_int64)]' in src
    assert '"score_stream_end", C.c_int, [C.c_void_p]' in src
    assert hasattr(region.Region, "score_stream")


def test_bytes_per_record():
    """Two row sets and two page-locked buffers: at least 2 x 640 B of records per unit of chunk_records, and the rows on top."""
    dll = C.CDLL(_ffi.gpu_library_path())
    fn = dll.uvcgpu_score_stream_bytes_per_record
    fn.restype, fn.argtypes = C.c_int64, []
    b = fn()
    rec = 4 * _ffi.NUM_SCORE_FIELDS
    assert b > 0 and b >= 2 * 640 and b >= 2 * rec
    assert b >= 2 * 3 * rec                                                 # records, their kept_only copy and the host buffer, twice
    assert b < 2 * 3 * rec + 2 * 4096                                       # and rows of the order DESIGN.md states (about 1.4 KB per record and set)
    fp = dll.uvcgpu_score_stream_footprint
    fp.restype, fp.argtypes = C.c_int64, [C.c_void_p]
    assert fp(None) == -1


def test_help_lists_the_option_as_cli():
    r = run(["--help"])
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("  --score-mem-mb ")]
    assert len(line) == 1 and line[0].split()[1] == "[CLI]" and "default=0" in line[0], line
    assert "MiB" in line[0] and "per worker" in line[0]
    timing = [l for l in r.stdout.splitlines() if l.startswith("  --timing ")]
    assert len(timing) == 1 and "chunks per tile" in timing[0]


@pytest.mark.parametrize("args", [
    ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "-A", "--score-mem-mb", "-5"],
    ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--score-mem-mb=-1"],
    ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--score-mem-mb", "lots"],
    ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--score-mem-mb", "1.5"],
    ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--score-mem-mb=true"],
    ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--score-mem-mb", ""],
    ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz", "--score-mem-mb", "-64"],
])
def test_bad_values_exit_2_before_any_file_or_device(tmp_path, args):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--score-mem-mb" in r.stderr and "MiB" in r.stderr, r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "o.vcf.gz") and not os.path.exists(tmp_path / "n.vcf.gz") and not os.path.exists(tmp_path / "t.vcf.gz")


def test_a_good_value_goes_on_to_the_files(tmp_path):
    """0 (the default, spelled out) and a size are accepted: the run goes on as without the option (here: --print-params needs no file)."""
    for v in ("0", "512"):
        r = run(["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--score-mem-mb", v, "--print-params", "--sequencing-platform", "1"], cwd=str(tmp_path))
        assert r.returncode == 0 and "--score-mem-mb" not in r.stderr, (v, r.stderr)


def test_the_oracle_binding_has_no_stream():
    """The oracle is called once and compared with the concatenation of the chunks: it needs no stream and exports none."""
    path = __import__("oracle").library_path()
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(_ffi.ROOT, "oracle")])
    lib = _ffi.Lib(path, "uvc_oracle_")
    for name in SYMBOLS:
        tail = name[len("uvcgpu_"):]
        assert not hasattr(lib.dll, "uvc_oracle_" + tail) and not hasattr(lib.dll, "uvc_oracle_" + tail.replace("region_", "")), name
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    assert "stream" not in out
