"""Merged BED regions without a device: the batch planner (uvcio_plan_bed_batches) against a Python restatement on random BED lists,
--merge-regions as a CLI option whose refusals come before any file or device is opened, and the ABI of the ranges call (UvcScoreRange is
16 bytes, UvcScoreRequest is what it was, the new entry points are exported by the HIP library)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")


def restated(tid, beg, end, merge, span):
    """The rule as include/uvcio.h words it, line by line."""
    out, batch, open_batch = [], -1, None          # open_batch: (tid, begin of the batch, end of its last line), None when nothing may join
    for i, (t, b, e) in enumerate(zip(tid, beg, end)):
        if e <= b:
            continue
        if e - b > span:                           # cut as --tile cuts it; every piece alone
            for pb in range(b, e, span):
                batch += 1
                out.append(dict(line=i, batch=batch, tid=t, beg=pb, end=min(pb + span, e)))
            open_batch = None
            continue
        joins = (open_batch is not None and t == open_batch[0] and b >= open_batch[2] + 1 and b - open_batch[2] <= merge and e - open_batch[1] <= span)
        if joins:
            open_batch = (t, open_batch[1], e)
        else:
            batch += 1
            open_batch = (t, b, e)
        out.append(dict(line=i, batch=batch, tid=t, beg=b, end=e))
    return out


def random_bed(rng, kind):
    n = int(rng.integers(0, 120))
    tid = np.sort(rng.integers(0, 3, n)) if kind != "contigs_interleaved" else rng.integers(0, 3, n)
    beg = np.zeros(n, np.int64)
    for t in range(3):
        m = tid == t
        beg[m] = np.sort(rng.integers(0, 50000, int(m.sum())))
    length = rng.integers(0, 400, n)
    if kind == "unsorted":
        beg = rng.permutation(beg)
    if kind == "abutting" and n > 1:                # many lines begin exactly where their predecessor ends, or one base behind
        for i in range(1, n):
            if tid[i] == tid[i - 1] and rng.random() < 0.6:
                beg[i] = beg[i - 1] + length[i - 1] + int(rng.integers(0, 2))
    if kind == "over_long":
        length = np.where(rng.random(n) < 0.2, rng.integers(3000, 20000, n), length)
    return tid.astype(np.int32).tolist(), beg.tolist(), (beg + length).tolist()


@pytest.mark.parametrize("kind", ["sorted", "unsorted", "abutting", "overlapping", "contigs_interleaved", "over_long"])
def test_planner_equals_the_restatement(kind):
    rng = np.random.default_rng(len(kind))
    n_merged = 0
    for _ in range(60):
        tid, beg, end = random_bed(rng, kind)
        merge = int(rng.choice([0, 1, 50, 500, 10 ** 6]))
        span = int(rng.choice([1000, 2500, 10 ** 6]))
        got = uio.plan_bed_batches(tid, beg, end, merge, span)
        want = restated(tid, beg, end, merge, span)
        assert got == want, (kind, merge, span)
        batches = [p["batch"] for p in got]
        assert batches == sorted(batches) and (not batches or (batches[0] == 0 and set(np.diff(batches).tolist()) <= {0, 1}))
        n_merged += len(batches) - len(set(batches))
        if merge == 0:
            assert len(set(batches)) == len(batches)                       # off: one region per line / piece
        for b in set(batches):                                             # inside a batch: one contig, sorted, a base apart, within the span
            ps = [p for p in got if p["batch"] == b]
            assert len(set(p["tid"] for p in ps)) == 1 and ps[-1]["end"] - ps[0]["beg"] <= span
            assert all(q["beg"] >= p["end"] + 1 and q["beg"] - p["end"] <= merge for p, q in zip(ps, ps[1:]))
    assert n_merged > 0 or kind in ("unsorted",)


def test_planner_examples_and_refusals():
    plan = lambda lines, m, s=1000: [(p["line"], p["batch"], p["beg"], p["end"]) for p in uio.plan_bed_batches([l[0] for l in lines], [l[1] for l in lines], [l[2] for l in lines], m, s)]   # noqa: E731
    lines = [(0, 100, 200), (0, 250, 300), (0, 300, 350), (0, 351, 400), (1, 360, 380), (0, 900, 1200), (0, 5000, 7500), (0, 7600, 7700), (0, 7750, 7750)]
    assert plan(lines, 100) == [(0, 0, 100, 200), (1, 0, 250, 300), (2, 1, 300, 350), (3, 1, 351, 400), (4, 2, 360, 380), (5, 3, 900, 1200),
                                (6, 4, 5000, 6000), (6, 5, 6000, 7000), (6, 6, 7000, 7500), (7, 7, 7600, 7700)]
    assert [b for _, b, _, _ in plan(lines[:4], 10 ** 6, 250)] == [0, 0, 1, 1]     # the span cap opens a batch
    assert plan([], 100) == []
    for bad in (dict(m=-1, s=1000), dict(m=10, s=0)):
        with pytest.raises(IOError):
            plan(lines, bad["m"], bad["s"])
    with pytest.raises(IOError, match="line 1"):
        plan([(0, 1, 5), (0, -4, 9)], 10)


def run(args, cwd=None):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=cwd)


def test_help_lists_the_option_as_cli():
    r = run(["--help"])
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("  --merge-regions ")]
    assert len(line) == 1 and line[0].split()[1] == "[CLI]" and "default=0" in line[0], line
    assert "BAQ" in line[0] and "gaps" in line[0]                           # what a merged region does not promise, next to the option


@pytest.mark.parametrize("args,what", [
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--merge-regions", "500"], "BED"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--targets", "chr1", "--merge-regions=500"], "BED"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "-R", "p.bed", "--merge-regions", "500", "--tumor-vcf", "t.vcf.gz"], "--tumor-vcf"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--tumor-vcf=t.vcf.gz", "--bed-in-fname", "p.bed", "--merge-regions=500"], "--tumor-vcf"),
    (["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz", "-R", "p.bed", "--merge-regions", "500"], "--normal-bam"),
    (["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz", "-R", "p.bed", "--merge-regions=500"], "--normal-bam"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "-R", "p.bed", "--merge-regions", "-5"], "distance"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "-R", "p.bed", "--merge-regions", "near"], "distance"),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, what):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = run(args, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--merge-regions" in r.stderr and what in r.stderr, r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "o.vcf.gz") and not os.path.exists(tmp_path / "n.vcf.gz") and not os.path.exists(tmp_path / "t.vcf.gz")


def test_merge_regions_zero_is_not_refused_for_want_of_a_bed_file(tmp_path):
    """The default, spelled out: the run goes on to its files as without the option (here: to the missing BAM)."""
    r = run(["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--merge-regions", "0", "--print-params", "--sequencing-platform", "1"], cwd=str(tmp_path))
    assert r.returncode == 0 and "--merge-regions" not in r.stderr, r.stderr


def test_abi():
    assert C.sizeof(_ffi.UvcScoreRange) == 16
    assert [f[0] for f in _ffi.UvcScoreRange._fields_] == ["pos_beg", "pos_end", "base_at_pos_beg", "region_beg"]
    names = [f[0] for f in _ffi.UvcScoreRequest._fields_]                   # unchanged: the oracle shares the struct
    assert names[-2:] == ["n_force_sites", "force_sites"] and C.sizeof(_ffi.UvcScoreRequest) == _ffi.UvcScoreRequest.force_sites.offset + 8 == 96
    hdr = open(os.path.join(_ffi.ROOT, "include", "uvcgpu.h")).read()
    assert "typedef struct UvcScoreRange {" in hdr
    dll = C.CDLL(_ffi.gpu_library_path())
    for name in ("uvcgpu_region_score_ranges", "uvcgpu_region_score_ranges_size", "uvcgpu_region_vcf_records_ranges"):
        assert hasattr(dll, name), name
    arr, n = region.Region.make_ranges([(5, 9), (9, 12, 1), (20, 30, 0, 20)])
    assert n == 3 and [(q.pos_beg, q.pos_end, q.base_at_pos_beg, q.region_beg) for q in arr] == [(5, 9, 0, 0), (9, 12, 1, 0), (20, 30, 0, 20)]


def test_the_oracle_binding_is_untouched():
    """The ranges entry points are bound lazily and for the HIP library alone: binding the oracle needs none of them."""
    path = __import__("oracle").library_path()
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(_ffi.ROOT, "oracle")])
    lib = _ffi.Lib(path, "uvc_oracle_")
    assert not hasattr(lib.dll, "uvc_oracle_region_score_ranges") and not hasattr(lib.dll, "uvc_oracle_score_ranges")
