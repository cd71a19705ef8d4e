"""The six report calls (uvcgpu_region_coverage, _error_profile, _family_stats, _callable, _read_profile, _msi) share the rules of a range
list and, the plane readers, the lookup of a lane's range on the device.
  * The same bad lists handed to all six raw entry points give the same return code and, behind the call's name, the same message; the
    handle answers as before afterwards.
  * Range borders inside a wave, on wave borders, on the 256-position step and on the 1 024-position block of the callable kernels, with a
    total that is no multiple of 64: coverage, error profile and callable runs equal the restatements over the oracle's planes, value by value.
  * The command line with all six reports in one run writes, report by report, the bytes of six runs with one report each.
Every number is an integer and is compared for equality."""
import ctypes as C
import gzip
import os
import subprocess
import time

import numpy as np
import pytest

import callable_restatement as cr
import errprofile_restatement as er
import famstats_restatement as fr
from test_gpu_coverage import EXE, measures_of, panel, rows_of
from test_gpu_parity import CASES
from util import run_region
from uvc_amd import _ffi, region, synth

pytestmark = pytest.mark.gpu

E = _ffi.ENUMS
EINVAL = E["UVCGPU_EINVAL"]
THR = [1, 3, 5]
SENTINEL = -123456789
RP_GATE = (0, 2, 500)   # read_profile: min_mapq, min_depth, max_alt_permille
MSI_REQ = (4, 2, 6)     # msi: min_tracklen, min_units, max_unitlen (short tracts: 600 random bases have some)


def raw_calls(lib, R):
    """name -> call(ranges, n) -> (rc, message, the output buffers untouched) of the six entry points as the ABI has them"""
    def bind(name, argtypes):
        fn = getattr(lib.dll, "uvcgpu_region_" + name)
        fn.restype, fn.argtypes = C.c_int, argtypes
        return fn
    cov = bind("coverage", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p])
    err = bind("error_profile", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
    fam = bind("family_stats", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    cal = bind("callable", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    rpf = bind("read_profile", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
    msi = bind("msi", [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
    thr = np.array(THR, np.int32)

    def pairs(ranges):
        return (_ffi.UvcCoverageRange * max(len(ranges), 1))(*[_ffi.UvcCoverageRange(a, b) for a, b in ranges])

    def done(rc, *outs):
        return rc, lib.last_error(), all((o == SENTINEL).all() for o in outs)

    def coverage(ranges, n):
        out = np.full((max(len(ranges), 1), E["UVC_NCOV"], E["UVC_COV_ROW"]), SENTINEL, np.int64)
        return done(cov(R.h, pairs(ranges), n, thr.ctypes.data, len(thr), out.ctypes.data), out)

    def error_profile(ranges, n):
        out = np.full((E["UVC_NERRLEVEL"], E["UVC_ERR_ROW"]), SENTINEL, np.int64)
        req = _ffi.UvcErrorProfileRequest(2, 500)
        return done(err(R.h, pairs(ranges), n, C.byref(req), out.ctypes.data), out)

    def family_stats(ranges, n):   # prev_end = the begin of the region: below every begin and every end of these lists, never decreasing
        arr = (_ffi.UvcFamilyRange * max(len(ranges), 1))(*[_ffi.UvcFamilyRange(a, b, min(R.beg, a), 0) for a, b in ranges])
        out = np.full((max(len(ranges), 1), E["UVC_FAMSTAT_ROW"]), SENTINEL, np.int64)
        return done(fam(R.h, arr, n, out.ctypes.data), out)

    def callable_(ranges, n):
        out, n_runs = np.full((R.npos, 4), SENTINEL, np.int32), np.full(1, SENTINEL, np.int64)
        req = _ffi.UvcCallableRequest((C.c_int32 * E["UVC_NCOV"])(0, 0, 0, 3, 0, 0), 0)
        return done(cal(R.h, pairs(ranges), n, C.byref(req), out.ctypes.data, R.npos, n_runs.ctypes.data), out, n_runs)

    def read_profile(ranges, n):
        out = np.full(E["UVC_READPROF_ROW"], SENTINEL, np.int64)
        req = _ffi.UvcReadProfileRequest(*RP_GATE)
        return done(rpf(R.h, pairs(ranges), n, C.byref(req), out.ctypes.data), out)

    def msi_(ranges, n):
        out, n_loci = np.full((R.npos, E["UVC_MSI_ROW"]), SENTINEL, np.int32), np.full(1, SENTINEL, np.int64)
        req = _ffi.UvcMsiRequest(*MSI_REQ)
        return done(msi(R.h, pairs(ranges), n, C.byref(req), out.ctypes.data, R.npos, n_loci.ctypes.data), out, n_loci)

    return {"coverage": coverage, "error_profile": error_profile, "family_stats": family_stats, "callable": callable_, "read_profile": read_profile, "msi": msi_}


def test_the_four_calls_refuse_the_same_lists_in_the_same_words(oracle_lib, gpu_lib):
    reads = synth.generate_region(**CASES["tiny_600bp_5x"])
    Ro = run_region(oracle_lib, reads)
    m, cells = measures_of(Ro.fetch), er.level_cells(Ro.fetch)
    Ro.close()
    R = run_region(gpu_lib, reads)   # one accumulate
    beg, end = R.beg, R.beg + R.npos
    ok = [(beg + 5, beg + 100), (beg + 100, beg + 101), (beg + 300, end)]
    fam_ok = [(beg + 5, beg + 100, beg, 0), (beg + 100, beg + 101, beg + 100, 0), (beg + 300, end, beg + 101, 0)]   # prev_end: the end of the range before
    want = dict(coverage=rows_of(m, beg, ok, THR), error_profile=er.Restatement(cells, reads["refseq"], beg, 2, 500).profile(ok),
                family_stats=fr.rows(fr.families(reads), fam_ok), callable=cr.runs_of(m, beg, ok, [0, 0, 0, 3, 0, 0], 0))
    assert want["coverage"].any() and want["error_profile"].any() and want["family_stats"].any() and len(want["callable"]) > 3

    def answers():
        return dict(coverage=R.coverage(ok, THR), error_profile=R.error_profile(ok, 2, 500), family_stats=R.family_stats(fam_ok),
                    callable=R.callable(ok, {"cDP12": 3}), read_profile=R.read_profile(ok, *RP_GATE), msi=R.msi(ok, *MSI_REQ))

    # the two newer calls have their restatements in their own tests: here their answers before any refusal are what they answer after one
    want.update((name, answers()[name]) for name in ("read_profile", "msi"))
    assert want["read_profile"].any() and len(want["msi"]) > 0 and (want["msi"][:, E["UVC_MSI_range"]] < len(ok)).all()

    def assert_right(what):
        got = answers()
        for name in want:
            assert np.array_equal(got[name], want[name]), (name, what)

    assert_right("before any refusal")
    calls = raw_calls(gpu_lib, R)
    bad_lists = [
        ("unsorted", [(beg + 200, beg + 250), (beg + 10, beg + 50)], None, "range 1 [%d, %d) begins in front of the end %d of range 0 (ranges must be sorted and disjoint)" % (beg + 10, beg + 50, beg + 250)),
        ("overlapping", [(beg + 10, beg + 50), (beg + 49, beg + 60)], None, "range 1 [%d, %d) begins in front of the end %d of range 0 (ranges must be sorted and disjoint)" % (beg + 49, beg + 60, beg + 50)),
        ("empty", [(beg + 10, beg + 50), (beg + 60, beg + 60)], None, "range 1 [%d, %d) is empty" % (beg + 60, beg + 60)),
        ("reversed", [(beg + 50, beg + 10)], None, "range 0 [%d, %d) is empty" % (beg + 50, beg + 10)),
        ("in front of the region", [(beg - 1, beg + 10)], None, "range 0 [%d, %d) is outside the region [%d, %d)" % (beg - 1, beg + 10, beg, end)),
        ("behind the region", [(beg + 10, beg + 20), (end - 3, end + 1)], None, "range 1 [%d, %d) is outside the region [%d, %d)" % (end - 3, end + 1, beg, end)),
        ("n_ranges = 0", ok, 0, "n_ranges 0 must be at least 1"),
    ]
    for what, ranges, n, text in bad_lists:
        got = {name: call(ranges, len(ranges) if n is None else n) for name, call in calls.items()}
        print(what, {name: g[:2] for name, g in got.items()})
        for name, (rc, msg, untouched) in got.items():
            assert rc == EINVAL and untouched, (what, name, rc, msg)
            assert msg.startswith(name + ": "), (what, name, msg)
        tails = {msg[len(name) + 2:] for name, (rc, msg, untouched) in got.items()}
        assert tails == {text}, (what, tails)
        assert_right("after: " + what)
    R.close()


# Lengths of adjacent ranges, the rest of the region behind them.  Their first compact positions: 0, 1, 2 (borders inside a wave), 64, 128 (on
# wave borders), 193, 194 (inside the next wave), 385 (inside the second 256-position step), 1 024 (the block border of the callable kernels,
# also a step and a wave border), 1 025.
LENGTHS = [1, 1, 62, 64, 65, 1, 191, 639, 1]


def cursor_ranges(beg, npos):
    ranges, at = [], beg + 7
    for n in LENGTHS:
        ranges.append((at, at + n))
        at += n
    ranges.append((at, beg + npos))
    return ranges


def test_range_borders_on_wave_step_and_block_borders(oracle_lib, gpu_lib):
    reads = synth.generate_region(**CASES["umi_duplex_2kb_400x"])
    Ro = run_region(oracle_lib, reads)
    m, cells = measures_of(Ro.fetch), er.level_cells(Ro.fetch)
    Ro.close()
    Rg = run_region(gpu_lib, reads)
    beg, npos = Rg.beg, Rg.npos
    ranges = cursor_ranges(beg, npos)
    firsts = np.cumsum([0] + [b - a for a, b in ranges])   # the compact position each range begins at, and the total
    print("npos", npos, "compact firsts", firsts.tolist())
    assert firsts[:10].tolist() == [0, 1, 2, 64, 128, 193, 194, 385, 1024, 1025] and firsts[-1] > 1025 + 256 and firsts[-1] % 64 != 0
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and ranges[0][0] == beg + 7 and ranges[9][1] == beg + npos
    med = {region.COVERAGE_MEASURES[k]: int(np.median(m[k])) for k in range(E["UVC_NCOV"])}
    assert all(v > 0 for v in med.values()), med
    for lst, what in ((ranges, "the list"), (ranges[:9], "without the rest: 1 025 positions"), (ranges[2:], "from the third range on")):
        for thr in ([1, 20, 100, 500], []):
            got, want = Rg.coverage(lst, thr), rows_of(m, beg, lst, thr)
            bad = np.argwhere(got != want)
            assert got.shape == want.shape and len(bad) == 0, ("coverage", what, thr, [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])
        for gate in ((20, 50), (1, 1000)):
            got, want = Rg.error_profile(lst, *gate), er.Restatement(cells, reads["refseq"], beg, *gate).profile(lst)
            bad = np.argwhere(got != want)
            assert got.shape == want.shape and len(bad) == 0, ("error_profile", what, gate, [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])
        for min_depth, max_aDP in ((med, 0), ({}, 0), ({"cDP12": med["cDP12"]}, med["aDP"])):
            got, want = Rg.callable(lst, min_depth, max_aDP), cr.runs_of(m, beg, lst, *cr.request(min_depth, max_aDP))
            assert got.shape == want.shape and np.array_equal(got, want), ("callable", what, min_depth, max_aDP, np.flatnonzero(got != want)[:6] if got.shape == want.shape else (got.shape, want.shape))
            assert sorted(set(got["range"].tolist())) == list(range(len(lst)))   # every range has its runs, under its own index
    Rg.close()


# ------------------------------------------------------------------------------------------------ command line: all six reports in one run
REPORT_OPTS = {"--coverage-out": "--coverage-window", "--error-profile-out": None, "--family-stats-out": "--family-stats-window", "--callable-out": None,
               "--msi-out": None, "--read-profile-out": None}


@pytest.mark.parametrize("case", ["bed_tile_1000", "windows_tile_1700"])
def test_all_six_reports_in_one_run_equal_six_runs_with_one_each(tmp_path, case):
    """One worker's range and target lists serve every report of a tile in turn, and --callable-out and --msi-out share their targets: the
    reports of a run that writes all six are, file by file, the bytes of six runs that write one each, and the seven VCFs are equal.  The
    panel of test_gpu_coverage: several tiles per target, a target without reads, a target over a contig's end; two workers."""
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    d = str(tmp_path)
    bam, fa, bed, _, _ = panel(d)
    shared = ["-R", bed, "--tile", "1000", "-t", "2"] if case == "bed_tile_1000" else ["--tile", "1700", "-t", "2"]
    windows = {opt: ([w, "1000"] if w and case == "windows_tile_1700" else []) for opt, w in REPORT_OPTS.items()}

    def run(tag, opts):   # its own child process and time limit; the case ends at the first run that does not exit 0
        args = [a for opt in opts for a in [opt, os.path.join(d, tag + opt)] + windows[opt]]
        r = subprocess.run([EXE, bam, "-f", fa, "-o", os.path.join(d, tag + ".vcf.gz"), "-s", "S"] + shared + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (tag, r.returncode, r.stderr[-2000:])
        vcf = [l for l in gzip.open(os.path.join(d, tag + ".vcf.gz"), "rt").read().splitlines() if not l.startswith(("##fileDate=", "##variantCallerCommand="))]
        return vcf, {opt: open(os.path.join(d, tag + opt), "rb").read() for opt in opts}

    t0 = time.time()
    vcf_all, all_six = run("all", list(REPORT_OPTS))
    assert len(vcf_all) > 100 and all(len(text) > 0 for text in all_six.values())
    for k, opt in enumerate(REPORT_OPTS):
        vcf_one, one = run("one%d" % k, [opt])
        assert one[opt] == all_six[opt], (case, opt)
        assert vcf_one == vcf_all, (case, opt)
    print("%s: seven runs in %.1f s" % (case, time.time() - t0))
