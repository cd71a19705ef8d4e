"""One handle carried through three regions -- 500 bp, 4 300 bp, 500 bp of reads at some 30x (700 and 4 500 positions with the halo of
uvc_amd/synth.py; 500 bp is the shortest region whose reads the generator keeps inside it, 300 bp gives reads in front of the region, which
set_reads refuses) -- against a fresh handle on the same input at every stop.  The long region crosses one dirty block of 4 096 positions and
four scan tiles: the smallest lengths at which every buffer of the handle grows (second stop), stays when the region shrinks (third stop),
and the full fill of the slab (the first accumulate of a stop: unknown layout, another length) and the selective fill (the accumulate of the
same length that every stop ends with) both run.  Everything a handle
answers from its own buffers is compared byte for byte: the 14 plane groups, columns of chosen positions, both block-statistics calls,
the one-call score plain and kept_only, a streamed score of three or more chunks, the coverage report, the InDel allele tables and the
haplotype links; uvcgpu_region_check_presence (whose second half walks the plane groups of each dirty family) reports no violation."""
import ctypes as C

import numpy as np
import pytest

from uvc_amd import region, synth
from util import INT_GROUPS, presence_violations

pytestmark = pytest.mark.gpu

VARIANTS = dict(depth=30, snv_every=40, somatic_every=130, indel_every=90, variant_inset=100)
STOPS = [dict(region_len=500, seed=71, beg=2_000_000), dict(region_len=4300, seed=72, beg=3_000_000), dict(region_len=500, seed=73, beg=2_500_000)]


def block_stats(R):
    lib, beg, end = R.lib, R.beg, R.beg + R.npos
    one = lib.dll.uvcgpu_region_block_stats_
    one.restype, one.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    whole = np.zeros((R.npos, 10), np.int32)
    assert one(R.h, beg, end, whole.ctypes.data) == 0, lib.last_error()
    many = lib.dll.uvcgpu_region_block_stats_windows_
    many.restype, many.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    win = np.array([beg, beg + 7, beg + 100, beg + 164, end - 65, end], np.int32)
    rows = np.zeros((7 + 64 + 65, 10), np.int32)
    assert many(R.h, win.ctypes.data, 3, rows.ctypes.data) == 0, lib.last_error()
    assert np.array_equal(rows, np.concatenate([whole[0:7], whole[100:164], whole[R.npos - 65:]]))
    assert whole[:, 8].sum() > 0
    return whole, rows


def answers(R):
    """everything the handle answers after an accumulate, in a fixed order; ends with an accumulate of the same length (the selective fill)"""
    beg, end = R.beg, R.beg + R.npos
    out = {"fetch " + g: R.fetch(g) for g in INT_GROUPS}
    assert len(out) == 14
    out["columns"] = R.fetch_columns([beg - 5, beg, beg + 1, beg + R.npos // 2, end - 1, end + 3])   # the first and the last lie outside: rows of zeros
    assert not out["columns"][0].any() and not out["columns"][-1].any() and out["columns"][1:-1].any()
    out["block statistics"], out["block statistics of windows"] = block_stats(R)
    out["score"] = R.score()
    out["score kept_only"] = R.score(kept_only=True)
    out["score all_out"] = R.score(all_out=True)
    n = len(out["score all_out"]["refpos"])
    chunks = list(R.score_stream(max(n // 4, 64), all_out=True))
    assert len(chunks) >= 3 and sum(len(rec["refpos"]) for rec, _ in chunks) == n, (len(chunks), n)
    for k, (rec, covered) in enumerate(chunks):
        out["stream chunk %d" % k] = rec
        out["stream chunk %d covers" % k] = np.array(covered)
    out["coverage"] = R.coverage([(beg, beg + 10), (beg + 10, beg + 20), (beg + 64, end - 30), (end - 30, end)], [1, 20])   # (sorted and disjoint)
    out["indel_alleles"] = R.indel_alleles()
    out["hap_links"] = R.hap_links()
    assert len(out["indel_alleles"]) > 0 or R.npos < 4096   # (synth plants InDels in the long region only)
    out["violations"] = presence_violations(R)
    R.accumulate()   # the same length again: the selective fill, from the marks of the accumulate above
    out.update({"second fetch " + g: R.fetch(g) for g in INT_GROUPS})
    out["second score"] = R.score()
    out["second violations"] = presence_violations(R)
    return out


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def test_one_handle_through_three_regions_equals_fresh_handles(gpu_lib):
    R = None
    for i, stop in enumerate(STOPS):
        t = synth.generate_region(**stop, **VARIANTS)
        got = {}
        for name in ("carried", "fresh"):
            if name == "fresh" or R is None:
                H = region.Region(gpu_lib, region.default_params(gpu_lib), t["tid"], t["beg"], t["end"], t["refseq"])
            else:
                H = R
                H.reset(t["tid"], t["beg"], t["end"], t["refseq"])
            H.set_reads(t)
            H.accumulate()
            got[name] = answers(H)
            if name == "fresh":
                H.close()
            else:
                R = H
        label = "stop %d (%d bp)" % (i, stop["region_len"])
        assert got["carried"].keys() == got["fresh"].keys(), label
        for k in got["fresh"]:
            assert same(got["carried"][k], got["fresh"][k]), "%s: %s of the carried handle differs from a fresh handle's" % (label, k)
        assert got["carried"]["violations"] == 0 and got["carried"]["second violations"] == 0, label
        assert all(same(got["carried"]["fetch " + g], got["carried"]["second fetch " + g]) for g in INT_GROUPS), label
    R.close()
