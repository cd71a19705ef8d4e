"""The device read preparation on its own: uvc_prep_reads, uvc_prep_compact and the order helpers of uvc_gap.hip (uvc_sort_by_pos_cls,
uvc_launch_rank_from_sorted, uvc_launch_gather4) against tests/prep_units_restatement.py, bit for bit -- every per-read column, every
FragRec / FsRec field set_reads fills, every list, every work-list entry, every total and bound of UvcPrepOut.  The handle sizes its
buffers from those totals and picks kernel forms from those bounds, and a total that is too small is not a plane difference: the plane
comparisons with the oracle cannot see it.

The entry points are internal, so a probe program (tests/native/prep_probe_main.cpp, built by uvc_amd/csrc/Makefile against the headers
themselves) calls them with plain device buffers in a child process and exchanges raw columns through files.  A child that fails, dies
on a signal or runs out of time fails its tests and is not started again.  tests/prep_unit_cases.py has the inputs,
tests/test_prep_units_cpu.py the proof that they reach their edges (carry: the second and third round of k_tile_tops)."""
import os
import subprocess

import numpy as np
import pytest

from uvc_amd import region
import prep_unit_cases as pc
import prep_units_restatement as pr

pytestmark = pytest.mark.gpu
PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "prep_probe")
_runs = {}


def run_probe(key, mode, dirs, timeout=120):
    """One child per key; what became of it is kept, so that a second test of the same key never starts it again."""
    if key not in _runs:
        assert os.path.exists(PROBE), "%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % PROBE
        try:
            p = subprocess.run([PROBE, mode] + [str(d) for d in dirs], capture_output=True, text=True, timeout=timeout)
            _runs[key] = None if p.returncode == 0 else "prep_probe %s exited with %d:\n%s" % (mode, p.returncode, p.stderr[-2000:])
        except subprocess.TimeoutExpired:
            _runs[key] = "prep_probe %s did not finish within %d s" % (mode, timeout)
    assert _runs[key] is None, _runs[key]


def first_difference(name, got, want):
    """None, or the message that names the first differing element"""
    want = np.asarray(want)
    if len(got) != len(want):
        return "%s: %d elements on the device, %d in the restatement" % (name, len(got), len(want))
    bad = np.flatnonzero(got.astype(np.int64) != want.astype(np.int64))
    if len(bad):
        return "%s[%d]: device %d, restatement %d (%d of %d elements differ)" % (name, bad[0], got[bad[0]], want[bad[0]], len(bad), len(want))
    return None


def params_of(lib, case):
    P = region.default_params(lib, platform=case["platform"])
    for k, v in case["overrides"].items():
        setattr(P, k, v)
    return P


def check_prep(case, key, d, gpu_lib):
    pc.write_prep(d, case)
    want = pr.prep_units(case["reads"], params_of(gpu_lib, case), case["rbeg"], case["rend"], case["npos"], case["zero_qual"])
    run_probe(key, "prep", [d])
    sc = pc.read_out_scalars(d)
    for name in pr.SCALARS:
        assert sc[name] == want[name], "%s: device %d, restatement %d" % (name, sc[name], want[name])
    for name, t in pr.ARRAYS.items():
        msg = first_difference(name, pc.read_out(d, name, t), want[name])
        assert msg is None, msg
    return sc


@pytest.mark.parametrize("arm", list(pc.NESTING_ARMS))
def test_nesting(arm, gpu_lib, tmp_path):
    sc = check_prep(pc.nesting(arm), "nesting_" + arm, tmp_path, gpu_lib)
    assert sc["n_frags"] > 2048 and sc["n_fs"] > 1024 and sc["n_complex"] > 2048


def test_carry(gpu_lib, tmp_path):
    """The carry loop of k_tile_tops (its second and third round) in all eight columns of the read scan; the three-column scans and the unit
    sort at 599 479 generic units with 4 093 distinct begins (the depth arms take the three-column scan into its second round)."""
    sc = check_prep(pc.carry(), "carry", tmp_path, gpu_lib)
    assert sc["n_frags"] > pc.ROUND // 2 and sc["n_p2"] > 2 * pc.ROUND


@pytest.mark.parametrize("arm", list(pc.DEPTH_ARMS))
def test_depth(arm, gpu_lib, tmp_path):
    sc = check_prep(pc.depth(arm), "depth_" + arm, tmp_path, gpu_lib)
    assert sc["max_frag_depth"] == pc.DEPTH_ARMS[arm][2]


def test_compact(tmp_path):
    l_qseq, n_cigar = pc.carry_lengths()
    pc.write_compact(tmp_path, l_qseq, n_cigar)
    run_probe("compact", "compact", [tmp_path])
    assert pc.read_out_scalars(tmp_path)["bad"] == 0
    for name, want in pr.compact_offsets(l_qseq, n_cigar).items():
        msg = first_difference(name, pc.read_out(tmp_path, name, np.int64), want)
        assert msg is None, msg


@pytest.fixture(scope="module")
def sort_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("sort")
    dirs = {}
    for pb, cb in pc.SORT_BITS:
        for n in pc.SORT_N:
            dirs[pb, cb, n] = (str(root / ("%d_%d_%d" % (pb, cb, n))), pc.sort_case(pb, cb, n))
            pc.write_sort(*dirs[pb, cb, n])
    return dirs


@pytest.mark.parametrize("n", pc.SORT_N)
@pytest.mark.parametrize("bits", pc.SORT_BITS, ids=lambda b: "%d_%d" % b)
def test_sort(bits, n, sort_dirs):
    """Stable order by (class, offset) with exactly pos_bits + cls_bits key bits; the ranks of the first n_first ids; the gathered work list."""
    run_probe("sort", "sort", [d for d, _ in sort_dirs.values()], timeout=300)
    d, c = sort_dirs[bits[0], bits[1], n]
    perm = pr.sorted_ids(c["pos"], c["cls"], c["beg"], c["pos_bits"])
    msg = first_difference("perm", pc.read_out(d, "perm", np.uint32), perm)
    assert msg is None, msg
    for k, n_first in enumerate(c["n_first"]):
        ids, rank = pr.rank_from_sorted(perm, n_first, pc.SENTINEL)
        for name, want in (("ids_%d" % k, ids), ("rank_%d" % k, rank)):
            msg = first_difference("%s (n_first %d)" % (name, n_first), pc.read_out(d, name, np.int32), want)
            assert msg is None, msg
    for k, l in enumerate(c["lists"]):
        o, slot = pr.gather4(perm, l["a"], l["kind"], pc.SENTINEL)
        for j in range(4):
            msg = first_difference("g%d_o%d" % (k, j), pc.read_out(d, "g%d_o%d" % (k, j), np.int32), o[j])
            assert msg is None, msg
        msg = first_difference("g%d_slot (%d entries, %d alignments)" % (k, n, len(l["kind"])), pc.read_out(d, "g%d_slot" % k, np.int32), slot)
        assert msg is None, msg
