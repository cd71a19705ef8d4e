"""The mismatch queue of the accumulate (RegionDev::mis, applied by k_p2_mism) made by P1 (misq=p1, the plain P2 form) and by the base pass
(UVCGPU_MISQ=p2, and always on the generic P2 forms).  Every case runs both ways:

  items    the read-out of the two queues (uvcgpu_region_debug_mis_queue), sorted, is the same list of (rank, epos, symval); it is the list
           tests/misq_cases.py makes from the read columns; its length is the device's count, and the count set_reads sized the queue by less
           the mismatches of the InDel reads that a low quality at an InDel keeps off the work list (none in `overflow`).
  results  all 14 plane groups and the records of the default gate and of all_out are equal bit for bit between the two runs; against the
           oracle the planes are equal bit for bit, no presence violation, and the records are within the classes of
           test_gpu_parity.compare_records (the oracle's floating-point fields are not the device's bit for bit on the parent either).

tests/test_misq_cpu.py shows that each input reaches the edge it is named after.  The line `[uvcgpu accumulate] misq=p1|p2` (UVCGPU_TIMING) says
who made the queue; it stands behind the forms line, whose keys are a closed set to tests/kernel_forms.py."""
import numpy as np
import pytest

import misq_cases as mc
from kernel_forms import IONTORRENT
from test_gpu_parity import compare_records
from test_gpu_worklist import check, oracle_run
from uvc_amd import region, synth
from util import amplicon_stack, diff_groups, presence_violations

pytestmark = pytest.mark.gpu

CASES = dict([("npos_%d" % n, (lambda n=n: mc.boundary(n)["reads"])) for n in mc.REGION_LENGTHS],
             overflow=mc.overflow, empty=mc.empty, with_n=lambda: mc.with_n()["reads"], quality_bytes=lambda: mc.quality_bytes()["reads"])
# how P1 runs: (environment, the P1 kernel the accumulate names); UVCGPU_ONE_STREAM is read when the handle is made
P1_FORMS = {"scan": ({}, "k_prep_scan"), "window": ({"UVCGPU_PREP": "window"}, "k_prep_fast<false>"), "split": ({"UVCGPU_SPLIT": "1"}, "k_prep_fast<true>"),
            "one_stream": ({"UVCGPU_ONE_STREAM": "1"}, "k_prep_scan")}
SWITCHES = ("UVCGPU_MISQ", "UVCGPU_PREP", "UVCGPU_SPLIT", "UVCGPU_ONE_STREAM", "UVCGPU_LINK", "UVCGPU_LINK_FORM")


def lines(err, key):
    return [l.split(key)[1] for l in err.splitlines() if l.startswith("[uvcgpu accumulate] " + key)]


def handle(gpu_lib, reads, monkeypatch, misq, env=None, platform=1):
    """A handle under the switches (misq: None or "p2"); the environment stays as set, for the accumulates that follow."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if misq:
        monkeypatch.setenv("UVCGPU_MISQ", misq)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    return region.Region(gpu_lib, region.default_params(gpu_lib, platform=platform), reads["tid"], reads["beg"], reads["end"], reads["refseq"])


def sorted_rows(rows):
    return sorted(map(tuple, rows.tolist()))


def same(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])] + [k for k in b if k not in a]


def two_runs(gpu_lib, reads, monkeypatch, capfd, env=None, platform=1):
    """-> {misq: (handle, queue rows sorted, n, total, the misq line, the P1 kernel line)} for misq unset and p2."""
    out = {}
    for misq in (None, "p2"):
        R = handle(gpu_lib, reads, monkeypatch, misq, env, platform)
        R.set_reads(reads)
        capfd.readouterr()
        R.accumulate()
        err = capfd.readouterr().err
        rows, n, total = R.debug_mis_queue()
        out[misq] = (R, sorted_rows(rows), n, total, lines(err, "misq="), lines(err, "prep kernel "))
    return out


@pytest.mark.parametrize("form", list(P1_FORMS))
@pytest.mark.parametrize("case", list(CASES))
def test_items_and_results(case, form, oracle_lib, gpu_lib, monkeypatch, capfd):
    reads, Ro, ro = oracle_run(oracle_lib, "misq_" + case, CASES[case])
    env, kernel = P1_FORMS[form]
    runs = two_runs(gpu_lib, reads, monkeypatch, capfd, env)
    (R1, rows1, n1, total1, who1, k1), (R2, rows2, n2, total2, who2, k2) = runs[None], runs["p2"]
    try:
        assert who1 == ["p1"] and who2 == ["p2"] and k1 == [kernel] and k2 == [kernel], (who1, who2, k1, k2)
        # items
        want, _ = mc.items(reads, added_misma=region.default_params(gpu_lib).bq_phred_added_misma)
        print("%s / %s: %d items by P1, %d by the base pass, %d restated, mis_total %d" % (case, form, n1, n2, len(want), total1))
        # (the count set_reads made also holds the InDel reads a low quality keeps off the list: misq_cases.demoted_mismatches)
        assert n1 == len(rows1) == n2 == len(rows2) == total1 - mc.demoted_mismatches(reads) and total2 == total1
        assert rows1 == rows2, [r for r in rows1 if r not in set(rows2)][:5] + [r for r in rows2 if r not in set(rows1)][:5]
        assert rows1 == want
        if case == "empty":
            assert n1 == 0
        # results: one run against the other, then against the oracle
        bad = diff_groups(R1, R2)
        assert not bad, "\n".join("%s: %d cells differ, first (index, p1, p2) %s" % (g, v[0], v[1]) for g, v in bad.items())
        assert presence_violations(R1) == 0 and presence_violations(R2) == 0
        for all_out in (False, True):
            a, b = R1.score(all_out=all_out), R2.score(all_out=all_out)
            assert not same(a, b), (all_out, same(a, b))
            if all_out:
                compare_records(Ro.score(all_out=True), a)
        check(Ro, ro, R1, "%s / %s / p1: " % (case, form))
        check(Ro, ro, R2, "%s / %s / p2: " % (case, form))
    finally:
        R1.close(); R2.close()


def generic_inputs(which):
    if which == "amplicon_stack":
        return amplicon_stack(), 1
    return synth.generate_region(region_len=2000, depth=100, seed=32, indel_every=300, clip_frac=0.05, variant_inset=200), IONTORRENT


@pytest.mark.parametrize("which", ["amplicon_stack", "iontorrent"])
def test_generic_forms_keep_the_queue_of_the_base_pass(which, oracle_lib, gpu_lib, monkeypatch, capfd):
    """An amplicon tile (util.amplicon_stack with the amplicon flag on every family: the amplicon arm of P2) and an IonTorrent run: misq=p2
    whatever UVCGPU_MISQ says, the same queue both times, results equal to the oracle's."""
    reads, platform = generic_inputs(which)
    if which == "amplicon_stack":
        reads = dict(reads, fam_dflag=np.full(reads["n_fams"], 4, np.uint8))   # every family carries the amplicon flag: RegionDev::any_amplicon
    Ro = region.Region(oracle_lib, region.default_params(oracle_lib, platform=platform), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Ro.set_reads(reads); Ro.accumulate()
    ro = Ro.score()
    runs = two_runs(gpu_lib, reads, monkeypatch, capfd, platform=platform)
    try:
        for misq, (R, rows, n, total, who, _) in runs.items():
            assert who == ["p2"], (misq, who)
            check(Ro, ro, R, "%s / %s: " % (which, misq))
        assert runs[None][1] == runs["p2"][1] and runs[None][2] == runs["p2"][2]
    finally:
        for R in (Ro, runs[None][0], runs["p2"][0]):
            R.close()


@pytest.mark.parametrize("misq", [None, "p2"])
def test_one_handle_used_again(misq, oracle_lib, gpu_lib, monkeypatch):
    """Accumulate twice on the same reads, then score; six rounds with the planes handed back every other one; a region of another length and
    back.  The records and the queue's count are the same every time: a count that was not zeroed would double."""
    big, Ro, ro = oracle_run(oracle_lib, "misq_npos_2049", CASES["npos_2049"])
    small = CASES["npos_1023"]()
    R = handle(gpu_lib, big, monkeypatch, misq)
    monkeypatch.delenv("UVCGPU_TIMING")
    try:
        R.set_reads(big)
        R.accumulate()
        rows0, n0, total0 = R.debug_mis_queue()
        first = R.score()
        compare_records(ro, first)
        assert n0 == total0 - mc.demoted_mismatches(big) > 0
        R.accumulate(); R.accumulate()
        rows, n, _ = R.debug_mis_queue()
        assert n == n0 and sorted_rows(rows) == sorted_rows(rows0)
        assert not same(first, R.score())
        for k in range(6):
            R.accumulate()
            assert R.debug_mis_queue()[1] == n0, k
            assert not same(first, R.score(release_state=(k % 2 == 1))), k
        R.reset(small["tid"], small["beg"], small["end"], small["refseq"])
        R.set_reads(small)
        R.accumulate()
        n_small, total_small = R.debug_mis_queue()[1:]
        assert n_small == total_small - mc.demoted_mismatches(small) == len(mc.items(small)[0]) != n0
        R.reset(big["tid"], big["beg"], big["end"], big["refseq"])
        R.set_reads(big)
        R.accumulate()
        rows, n, total = R.debug_mis_queue()
        assert n == n0 and total == total0 and sorted_rows(rows) == sorted_rows(rows0)
        assert not same(first, R.score())
        assert not diff_groups(Ro, R)
    finally:
        R.close()
