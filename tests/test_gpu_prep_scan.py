"""P1 of the simple alignments in its two forms: k_prep_fast<false> (UVCGPU_PREP=window: every 64-position window walks the reads that
reach it) and k_prep_scan (UVCGPU_PREP=scan, the default: every read is scanned once, eight bases per lane, and the counters behind the
base quality are interval sums minus a correction per low-quality base).  Every case runs in both forms; both must equal the oracle bit
for bit in all 14 plane groups, with no presence violation and the records within the classes of test_gpu_parity.compare_records.  The
UVCGPU_TIMING line `[uvcgpu accumulate] prep kernel ...` says which kernel ran.

Case 1 has bases of quality 0.  Their value is 0 (bq_phred_added_misma = 0), and the reference skips a (fragment, position) whose
consensus counts add up to 0; set_reads sends a fragment with such a base to the per-position P3 kernels (FragRec::stat_kind 2,
k_build_frags), which skip it the same way.  `paired_from_1` is the same case with qualities 1..19: no fragment takes that route."""
import numpy as np
import pytest

from uvc_amd import region, synth
from test_gpu_worklist import CASE5, M, S, check, indel_only, oracle_run, unpaired
from util import diff_groups, run_region

pytestmark = pytest.mark.gpu

FORMS = {"window": "k_prep_fast<false>", "scan": "k_prep_scan"}
TILES = (256, 512, 1024)   # the tile sizes k_prep_scan was tried with: every case has reads on these boundaries
EINVAL = -2   # UVCGPU_EINVAL


def ran(err):
    """The P1 kernels the accumulates named on stderr."""
    return [l.split("prep kernel ")[1] for l in err.splitlines() if l.startswith("[uvcgpu accumulate] prep kernel ")]


@pytest.fixture(params=list(FORMS))
def form(request, monkeypatch):
    monkeypatch.setenv("UVCGPU_PREP", request.param)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    monkeypatch.delenv("UVCGPU_SPLIT", raising=False)
    return request.param


def lower_qualities(reads, seed, lowest=0):
    """About a quarter of the qualities become lowest..19 (below bias_thres_highBQ) in runs of 1..12 bases, which cross the 8-byte words of
    the scan; every 9th read is low at its first and last aligned base, every 23rd throughout."""
    rng = np.random.default_rng(seed)
    reads = dict(reads)
    q = reads["quals"].copy()
    for k in range(reads["n_reads"]):
        off, l = int(reads["seq_off"][k]), int(reads["l_qseq"][k])
        i = 0
        while i < l:
            if rng.random() < 0.05:
                n = int(rng.integers(1, 13))
                q[off + i:off + min(i + n, l)] = rng.integers(lowest, 20, min(i + n, l) - i)
                i += n
            else:
                i += 1
        cg = reads["cigars"][int(reads["cigar_off"][k]):int(reads["cigar_off"][k]) + int(reads["n_cigar"][k])]
        lead = int(cg[0] >> 4) if (cg[0] & 0xF) == S else 0
        trail = int(cg[-1] >> 4) if (len(cg) > 1 and (cg[-1] & 0xF) == S) else 0
        if k % 9 == 0 and lead + trail < l:
            q[off + lead] = lowest
            q[off + l - 1 - trail] = 19
        if k % 23 == 0:
            q[off:off + l] = rng.integers(lowest, 20, l)
    reads["quals"] = q
    return reads


def case1(lowest=0):
    """Paired reads over 2600 positions (no multiple of 64 or of a tile size; boundaries of all three tile sizes inside), 3 % errors (SNV /
    DNV runs, some across a boundary), 30 % clipped reads, InDel reads in between."""
    reads = lower_qualities(synth.generate_region(seed=41, region_len=2600, depth=40, err_rate=0.03, clip_frac=0.3, indel_every=500), seed=42, lowest=lowest)
    assert 0.2 < (reads["quals"] < 20).mean() < 0.4 and reads["quals"].min() == lowest
    return reads


def case1_from_1():
    """Case 1 with low qualities 1..19: no base of quality 0 (see the module's docstring)."""
    return case1(lowest=1)


def edges():
    """Unpaired reads of every length mod 8 and shorter than a word, clipped on either or both sides, on the region's first position and up to
    its last read position, and for every tile size one read that ends on the tile boundary, one that begins on it and one across it."""
    n_ref = 1100
    specs = []

    def add(start, m, lclip=0, rclip=0):
        cg = ([(S, lclip)] if lclip else []) + [(M, m)] + ([(S, rclip)] if rclip else [])
        specs.append((start, 0, cg))

    lengths = list(range(1, 18)) + [63, 64, 65]
    for k, m in enumerate(lengths):
        add(0, m, lclip=(k % 3 == 1) * 4, rclip=(k % 3 == 2) * 7)              # begin on the region's first position
        add(30 + 11 * k, m, lclip=(k % 2) * 3, rclip=(k % 4 >= 2) * 5)
        add(n_ref - m, m, lclip=(k % 3 == 0) * 6, rclip=(k % 3 == 1) * 2)      # end on the last position a read may cover
    for t in TILES:
        for m in (5, 8, 13, 64, 70):
            add(t - m, m, rclip=3)           # ends exactly at the boundary
            add(t, m, lclip=2)               # begins on it
            add(t - m // 2 - 1, m, lclip=1, rclip=1)   # straddles it
    specs.sort(key=lambda sp: sp[0])
    specs = [(st, 16 * (k % 2), cg) for k, (st, _, cg) in enumerate(specs)]
    reads = unpaired(specs, n_ref=n_ref, seed=43)
    # a read may not cover the region's last position (both libraries refuse it): one more reference base behind the reads
    reads["end"] += 1
    reads["refseq"] += "A"
    reads["fam_dflag"] = (np.arange(reads["n_reads"]) % 2 * 4).astype(np.uint8)   # every other family is an amplicon family: both arms of clip_event
    return reads


def sparse_head():
    """Reads in the first 200 of 1500 positions only: the later tiles are empty."""
    rng = np.random.default_rng(44)
    starts = np.sort(rng.integers(0, 140, 60))
    return unpaired([(int(s), 16 * (k % 2), [(M, 60)]) for k, s in enumerate(starts)], n_ref=1500, seed=45)


CASES = {"paired": case1, "paired_from_1": case1_from_1, "edges": edges, "indel_only": indel_only, "sparse_head": sparse_head}


@pytest.mark.parametrize("case", list(CASES))
def test_both_forms_match_the_oracle(case, form, oracle_lib, gpu_lib, capfd):
    reads, Ro, ro = oracle_run(oracle_lib, "prep_scan_" + case, CASES[case])
    if case == "indel_only":
        assert (reads["n_cigar"] > 1).all()
    capfd.readouterr()
    Rg = run_region(gpu_lib, reads)
    assert ran(capfd.readouterr().err) == [FORMS[form]]
    check(Ro, ro, Rg, "%s / %s: " % (case, form))
    if case != "indel_only":
        assert Rg.fetch("PREP32").any()
    Rg.close()


def test_the_two_forms_leave_the_same_planes(oracle_lib, gpu_lib, monkeypatch):
    """Case 1 (qualities from 0 on) by k_prep_fast<false> and by k_prep_scan: all 14 plane groups and the records, one against the other."""
    reads = case1()
    out = {}
    for f in FORMS:
        monkeypatch.setenv("UVCGPU_PREP", f)
        out[f] = run_region(gpu_lib, reads)
    bad = diff_groups(out["window"], out["scan"])
    assert not bad, "\n".join("%s: %d cells differ, e.g. %s" % (g, v[0], v[1]) for g, v in bad.items())
    rw, rs = out["window"].score(), out["scan"].score()
    assert all(np.array_equal(rw[k], rs[k]) for k in rw)
    assert out["scan"].fetch("PREP64").any()
    for R in out.values():
        R.close()


def test_reads_outside_the_region_are_refused(oracle_lib, gpu_lib):
    """A read that begins before the region or ends behind it never reaches the accumulate (the scan relies on it: every byte it compares has
    a reference position inside the region)."""
    reads = edges()
    for cut in (dict(beg=reads["beg"] + 1, refseq=reads["refseq"][1:]), dict(end=reads["end"] - 2, refseq=reads["refseq"][:-2])):
        narrow = dict(reads, **cut)
        for lib in (oracle_lib, gpu_lib):
            R = region.Region(lib, region.default_params(lib), narrow["tid"], narrow["beg"], narrow["end"], narrow["refseq"])
            with pytest.raises(region.UvcError) as e:
                R.set_reads(narrow)
            assert e.value.code == EINVAL, e.value
            R.close()


@pytest.mark.parametrize("case", ["paired", "paired_from_1"])
def test_one_handle_used_again(case, form, oracle_lib, gpu_lib, capfd):
    """Case 1, a shorter region, case 1 again on one handle, and two accumulates on the same reads: LDS or plane state that stayed behind
    would show."""
    one = oracle_run(oracle_lib, "prep_scan_" + case, CASES[case])
    short = oracle_run(oracle_lib, "case5", lambda: synth.generate_region(**CASE5))
    assert short[0]["end"] - short[0]["beg"] < one[0]["end"] - one[0]["beg"]   # region_len=1000
    R = None
    for k, (reads, Ro, ro) in enumerate((one, short, one)):
        if R is None:
            R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        else:
            R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        R.set_reads(reads)
        capfd.readouterr()
        R.accumulate()
        check(Ro, ro, R, "use %d / %s: " % (k, form))
    R.accumulate()
    assert ran(capfd.readouterr().err)[-1] == FORMS[form]
    assert not diff_groups(one[1], R), "second accumulate on the same reads"
    R.close()


def test_large_baq_increments_keep_the_window_form(form, oracle_lib, gpu_lib, capfd):
    """indel_nonSTR_phred_per_base in the millions: the BAQ prefix sums grow by 3 100 000 per position (their low words wrap inside the
    region), two of them a read and a tile (of any of the sizes above) apart can differ by 2^30 and more, and the 32-bit split of k_prep_scan is no longer provably exact
    (prep_scan_exact): k_prep_fast<false> runs whatever UVCGPU_PREP says.  (Three reads deep: the sums of such BAQ differences stay below
    2^31 per position.)"""
    reads = lower_qualities(unpaired([(40 * k, 16 * (k % 2), [(M, 100)]) for k in range(35)], n_ref=1500, seed=46), seed=47, lowest=1)
    params = {}
    for lib in (oracle_lib, gpu_lib):
        params[lib] = region.default_params(lib)
        params[lib].indel_nonSTR_phred_per_base = 3_100_000
    Ro = run_region(oracle_lib, reads, params=params[oracle_lib])
    baq = Ro.fetch("BAQ")[0]
    assert np.abs(np.diff(baq)).max() * (100 + min(TILES)) >= 1 << 30 and baq.max() >= 1 << 31
    capfd.readouterr()
    Rg = run_region(gpu_lib, reads, params=params[gpu_lib])
    assert ran(capfd.readouterr().err) == ["k_prep_fast<false>"]
    check(Ro, Ro.score(), Rg, form + ": ")
    Rg.close()
    Ro.close()
