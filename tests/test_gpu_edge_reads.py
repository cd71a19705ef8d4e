"""The 16-bit fields and fall-backs of the accumulate work list, and long reads, against the oracle (inputs: tests/edge_reads.py; their
preconditions: tests/test_edge_reads_cpu.py).  Every cell: all 14 plane groups bit-exact, no presence violation, the InDel allele rows and the
three haplotype-link maps equal, the records within the classes of test_gpu_parity.compare_records (all-out for the small regions, the default
gate for the 66.5 kb one).  One oracle run per input, shared and never changed.

Before FastRec::clips saturated its halves (fill_fastrec), `clips` failed here in PREP32 only: the a_near_long_clip_dp cells of the six clips of
65 536 bases and more (positions 67, 114, 220, 255, 267, 351 of the region) were 0 where the oracle has 1 (ordinary families), and the two
five-position a_near_pcr_clip_dp windows of the clips of exactly 65 536 (65 .. 69, 218 .. 222) were missing (amplicon families).  Nothing else
in this file differed."""
import numpy as np
import pytest

from uvc_amd import region
import edge_reads as er
from test_gpu_device_reads import DeviceColumns
from test_gpu_parity import compare_records
from util import INT_GROUPS, diff_groups, presence_violations

pytestmark = pytest.mark.gpu

_oracle_runs = {}


def oracle_run(oracle_lib, key, reads, platform=1, all_out=True):
    """The oracle's handle, records, allele rows and links of an input, computed once and shared (never changed) by the tests that need it."""
    if key not in _oracle_runs:
        Ro = region.Region(oracle_lib, region.default_params(oracle_lib, platform=platform), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        Ro.set_reads(reads)
        Ro.accumulate()              # refuses none of these inputs (tests/test_edge_reads_cpu.py)
        _oracle_runs[key] = (Ro, Ro.score(all_out=all_out), Ro.indel_alleles(), Ro.hap_links(), all_out)
    return _oracle_runs[key]


def gpu_handle(gpu_lib, reads, platform=1, device=False, handle=None):
    """set_reads (host columns) or set_reads_device (compact columns in HBM) + accumulate, on a fresh handle or on `handle` after a reset."""
    if handle is None:
        R = region.Region(gpu_lib, region.default_params(gpu_lib, platform=platform), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    else:
        R = handle
        R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    cols = None
    if device:
        cols = DeviceColumns(region.compact_form(reads))
        R.set_reads_device((cols.soa, cols))
    else:
        R.set_reads(reads)
    R.accumulate()
    R.fetch("PREP32")                # surfaces device-side error flags
    return R, cols


def check(oracle, Rg, what=""):
    Ro, ro, alleles, links, all_out = oracle
    assert len(INT_GROUPS) == 14
    bad = diff_groups(Ro, Rg)
    assert not bad, what + "\n".join("%s: %d cells differ, e.g. %s" % (g, v[0], v[1]) for g, v in bad.items())
    assert presence_violations(Rg) == 0, what
    assert Rg.indel_alleles() == alleles, what
    assert Rg.hap_links() == links, what
    compare_records(ro, Rg.score(all_out=all_out))


def compare(oracle_lib, gpu_lib, key, reads, platform=1, device=False, all_out=True):
    oracle = oracle_run(oracle_lib, key, reads, platform, all_out)
    Rg, cols = gpu_handle(gpu_lib, reads, platform, device)
    try:
        check(oracle, Rg)
    finally:
        Rg.close()
        if cols: cols.free()


def set_switch(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("UVCGPU_SPLIT", "UVCGPU_FRAG32", "UVCGPU_FAM_PATH"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("amplicon", [False, True])
def test_clips(amplicon, reverse, device, oracle_lib, gpu_lib):
    """Clip ops of 32 767 .. 131 075 bases beside the M run of a simple alignment, in ordinary and in amplicon families (both arms of clip_event)."""
    compare(oracle_lib, gpu_lib, ("clips", amplicon, reverse), er.clips(amplicon, reverse)["reads"], device=device)


def test_clips_with_a_minimum_length_beyond_16_bits(oracle_lib, gpu_lib):
    """microadjust_alignment_clip_min_len = 65 537: a saturated half alone would call every clip of 65 535 and more long; the oracle counts the
    clips of 65 537, 65 539, 65 540 and 131 075 and not the four of 65 535 and 65 536."""
    reads = er.clips(False, False)["reads"]
    out = []
    for lib in (oracle_lib, gpu_lib):
        P = region.default_params(lib)
        P.microadjust_alignment_clip_min_len = 65537
        R = region.Region(lib, P, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        R.set_reads(reads)
        R.accumulate()
        out.append(R)
    assert int(out[0].fetch("PREP32")[11].sum()) == 4      # UVC_P_a_near_long_clip_dp
    bad = diff_groups(*out)
    assert not bad, "\n".join("%s: %d cells differ, e.g. %s" % (g, v[0], v[1]) for g, v in bad.items())
    for R in out:
        R.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("platform", [1, 2])
@pytest.mark.parametrize("beg", [100_000, 1_000])
def test_run_offsets(beg, platform, device, oracle_lib, gpu_lib):
    """M runs 65 535 / 65 536 from either end of a 66 kb alignment with sixty InDels, deletions of 32 766 .. 65 536, a 66 000-base skip, fragment
    spans of 65 535 .. 65 537; with and without InDel reads on the work list (region begin below 65 536, IonTorrent)."""
    compare(oracle_lib, gpu_lib, ("run_offsets", beg, platform), er.run_offsets(beg)["reads"], platform=platform, device=device, all_out=False)


def test_run_offsets_on_a_handle_that_held_clips(oracle_lib, gpu_lib):
    """600 positions, then 66 500 on the same handle, then 600 again: the work list, the item lists and the planes grow and shrink."""
    small, large = er.clips(False, False)["reads"], er.run_offsets(100_000)["reads"]
    R = None
    for k, (key, reads, all_out) in enumerate(((("clips", False, False), small, True), (("run_offsets", 100_000, 1), large, False), (("clips", False, False), small, True))):
        oracle = oracle_run(oracle_lib, key, reads, 1, all_out)
        R, _ = gpu_handle(gpu_lib, reads, handle=R)
        check(oracle, R, "use %d: " % k)
    R.close()


@pytest.mark.parametrize("beg", [0, 65535, 65536])
def test_region_begin(beg, oracle_lib, gpu_lib):
    """The region begin decides whether any InDel read may take the work-list path (the M-run offsets are stored against 16 bits)."""
    compare(oracle_lib, gpu_lib, ("region_begin", beg), er.region_begin(beg)["reads"])


def test_nm_penalty_at_the_limit(oracle_lib, gpu_lib):
    """by_nm + by_clip = -30 000 exactly, by NM alone and by NM and a soft clip: the lowest penalty the 16-bit value fields take."""
    compare(oracle_lib, gpu_lib, ("nm_penalty", False), er.nm_penalty(False)["reads"])


def test_nm_penalty_below_the_limit_is_refused(gpu_lib):
    """-30 001: UVCGPU_EUNSUPPORTED (the documented limit), not a wrapped value."""
    reads = er.nm_penalty(True)["reads"]
    R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    with pytest.raises(region.UvcError) as e:
        R.set_reads(reads)
        R.accumulate()
        R.fetch("PREP32")
    assert e.value.code == er.EUNSUPPORTED, e.value
    R.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("which", er.LONG_FUZZ)
def test_long_fuzz(which, device, oracle_lib, gpu_lib):
    """Fuzzed reads of up to 3 000 reference bases; single M runs of 4 095 .. 8 213 bases at 1 % mismatches, whole and with one deletion."""
    compare(oracle_lib, gpu_lib, ("long_fuzz", which), er.long_fuzz(which)["reads"], device=device)


@pytest.mark.parametrize("split", ["0", "1"])
def test_long_fuzz_by_both_forms_of_the_window_kernels(split, oracle_lib, gpu_lib, monkeypatch):
    monkeypatch.setenv("UVCGPU_SPLIT", split)
    compare(oracle_lib, gpu_lib, ("long_fuzz", "runs_4096_del"), er.long_fuzz("runs_4096_del")["reads"])


FRAG32_INPUTS = {
    "clips": lambda: (("clips", False, False), er.clips(False, False)["reads"], True),
    "run_offsets": lambda: (("run_offsets", 100_000, 1), er.run_offsets(100_000)["reads"], False),
    "region_begin": lambda: (("region_begin", 65536), er.region_begin(65536)["reads"], True),
    "nm_penalty": lambda: (("nm_penalty", False), er.nm_penalty(False)["reads"], True),
    **{"long_" + w: (lambda w=w: (("long_fuzz", w), er.long_fuzz(w)["reads"], True)) for w in er.LONG_FUZZ},
    "planted_haplotypes": lambda: (("planted_haplotypes",), er.planted_haplotypes()["reads"], True),
}


@pytest.mark.parametrize("name", list(FRAG32_INPUTS))
def test_with_32_bit_buckets(name, oracle_lib, gpu_lib, monkeypatch):
    """UVCGPU_FRAG32=1 (read by set_reads): k_frag<false> on inputs that would take the 16-bit bucket counters."""
    monkeypatch.setenv("UVCGPU_FRAG32", "1")
    key, reads, all_out = FRAG32_INPUTS[name]()
    compare(oracle_lib, gpu_lib, key, reads, all_out=all_out)


@pytest.mark.parametrize("device", [False, True])
def test_planted_haplotypes(device, oracle_lib, gpu_lib):
    """The only input of the suite's fuzz family with haplotype links: six events per form, ten 64-position chunks between the first and the
    last, an insertion and a base at one position; and a fragment of about 90 events."""
    oracle = oracle_run(oracle_lib, ("planted_haplotypes",), er.planted_haplotypes()["reads"])
    assert all(len(m) >= 1 for m in oracle[3])      # (tests/test_edge_reads_cpu.py says what they hold)
    compare(oracle_lib, gpu_lib, ("planted_haplotypes",), er.planted_haplotypes()["reads"], device=device)
