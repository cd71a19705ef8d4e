"""Every specialisation uvc_launch_accumulate can pick, against the oracle.

A matrix of (tile, parameter arm) x forced switches.  Per (tile, arm) one oracle run; on the GPU one handle per (UVCGPU_FRAG32, UVCGPU_FAM_PATH)
-- both are read by set_reads -- and on it two accumulates, UVCGPU_SPLIT=0 and then 1 (read by every accumulate: the second also checks that
the first form left the transient bucket planes clean for the other).  Each accumulate must print the forms line expected_forms computes
(tests/kernel_forms.py), leave all 14 plane groups bit-exact, and give score records within the tolerance classes of test_gpu_parity.py."""
import functools

import pytest

from uvc_amd import region, synth
from kernel_forms import ARMS, STACK, TILES, arm_params, expected_forms, forms_match, parse_forms, switches
from test_gpu_parity import compare_records
from util import amplicon_stack, diff_groups

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def tile_reads(tile):
    reads = synth.generate_region(**TILES[tile]["gen"])
    if TILES[tile]["amplicon"]:
        reads["fam_dflag"] = reads["fam_dflag"].copy()
        reads["fam_dflag"][::2] |= 0x4
    return reads


def params(lib, arm):
    return arm_params(region.default_params(lib, platform=ARMS[arm].get("platform", 1)), arm)


def set_switch(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def check_cell(label, Ro, ro, R, want, err):
    """One accumulate on the GPU handle R: its forms line, its planes and its records.  -> a list of failure lines naming the cell."""
    bad = []
    lines = parse_forms(err)
    if len(lines) != 1 or not forms_match(lines[0], want):
        bad.append("%s: forms line %s, expected %s" % (label, lines, want))
    diff = diff_groups(Ro, R)
    bad += ["%s: %s: %d cells differ, first (index, oracle, gpu) %s" % (label, g, v[0], v[1]) for g, v in diff.items()]
    if ro is not None:
        try:
            compare_records(ro, R.score(all_out=False))
        except AssertionError as e:
            bad.append("%s: records: %s" % (label, e))
    return bad


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("tile", list(TILES))
def test_every_form_matches_the_oracle(tile, arm, oracle_lib, gpu_lib, monkeypatch, capfd):
    reads = tile_reads(tile)
    Ro = region.Region(oracle_lib, params(oracle_lib, arm), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Ro.set_reads(reads)
    Ro.accumulate()
    p = params(gpu_lib, arm)
    ro = Ro.score(all_out=False) if p.inferred_is_vcf_generated else None   # (no scoring on a FASTQ-only run, as in test_parameter_variants)
    failures, n_cells = [], 0
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    try:
        for frag32, fam_path, splits in switches(tile):
            set_switch(monkeypatch, "UVCGPU_FRAG32", "1" if frag32 else None)
            set_switch(monkeypatch, "UVCGPU_FAM_PATH", fam_path)
            R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
            capfd.readouterr()
            R.set_reads(reads)
            fam_line = [l for l in capfd.readouterr().err.splitlines() if "family form" in l]
            want_family = TILES[tile]["family"] if TILES[tile]["family"] == "none" or fam_path is None else "generic"
            if want_family != "none":   # the set_reads line names the form it chose
                assert len(fam_line) == 1 and fam_line[0].endswith("family form " + want_family), (tile, arm, fam_path, fam_line)
            for split in splits:
                monkeypatch.setenv("UVCGPU_SPLIT", split)
                R.accumulate()
                err = capfd.readouterr().err
                label = "%s / %s / FRAG32=%s FAM_PATH=%s SPLIT=%s" % (tile, arm, int(frag32), fam_path or "auto", split)
                want = expected_forms(p, TILES[tile], split, frag32=frag32, fam_generic=(fam_path == "generic"))
                failures += check_cell(label, Ro, ro, R, want, err)
                n_cells += 1
            R.close()
    finally:
        for name in ("UVCGPU_TIMING", "UVCGPU_FRAG32", "UVCGPU_FAM_PATH", "UVCGPU_SPLIT"):
            monkeypatch.delenv(name, raising=False)
        Ro.close()
    assert not failures, "%d of %d cells fail:\n" % (len({f.split(":")[0] for f in failures}), n_cells) + "\n".join(failures)


def test_32_bit_buckets_without_forcing_match_the_oracle(oracle_lib, gpu_lib, monkeypatch, capfd):
    """The 70 000-read stack under fam_flag=1: more than 65 535 fragments on a position and the SSCS-table arm take k_frag<false> by
    themselves (no switch forced)."""
    reads = amplicon_stack()
    Ro = region.Region(oracle_lib, params(oracle_lib, "sscs_table"), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Ro.set_reads(reads)
    Ro.accumulate()
    p = params(gpu_lib, "sscs_table")
    for name in ("UVCGPU_FRAG32", "UVCGPU_FAM_PATH", "UVCGPU_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    capfd.readouterr()
    R.accumulate()
    err = capfd.readouterr().err
    monkeypatch.delenv("UVCGPU_TIMING")
    want = expected_forms(p, STACK, None)
    assert want["frag"] == "b32,wave,generic"
    failures = check_cell("amplicon_stack / sscs_table / no switch", Ro, Ro.score(all_out=False), R, want, err)
    assert R.fetch("FRAG")[:, 0].sum(axis=(0, 1)).max() >= 65536
    R.close()
    Ro.close()
    assert not failures, "\n".join(failures)
