"""The sparse form of the completion pass of LINK_M and its early phase inside the accumulate.

Where few windows need the 34 bias cells of LINK_M, a block of sixteen waves serves one window (k_p2_link_sparse): wave w walks slice w >> 2 of
class list w & 3, and the partial counters are added up in LDS.  UVCGPU_LINK_FORM=sparse | wave forces the form of an INDEL or POSITIONS pass,
UVCGPU_LINK=eager completes every window inside the accumulate with the wave / split form.  The three and the oracle must agree bit for bit in
every cell, whatever the streams, the split switch, the depth of a window's lists, and however often a window is asked for.  The accumulate
runs the INDEL scope twice, once beside the fragment kernels and once at its end; the windows run are the oracle's InDel windows either way.
The guard of k_enum (a LINK group in a window that is not complete fails the call) is active throughout."""
import functools
import re

import numpy as np
import pytest

from uvc_amd import region, synth
from test_gpu_acc_streams import CASES
from test_gpu_force_sites import compose
from test_gpu_link_lazy import ALL_CASES, INDELS, case_of, differing, differing_planes, edge_tile, oracle_state, params_for, planes_of, tile
from test_gpu_parity import compare_records, set_validator, tumor_keys_from

pytestmark = pytest.mark.gpu

LINK_M = 6


def set_mode(monkeypatch, mode):
    """mode: "sparse" or "wave" (UVCGPU_LINK_FORM, read on every call), "eager" (UVCGPU_LINK, read on every accumulate), None (the oracle)."""
    if mode == "eager":
        monkeypatch.setenv("UVCGPU_LINK", "eager")
        monkeypatch.delenv("UVCGPU_LINK_FORM", raising=False)
    else:
        monkeypatch.delenv("UVCGPU_LINK", raising=False)
        if mode:
            monkeypatch.setenv("UVCGPU_LINK_FORM", mode)
        else:
            monkeypatch.delenv("UVCGPU_LINK_FORM", raising=False)


def make(lib, reads, monkeypatch, mode, params, one_stream=False, env=None):
    """An accumulated handle.  The mode's switches stay set: the caller finishes with one handle before it makes the next."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    set_mode(monkeypatch, mode)
    if one_stream:
        monkeypatch.setenv("UVCGPU_ONE_STREAM", "1")   # read when the handle is created
    try:
        R = region.Region(lib, params, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    finally:
        monkeypatch.delenv("UVCGPU_ONE_STREAM", raising=False)
    R.set_reads(reads)
    R.accumulate()
    return R


def link_lines(capfd):
    return [l for l in capfd.readouterr().err.splitlines() if l.startswith("[uvcgpu link_complete]")]


def done_of(line):
    m = re.search(r"scope=(\w+) done=(\d+) of (\d+) windows", line)
    return m.group(1), int(m.group(2)), int(m.group(3))


def indel_windows_of(planes, npos):
    """The 64-position windows in which the oracle's SEG32 / FAM planes hold a cell of a LINK symbol other than LINK_M."""
    any_ = np.zeros(npos, bool)
    for g in ("SEG32", "FAM"):
        a = planes[g][..., LINK_M + 1:, :] != 0   # [.., symbol, position]
        any_ |= a.reshape(-1, a.shape[-1]).any(axis=0)
    return set((np.nonzero(any_)[0] >> 6).tolist())


VARIANTS = {"streams": dict(), "one_stream": dict(one_stream=True), "split0": dict(env={"UVCGPU_SPLIT": "0"}), "split1": dict(env={"UVCGPU_SPLIT": "1"})}


@pytest.mark.parametrize("validator", ["on", "off"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ALL_CASES)
def test_forms_agree(name, variant, validator, oracle_lib, gpu_lib, monkeypatch):
    set_validator(monkeypatch, validator)
    want = oracle_state(oracle_lib, name)
    reads = tile(name)
    got = {}
    for mode in ("sparse", "wave", "eager"):
        v = VARIANTS[variant]
        R = make(gpu_lib, reads, monkeypatch, mode, params_for(gpu_lib, name), one_stream=v.get("one_stream", False), env=dict(case_of(name)["env"], **v.get("env", {})))
        try:
            o = dict(default=R.score(all_out=False), kept=R.score(all_out=False, kept_only=True))   # nothing between the accumulate and the score
            o["planes"], o["alleles"] = planes_of(R), R.indel_alleles()
            R.accumulate()
            o["default2"], o["all_out"] = R.score(all_out=False), R.score(all_out=True)
            got[mode] = o
        finally:
            R.close()
    s = got["sparse"]
    assert len(s["default"]["refpos"]) > 0
    for other in ("wave", "eager"):
        for k in ("default", "kept", "default2", "all_out"):
            assert not differing(s[k], got[other][k]), (other, k, differing(s[k], got[other][k]))
        assert not differing_planes(got[other]["planes"], s["planes"]), (other, differing_planes(got[other]["planes"], s["planes"]))
        assert s["alleles"] == got[other]["alleles"]
    assert not differing(s["default"], s["default2"])
    compare_records(want["default"], s["default"])
    compare_records(want["all_out"], s["all_out"])
    assert not differing_planes(want["planes"], s["planes"]), differing_planes(want["planes"], s["planes"])
    assert s["alleles"] == want["alleles"]


# ---- slicing: a class list of a window against the slices of the block's waves ----
def one_strand_tile():
    """The hand-made tile with every read on the forward strand: only one of a window's four class lists holds anything."""
    reads = dict(edge_tile())
    reads["flag"] = np.zeros(reads["n_reads"], np.uint16)
    reads["fam_strand"] = np.zeros(reads["n_reads"], np.uint8)
    return reads


@functools.lru_cache(maxsize=None)
def slicing_tile(name):
    if name == "deep_1kb_3000x":   # about 1 000 records per class and window: every slice of sixteen waves holds more than 64
        return synth.generate_region(region_len=1000, depth=3000, seed=51, indel_every=150, snv_every=100, clip_frac=0.05, variant_inset=200)
    if name == "thin_2kb_4x":      # one to three records in a class of a window: fewer than there are slices
        return synth.generate_region(region_len=2000, depth=4, seed=52, indel_every=150, snv_every=100, clip_frac=0.0, variant_inset=200)
    return one_strand_tile()


@functools.lru_cache(maxsize=None)
def slicing_oracle(lib, name):
    reads = slicing_tile(name)
    R = region.Region(lib, region.default_params(lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    R.accumulate()
    out = planes_of(R)
    R.close()
    return out


def test_thin_tile_has_classes_shorter_than_the_slices():
    """Worth its name: windows whose class lists begin with one, two and three reads each exist (counted from the reads' begins)."""
    reads = slicing_tile("thin_2kb_4x")
    plain = reads["n_cigar"] == 1
    cls = ((reads["flag"][plain] & 16) != 0).astype(np.int64)
    w = (reads["pos"][plain].astype(np.int64) - reads["beg"]) >> 6
    counts = np.bincount(w[w >= 0] * 2 + cls[w >= 0])
    assert {1, 2, 3} <= set(counts.tolist()), sorted(set(counts.tolist()))


@pytest.mark.parametrize("validator", ["on", "off"])
@pytest.mark.parametrize("name", ["deep_1kb_3000x", "one_strand_2kb", "thin_2kb_4x"])
def test_slices_of_long_empty_and_short_class_lists(name, validator, oracle_lib, gpu_lib, monkeypatch, capfd):
    """Every window through the sparse form (POSITIONS at one position per window, forced), then the planes against the oracle's."""
    set_validator(monkeypatch, validator)
    reads, want = slicing_tile(name), slicing_oracle(oracle_lib, name)
    npos = reads["end"] - reads["beg"]
    R = make(gpu_lib, reads, monkeypatch, "sparse", region.default_params(gpu_lib))
    try:
        monkeypatch.setenv("UVCGPU_TIMING", "1")
        capfd.readouterr()
        R.fetch_columns(reads["beg"] + np.arange(0, npos + 64, 64).clip(max=npos))
        lines = link_lines(capfd)
        monkeypatch.delenv("UVCGPU_TIMING")
        scope, done, nwin = done_of(lines[-1])
        assert scope == "positions" and done == nwin == (npos + 1 + 63) // 64, lines
        got = planes_of(R)
        assert not differing_planes(want, got), differing_planes(want, got)
        assert (got["SEG32"][:, LINK_M, :] != 0).any(axis=1).sum() > 4   # more planes of LINK_M than the four aDP** hold something
    finally:
        R.close()


@pytest.mark.parametrize("validator", ["on", "off"])
def test_positions_at_window_edges_with_duplicates_and_strays(validator, oracle_lib, gpu_lib, monkeypatch, capfd):
    set_validator(monkeypatch, validator)
    name = "no_indel_reads_2kb_300x"   # the accumulate itself completes no window
    reads = tile(name)
    npos = reads["end"] - reads["beg"] + 1   # plane indices 0 .. npos - 1
    xs = np.array([0, 63, 64, npos - 1, 63, 0, 64, -5, npos, npos + 70, npos - 1])
    cols = {}
    for mode in ("sparse", "eager"):
        R = make(gpu_lib, reads, monkeypatch, mode, params_for(gpu_lib, name))
        try:
            monkeypatch.setenv("UVCGPU_TIMING", "1")
            capfd.readouterr()
            cols[mode] = R.fetch_columns(reads["beg"] + xs)
            lines = link_lines(capfd)
            monkeypatch.delenv("UVCGPU_TIMING")
            if mode == "sparse":
                assert len(lines) == 1 and done_of(lines[0])[:2] == ("positions", len({0, 1, (npos - 1) >> 6})), lines
                got = planes_of(R)
                want = oracle_state(oracle_lib, name)["planes"]
                assert not differing_planes(want, got), differing_planes(want, got)
        finally:
            R.close()
    assert np.array_equal(cols["sparse"], cols["eager"])
    assert cols["sparse"].any() and not cols["sparse"][7:10].any()   # (the strays give rows of zeros)


@pytest.mark.parametrize("validator", ["on", "off"])
@pytest.mark.parametrize("name", ["paired_2kb_300x_indel_reads", "window_edges"])
def test_a_window_asked_for_again_is_run_once(name, validator, oracle_lib, gpu_lib, monkeypatch):
    """POSITIONS, the same POSITIONS again, then ALL through a fetch of SEG32: a window run twice shows as doubled counters."""
    set_validator(monkeypatch, validator)
    reads, want = tile(name), oracle_state(oracle_lib, name)["planes"]
    npos = reads["end"] - reads["beg"]
    R = make(gpu_lib, reads, monkeypatch, "sparse", params_for(gpu_lib, name))
    try:
        pos = reads["beg"] + np.arange(3, npos, 131)
        a = R.fetch_columns(pos)
        b = R.fetch_columns(pos)
        assert np.array_equal(a, b)
        assert np.array_equal(R.fetch("SEG32"), want["SEG32"])
        got = planes_of(R)
        assert not differing_planes(want, got), differing_planes(want, got)
    finally:
        R.close()


# ---- the early and the final phase of the accumulate ----
@functools.lru_cache(maxsize=None)
def family_tile():
    """InDel reads and duplicate families: n_generic_fs > 0, so the family kernels run between the two phases."""
    return synth.generate_region(region_len=3000, depth=200, seed=53, umi=True, indel_every=150, snv_every=100, clip_frac=0.05, variant_inset=200)


@pytest.mark.parametrize("validator", ["on", "off"])
def test_early_and_final_phase_run_the_oracles_indel_windows(validator, oracle_lib, gpu_lib, monkeypatch, capfd):
    set_validator(monkeypatch, validator)
    reads = family_tile()
    assert len(np.unique(reads["fam_id"])) < reads["n_reads"] // 2   # families of more than one read
    Ro = make(oracle_lib, reads, monkeypatch, None, region.default_params(oracle_lib))
    want = planes_of(Ro)
    Ro.close()
    npos = reads["end"] - reads["beg"] + 1
    windows = indel_windows_of(want, want["SEG32"].shape[-1])
    done = {}
    for one_stream in (False, True):
        monkeypatch.setenv("UVCGPU_TIMING", "1")
        capfd.readouterr()
        R = make(gpu_lib, reads, monkeypatch, None, region.default_params(gpu_lib), one_stream=one_stream)
        try:
            err = capfd.readouterr().err.splitlines()
            monkeypatch.delenv("UVCGPU_TIMING")
            lines = [l for l in err if l.startswith("[uvcgpu link_complete]")]
            forms = [l for l in err if l.startswith("[uvcgpu link_form]")]
            assert len(lines) == 1 and done_of(lines[0])[0] == "indel", lines
            assert forms == ["[uvcgpu link_form] scope=indel form=sparse"] * 2, forms   # the early and the final phase
            assert any("family=" in l and "family=none" not in l for l in err if "[uvcgpu accumulate] forms" in l), err
            done[one_stream] = done_of(lines[0])[1]
            nwin = done_of(lines[0])[2]
            assert len(R.score(all_out=False)["refpos"]) > 0
            got = planes_of(R)
            assert not differing_planes(want, got), differing_planes(want, got)
        finally:
            R.close()
    print("windows run with side streams %d, on one stream %d, InDel windows of the oracle %d of %d" % (done[False], done[True], len(windows), nwin))
    assert done[False] == done[True] == len(windows)
    assert 4 <= len(windows) < nwin and nwin == (npos + 63) // 64


# ---- scopes where the host knows the positions ----
@pytest.mark.parametrize("validator", ["on", "off"])
def test_keyed_and_forced_scopes_complete_their_windows_only(validator, oracle_lib, gpu_lib, monkeypatch, capfd):
    """The layout of test_tumor_keys_and_forced_sites_away_from_indels: a normal pass keyed at SNV positions in windows without an InDel, and
    forced sites in such windows behind a default-gate score."""
    set_validator(monkeypatch, validator)
    name = "paired_2kb_300x_indel_reads"
    reads, rec = tile(name), oracle_state(oracle_lib, name)["default"]
    beg = reads["beg"]
    indel_windows = {int(p - beg) >> 6 for p, s in zip(rec["refpos"], rec["symbol"]) if s in INDELS}
    snv = {k: v[(rec["symbol"] <= 5) & ~np.isin((rec["refpos"] - beg) >> 6, sorted(indel_windows))] for k, v in rec.items()}
    keys = tumor_keys_from(snv)
    sites = [int(beg + x) for x in range(130, reads["end"] - beg - 130, 97) if (x >> 6) not in indel_windows]
    assert len(keys) >= 4 and len(sites) >= 8 and indel_windows
    out, done = {}, {}
    for who, lib, mode in (("oracle", oracle_lib, None), ("eager", gpu_lib, "eager"), ("sparse", gpu_lib, "sparse")):
        Rn = make(lib, reads, monkeypatch, mode, params_for(lib, name, tumor_vcf_is_provided=1))
        Rf = make(lib, reads, monkeypatch, mode, params_for(lib, name))
        try:
            if who == "sparse":
                Rf.score(all_out=False)   # a default-gate score first: the forced sites then complete what it left
                monkeypatch.setenv("UVCGPU_TIMING", "1")
            capfd.readouterr()
            a = Rn.score(tumor_keys=keys)
            done["keys"] = link_lines(capfd)
            b = Rf.score(all_out=False, force_sites=sites)
            done["sites"] = link_lines(capfd)
            monkeypatch.delenv("UVCGPU_TIMING", raising=False)
            out[who] = (a, b)
        finally:
            Rn.close()
            Rf.close()
    want = (out["oracle"][0], compose(rec, oracle_state(oracle_lib, name)["all_out"], sites))
    for i in range(2):
        assert len(out["sparse"][i]["refpos"]) > len(rec["refpos"]) * i
        assert not differing(out["eager"][i], out["sparse"][i]), (i, differing(out["eager"][i], out["sparse"][i]))
        compare_records(want[i], out["sparse"][i])
    for what, asked in (("keys", {(k[0] - beg) >> 6 for k in keys}), ("sites", {(p - beg) >> 6 for p in sites})):
        assert len(done[what]) == 1, done[what]
        scope, n, nwin = done_of(done[what][0])
        print(what, "windows done %d of %d, asked for %d, InDel windows %d" % (n, nwin, len(asked), len(indel_windows)))
        assert scope == "positions" and len(asked) <= n <= len(asked | indel_windows) + 4 and n < nwin, done[what]


# ---- handle reuse ----
@pytest.mark.parametrize("validator", ["on", "off"])
def test_rounds_release_and_reset(validator, oracle_lib, gpu_lib, monkeypatch):
    """Ten accumulate + score rounds, the planes handed back with every other score; then another region on the same handle and back."""
    set_validator(monkeypatch, validator)
    name, other = "paired_2kb_300x_indel_reads", "window_edges"
    want = {nm: oracle_state(oracle_lib, nm) for nm in (name, other)}
    R = make(gpu_lib, tile(name), monkeypatch, "sparse", params_for(gpu_lib, name))
    try:
        first = R.score(all_out=False)
        compare_records(want[name]["default"], first)
        for k in range(10):
            R.accumulate()
            rec = R.score(all_out=False, release_state=(k % 2 == 1))
            assert not differing(first, rec), (k, differing(first, rec))
        for nm in (other, name):
            reads = tile(nm)
            R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
            R.set_reads(reads)
            R.accumulate()
            compare_records(want[nm]["default"], R.score(all_out=False))
            compare_records(want[nm]["all_out"], R.score(all_out=True))
            got = planes_of(R)
            assert not differing_planes(want[nm]["planes"], got), (nm, differing_planes(want[nm]["planes"], got))
        assert not differing(first, R.score(all_out=False))
    finally:
        R.close()
