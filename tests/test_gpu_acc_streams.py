"""The side streams of uvc_launch_accumulate (uvc_amd/csrc/uvc_kernels_acc.hip) against one stream, and the overflow sweep's strided grid.

A handle created under UVCGPU_ONE_STREAM=1 runs every kernel of the accumulate on its one stream, in the order of the launches; a handle
created without it deals them to three streams ordered by events (the dependency table in front of uvc_launch_accumulate).  Both must leave
the same planes, allele rows and records bit for bit, and the three-stream handle the same ones round after round with nothing but stream
order between an accumulate and its score."""
import functools

import numpy as np
import pytest

from uvc_amd import region, synth
from kernel_forms import IONTORRENT, TILES
from test_gpu_parity import compare_records, set_validator
from util import diff_groups

pytestmark = pytest.mark.gpu

# gen: synth.generate_region; platform: 1 Illumina-like, 2 IonTorrent (no k_frag_sums, every fragment through k_frag_generic); env: the
# switches tests/test_gpu_kernel_forms.py forces, here so that the duplex tile takes the split window kernels beside the digest family form
CASES = {
    "paired_2kb_300x_indel_reads": dict(gen=dict(region_len=2000, depth=300, seed=31, indel_every=150, snv_every=100, clip_frac=0.05, variant_inset=200), platform=1, env={}),
    "umi_duplex_2kb_400x_split_digest": dict(gen=TILES["umi_duplex_2kb_400x"]["gen"], platform=1, env={"UVCGPU_SPLIT": "1"}),
    "iontorrent_2kb_100x": dict(gen=dict(region_len=2000, depth=100, seed=32, indel_every=300, clip_frac=0.05, variant_inset=200), platform=IONTORRENT, env={}),
    "no_indel_reads_2kb_300x": dict(gen=dict(region_len=2000, depth=300, seed=33, indel_every=0, clip_frac=0.0), platform=1, env={}),
}
ROUNDS = 10


@functools.lru_cache(maxsize=None)
def case_reads(name):
    return synth.generate_region(**CASES[name]["gen"])


def new_handle(lib, name, reads, monkeypatch, one_stream):
    """A handle for the case; UVCGPU_ONE_STREAM is read when the handle is created, and only then."""
    if one_stream:
        monkeypatch.setenv("UVCGPU_ONE_STREAM", "1")
    else:
        monkeypatch.delenv("UVCGPU_ONE_STREAM", raising=False)
    try:
        return region.Region(lib, region.default_params(lib, platform=CASES[name]["platform"]), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    finally:
        monkeypatch.delenv("UVCGPU_ONE_STREAM", raising=False)


def same_records(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])] + [k for k in b if k not in a]


@pytest.mark.parametrize("name", list(CASES))
def test_side_streams_equal_one_stream(name, oracle_lib, gpu_lib, monkeypatch, capfd):
    reads = case_reads(name)
    n_indel_reads = int((reads["n_cigar"] > 1).sum())
    assert (n_indel_reads == 0) == (name == "no_indel_reads_2kb_300x"), n_indel_reads
    for k, v in CASES[name]["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    R1 = new_handle(gpu_lib, name, reads, monkeypatch, one_stream=True)
    R3 = new_handle(gpu_lib, name, reads, monkeypatch, one_stream=False)
    try:
        capfd.readouterr()
        for R in (R1, R3):
            R.set_reads(reads)
            R.accumulate()
        forms = [l for l in capfd.readouterr().err.splitlines() if "[uvcgpu accumulate] forms" in l]
        monkeypatch.delenv("UVCGPU_TIMING")
        assert len(forms) == 2 and forms[0] == forms[1], forms
        if name == "umi_duplex_2kb_400x_split_digest":
            assert "prep=split" in forms[0] and "family=digest" in forms[0] and "duplex=digest" in forms[0], forms[0]
        if name == "iontorrent_2kb_100x":
            assert "frag_generic=all" in forms[0], forms[0]
        bad = diff_groups(R1, R3)
        assert not bad, "\n".join("%s: %d cells differ, first (index, one stream, three streams) %s" % (g, v[0], v[1]) for g, v in bad.items())
        alleles = R3.indel_alleles()
        assert R1.indel_alleles() == alleles
        if n_indel_reads == 0:
            assert alleles == []
        elif CASES[name]["platform"] != IONTORRENT:
            assert len(alleles) > 0
        first = {}
        for all_out in (False, True):
            a, b = R1.score(all_out=all_out), R3.score(all_out=all_out)
            assert len(b["refpos"]) > 0
            assert not same_records(a, b), (all_out, same_records(a, b))
            first[all_out] = b
        planes = {g: R3.fetch(g).copy() for g in ("PREP32", "SEG32", "BQSUM", "FRAG", "FAM", "VQ")}
        if name == "paired_2kb_300x_indel_reads":   # once against the oracle
            Ro = region.Region(oracle_lib, region.default_params(oracle_lib, platform=CASES[name]["platform"]), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
            Ro.set_reads(reads)
            Ro.accumulate()
            bad = diff_groups(Ro, R3)
            assert not bad, "\n".join("%s: %d cells differ, first (index, oracle, gpu) %s" % (g, v[0], v[1]) for g, v in bad.items())
            compare_records(Ro.score(all_out=False), first[False])
            Ro.close()
        # accumulate + score with nothing but the streams between them (no presence check, no fetch in front of the score), the planes handed
        # back with every other score (zeroed on the side stream, where the next accumulate picks them up)
        set_validator(monkeypatch, "off")
        for k in range(ROUNDS):
            release = (k % 2 == 1)
            R3.accumulate()
            rec = R3.score(all_out=False, release_state=release)
            assert not same_records(first[False], rec), (k, same_records(first[False], rec))
            assert R3.indel_alleles() == alleles, k
            if not release:
                diff = [g for g in planes if not np.array_equal(R3.fetch(g), planes[g])]
                assert not diff, (k, diff)
    finally:
        R1.close()
        R3.close()


def test_overflow_list_longer_than_its_grid(oracle_lib, gpu_lib):
    """5 kb x 1000x of paired reads with 8 % base errors: nearly every fragment has more than UVC_MAXEV (8) mutation events and goes through the
    overflow sweep, whose list is then more than three times 4 096 entries long: under a grid of up to 4 096 blocks a launch that does not
    stride leaves n_cov / n_near of the rest at 0, which shows in FRAG (bTA / bTB).  (Lists beyond the 65 535 blocks of the present launch:
    tests/test_gpu_large.py, noisy_20kb_2000x.)"""
    reads = synth.generate_region(region_len=5000, depth=1000, seed=41, err_rate=0.08)
    n, L = reads["n_reads"], synth.READ_LEN
    ref = np.frombuffer(reads["refseq"].encode(), np.uint8)
    # counted conservatively: fragments of two whole-read matches (`L`M), bases of quality 30 and more (bias_thres_highBQ is 20) that differ
    # from the reference at a position only one of the two mates covers (where the fragment's consensus is that base)
    plain = (reads["n_cigar"] == 1) & (reads["cigars"][reads["cigar_off"]] == ((L << 4) | 0))
    x = (reads["pos"].astype(np.int64) - reads["beg"])[:, None] + np.arange(L)[None, :]
    x = np.where(plain[:, None], x, 0)
    bases, quals = reads["bases"].reshape(n, L), reads["quals"].reshape(n, L)
    frag = reads["frag_id"].astype(np.int64)
    n_frags = int(frag.max()) + 1
    lo, hi = np.full(n_frags, np.iinfo(np.int64).max), np.full(n_frags, -1)   # begin of the fragment's left and of its right mate
    np.minimum.at(lo, frag[plain], x[plain, 0])
    np.maximum.at(hi, frag[plain], x[plain, 0])
    alone = ~((x >= hi[frag][:, None]) & (x < (lo[frag] + L)[:, None]))   # outside [right begin, left end), the part both mates cover
    mism = plain[:, None] & alone & (quals >= 30) & (bases != np.frombuffer(b"ACGT", np.uint8).searchsorted(ref)[x])
    per_frag = np.bincount(frag, weights=mism.sum(axis=1), minlength=n_frags)
    whole = np.bincount(frag, weights=plain, minlength=n_frags) == 2
    n_over = int(((per_frag > 8) & whole).sum())
    print("fragments %d, with more than 8 mismatching bases %d" % (n_frags, n_over))
    assert n_over >= 3 * 4096, (n_frags, n_over)
    P = region.default_params(gpu_lib)
    Ro = region.Region(oracle_lib, region.default_params(oracle_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    Rg = region.Region(gpu_lib, P, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    try:
        for R in (Ro, Rg):
            R.set_reads(reads)
            R.accumulate()
        bad = diff_groups(Ro, Rg, groups=["FRAG", "VQ"])
        assert not bad, "\n".join("%s: %d cells differ, first (index, oracle, gpu) %s" % (g, v[0], v[1]) for g, v in bad.items())
    finally:
        Ro.close()
        Rg.close()
