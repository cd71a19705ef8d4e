"""The bias counters of LINK_M are made where somebody reads them.

An accumulate leaves the 34 cells of LINK_M beyond aDP** / BQSUM complete only in the 64-position windows with an InDel mark; every reader of
the others sends the completion pass first (link_complete, uvc_amd/csrc/uvc_host.cpp).  UVCGPU_LINK=eager completes every window inside the
accumulate.  A lazy handle, an eager handle and the oracle must agree: the default-gate records with nothing between accumulate and score,
all 14 plane groups and the allele rows fetched behind that score, -A, tumor keys and forced sites on the same accumulate, round after round,
across a reset, and with InDels on the edges of the windows.  The guard of k_enum (a LINK group whose window is not complete fails the call)
is active throughout and must stay silent; nothing here provokes it."""
import functools

import numpy as np
import pytest

from uvc_amd import region, synth
from test_gpu_acc_streams import CASES, case_reads
from test_gpu_force_sites import compose
from test_gpu_parity import compare_records, set_validator, tumor_keys_from
from util import INT_GROUPS

pytestmark = pytest.mark.gpu

INDELS = (7, 8, 9, 10, 11, 12)   # D3P D2 D1 I3P I2 I1
# Anchors of the hand-made tile: the base in front of an insertion and of a deletion, as region offsets; the InDel's records are at anchor + 1.
# 62 and 63 put them on the last position of window 0 and the first of window 1.  5 and EDGE_LEN - 11 are the nearest to the region's ends at
# which the oracle still gives both a default-gate record (probed on the CPU: an InDel within five bases of the first or ten of the last
# position gets none or one, and offsets 0 and npos - 1 are outside the default score range), so those two stand in for "first" and "last".
EDGE_LEN = 2000
EDGE_ANCHORS = (5, 62, 63, EDGE_LEN - 11)
# The very ends all the same: an insertion and a deletion behind offset 0, and an insertion behind the last reference base (its symbol lies at
# npos - 1).  No default-gate record, but the planes and the -A records hold them.
EDGE_EXTRA = (0, EDGE_LEN - 1)


def edge_tile():
    """2 kb of unpaired reads, each a fragment and a family of its own: 40x of plain 100-base reads, and per anchor 24 reads with a 2-base
    insertion and 24 with a 2-base deletion behind the anchor base.  The InDel reads reach at least 40 bases to either side where the region
    has them, so each also covers the neighbouring 64-position window."""
    rng = np.random.default_rng(77)
    n, beg, L = EDGE_LEN, 3_000_000, 100
    ref = rng.integers(0, 4, n)
    for a in EDGE_ANCHORS + EDGE_EXTRA:   # no repeat around an anchor: the InDel stays where the read puts it
        lo, hi = max(a - 3, 0), min(a + 6, n)
        ref[lo:hi] = (np.arange(lo, hi) + (ref[lo] if lo else 0)) % 4
    rows = []   # (pos, [(op, len)], bases)
    for s in range(0, n - L + 1, 5):   # 40x
        for _ in range(2):
            rows.append((s, [(0, L)], ref[s:s + L].copy()))
    for a in EDGE_ANCHORS + EDGE_EXTRA:
        left = min(a + 1, 60)   # aligned bases up to and including the anchor
        p0 = a + 1 - left
        for k in range(24):
            right = min(60, n - (a + 1))
            ins = np.array([(ref[min(a + 1, n - 1)] + 1) % 4, (ref[a] + 2) % 4])
            cig = [(0, left), (1, 2)] + ([(0, right)] if right else [])
            rows.append((p0, cig, np.concatenate([ref[p0:a + 1], ins, ref[a + 1:a + 1 + right]])))
            right_d = min(60, n - (a + 3))
            if right_d > 0:
                rows.append((p0, [(0, left), (2, 2), (0, right_d)], np.concatenate([ref[p0:a + 1], ref[a + 3:a + 3 + right_d]])))
    rows.sort(key=lambda r: r[0])
    m = len(rows)
    l_qseq = np.array([len(r[2]) for r in rows], np.int32)
    seq_off = np.zeros(m, np.int64); seq_off[1:] = np.cumsum(l_qseq[:-1])
    n_cigar = np.array([len(r[1]) for r in rows], np.int32)
    cigar_off = np.zeros(m, np.int64); cigar_off[1:] = np.cumsum(n_cigar[:-1])
    cigars = np.array([(ln << 4) | op for r in rows for op, ln in r[1]], np.uint32)
    nm = np.array([sum(ln for op, ln in r[1] if op) for r in rows], np.int32)
    return dict(n_reads=m, pos=np.array([beg + r[0] for r in rows], np.int32), mpos=np.full(m, -1, np.int32), isize=np.zeros(m, np.int32),
                flag=np.where(np.arange(m) % 2, 16, 0).astype(np.uint16), mapq=np.full(m, 60, np.uint8), nm=nm, l_qseq=l_qseq, seq_off=seq_off, cigar_off=cigar_off,
                n_cigar=n_cigar, frag_id=np.arange(m, dtype=np.int32), fam_id=np.arange(m, dtype=np.int32), fam_strand=(np.arange(m) % 2).astype(np.uint8), n_fams=m,
                fam_dflag=np.zeros(m, np.uint8), bases=np.concatenate([r[2] for r in rows]).astype(np.uint8), quals=np.full(int(l_qseq.sum()), 35, np.uint8), cigars=cigars,
                tid=2, beg=beg, end=beg + n, refseq="".join("ACGT"[b] for b in ref))


def tile(name):
    return edge_tile() if name == "window_edges" else case_reads(name)


def case_of(name):
    return CASES.get(name, dict(platform=1, env={}))


def params_for(lib, name, **fields):
    p = region.default_params(lib, platform=case_of(name)["platform"])
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def handle(lib, name, monkeypatch, link=None, **fields):
    """An accumulated handle for the case.  link: "eager", "lazy" or None (the oracle).  UVCGPU_LINK and UVCGPU_SPLIT are read on every accumulate."""
    reads = tile(name)
    for k, v in case_of(name)["env"].items():
        monkeypatch.setenv(k, v)
    accumulate(None, monkeypatch, link)
    R = region.Region(lib, params_for(lib, name, **fields), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    R.accumulate()
    return R


def accumulate(R, monkeypatch, link):
    if link == "eager":
        monkeypatch.setenv("UVCGPU_LINK", "eager")
    else:
        monkeypatch.delenv("UVCGPU_LINK", raising=False)
    if R is not None:
        R.accumulate()


def planes_of(R):
    return {g: R.fetch(g).copy() for g in INT_GROUPS}


@functools.lru_cache(maxsize=None)
def oracle_state(lib, name):
    """The oracle's answers for a case, computed once: default-gate and -A records, the 14 plane groups, the allele rows."""
    reads = tile(name)
    R = region.Region(lib, params_for(lib, name), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    R.accumulate()
    out = dict(default=R.score(all_out=False), all_out=R.score(all_out=True), planes=planes_of(R), alleles=R.indel_alleles())
    R.close()
    return out


def differing(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k])] + [k for k in b if k not in a]


def differing_planes(a, b):
    return {g: int((a[g] != b[g]).sum()) for g in a if not np.array_equal(a[g], b[g])}


ALL_CASES = list(CASES) + ["window_edges"]


def test_every_edge_indel_gives_a_default_gate_record(oracle_lib):
    """The hand-made tile is worth its name only if every one of its InDels is a default-gate record of the oracle, at the offsets meant."""
    reads, rec = edge_tile(), oracle_state(oracle_lib, "window_edges")["default"]
    off = rec["refpos"] - reads["beg"]
    got = {(int(o), "ins" if s >= 10 else "del") for o, s in zip(off, rec["symbol"]) if s in INDELS}
    print(sorted(got))
    want = {(a + 1, kind) for a in EDGE_ANCHORS for kind in ("ins", "del") if not (kind == "del" and a + 3 >= EDGE_LEN)}
    assert want <= got, sorted(want - got)
    assert {o for o, _ in want} == {6, 63, 64, EDGE_LEN - 10} and {o >> 6 for o, _ in want} == {0, 1, (EDGE_LEN - 10) >> 6}


@pytest.mark.parametrize("validator", ["on", "off"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_lazy_equals_eager_and_oracle(name, validator, oracle_lib, gpu_lib, monkeypatch):
    set_validator(monkeypatch, validator)
    want = oracle_state(oracle_lib, name)
    Rl, Re = handle(gpu_lib, name, monkeypatch, "lazy"), handle(gpu_lib, name, monkeypatch, "eager")
    try:
        # 1. default-gate records: nothing is called on the lazy handle between its accumulate and the score
        for kept_only in (False, True):
            a, b = Rl.score(all_out=False, kept_only=kept_only), Re.score(all_out=False, kept_only=kept_only)
            assert len(b["refpos"]) > 0
            assert not differing(a, b), (kept_only, differing(a, b))
            if not kept_only:
                compare_records(want["default"], a)
                exact = differing(want["default"], a)
                print(name, validator, "default-gate fields that differ from the oracle bit for bit:", exact)
        # 2. the planes and the allele rows behind that score: complete on the lazy handle too
        pl, pe = planes_of(Rl), planes_of(Re)
        assert not differing_planes(pe, pl), differing_planes(pe, pl)
        assert not differing_planes(want["planes"], pl), differing_planes(want["planes"], pl)
        assert Rl.indel_alleles() == Re.indel_alleles() == want["alleles"]
        # 3. -A behind a default-gate score of the same accumulate
        accumulate(Rl, monkeypatch, "lazy")
        assert not differing(Rl.score(all_out=False), Re.score(all_out=False))
        a, b = Rl.score(all_out=True), Re.score(all_out=True)
        assert not differing(a, b), differing(a, b)
        compare_records(want["all_out"], a)
    finally:
        Rl.close()
        Re.close()


@pytest.mark.parametrize("validator", ["on", "off"])
def test_rounds_release_and_reset(validator, oracle_lib, gpu_lib, monkeypatch):
    """Ten accumulate + score rounds, the planes handed back with every other score; then another region on the same handle and back."""
    set_validator(monkeypatch, validator)
    name, other = "paired_2kb_300x_indel_reads", "no_indel_reads_2kb_300x"
    Rl, Re, Ro = handle(gpu_lib, name, monkeypatch, "lazy"), handle(gpu_lib, name, monkeypatch, "eager"), handle(gpu_lib, other, monkeypatch, "eager")
    try:
        first, first_all, planes = Re.score(all_out=False), Re.score(all_out=True), planes_of(Re)
        for k in range(10):
            accumulate(Rl, monkeypatch, "lazy")
            rec = Rl.score(all_out=False, release_state=(k % 2 == 1))
            assert not differing(first, rec), (k, differing(first, rec))
        for nm, want_rec, want_all, want_pl in ((other, Ro.score(all_out=False), Ro.score(all_out=True), planes_of(Ro)), (name, first, first_all, planes)):
            reads = tile(nm)
            Rl.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
            Rl.set_reads(reads)
            accumulate(Rl, monkeypatch, "lazy")
            assert not differing(want_rec, Rl.score(all_out=False)), nm
            assert not differing(want_all, Rl.score(all_out=True)), nm
            assert not differing_planes(want_pl, planes_of(Rl)), (nm, differing_planes(want_pl, planes_of(Rl)))
    finally:
        for R in (Rl, Re, Ro):
            R.close()


@pytest.mark.parametrize("validator", ["on", "off"])
def test_tumor_keys_and_forced_sites_away_from_indels(validator, oracle_lib, gpu_lib, monkeypatch):
    """Gates that open LINK groups where the accumulate completed nothing: a normal pass keyed at SNV positions, and forced sites."""
    set_validator(monkeypatch, validator)
    name = "paired_2kb_300x_indel_reads"
    reads, rec = tile(name), oracle_state(oracle_lib, name)["default"]
    indel_windows = {int(p - reads["beg"]) >> 6 for p, s in zip(rec["refpos"], rec["symbol"]) if s in INDELS}
    snv = {k: v[(rec["symbol"] <= 5) & ~np.isin((rec["refpos"] - reads["beg"]) >> 6, sorted(indel_windows))] for k, v in rec.items()}
    keys = tumor_keys_from(snv)
    sites = [int(reads["beg"] + x) for x in range(130, reads["end"] - reads["beg"] - 130, 97) if (x >> 6) not in indel_windows]
    assert len(keys) >= 4 and len(sites) >= 8 and indel_windows
    out = {}
    for who, lib, link in (("oracle", oracle_lib, None), ("eager", gpu_lib, "eager"), ("lazy", gpu_lib, "lazy")):
        Rn = handle(lib, name, monkeypatch, link, tumor_vcf_is_provided=1)
        Rf = handle(lib, name, monkeypatch, link)
        if who == "lazy":
            Rf.score(all_out=False)   # a default-gate score first: the forced sites then complete what it left
        out[who] = (Rn.score(tumor_keys=keys), Rf.score(all_out=False, force_sites=sites))
        Rn.close()
        Rf.close()
    # (the oracle takes no forced sites: what they must give is its -A groups at the sites and its default-gate groups elsewhere)
    want = (out["oracle"][0], compose(rec, oracle_state(oracle_lib, name)["all_out"], sites))
    for i in range(2):
        assert len(out["lazy"][i]["refpos"]) > len(rec["refpos"]) * i
        assert not differing(out["eager"][i], out["lazy"][i]), (i, differing(out["eager"][i], out["lazy"][i]))
        compare_records(want[i], out["lazy"][i])


@pytest.mark.parametrize("validator", ["on", "off"])
def test_tile_without_indel_reads_runs_no_window(validator, oracle_lib, gpu_lib, monkeypatch, capfd):
    """No InDel mark, no window for the completion pass at the end of the accumulate; a later fetch still returns full planes of LINK_M."""
    set_validator(monkeypatch, validator)
    name = "no_indel_reads_2kb_300x"
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    capfd.readouterr()
    R = handle(gpu_lib, name, monkeypatch, "lazy")
    try:
        lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[uvcgpu link_complete]")]
        monkeypatch.delenv("UVCGPU_TIMING")
        assert len(lines) == 1 and " scope=indel done=0 of " in lines[0], lines
        assert len(R.score(all_out=False)["refpos"]) > 0
        want = oracle_state(oracle_lib, name)["planes"]
        seg = R.fetch("SEG32")
        assert np.array_equal(seg, want["SEG32"]) and (seg[:, 6, :] != 0).any(axis=1).sum() > 4   # LINK_M is symbol 6: more planes than the four aDP** hold something
        assert not differing_planes(want, planes_of(R))
    finally:
        R.close()
