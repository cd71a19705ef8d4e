"""Force-output sites on the device: a score call with UvcScoreRequest::force_sites (S) returns, group by group, the records of the all-out
call (B) at the selected (zerobased_pos, symbol type) groups and those of the default call (A) everywhere else -- every int32 field bit for
bit, on the same accumulated handle; the same composition made from the oracle's own default and all-out records holds S in the suite's
tolerance classes.  uvc1-mi355x --force-sites writes the default run's lines with the lines of the selected positions taken from the -A run."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cli_params import resolved
from test_gpu_parity import CASES, compare_records
from test_pipeline import make_files
from util import diff_groups, kept_groups, run_region
from uvc_amd import _ffi, io as uio, pipeline, region, synth

pytestmark = pytest.mark.gpu

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
PLANES = ["PREP32", "PREP64", "SEG32", "SEG64", "FRAG", "FAM", "FAMINFO32", "FAMINFO64", "DUPLEX", "VQ"]
INPUTS = {
    "synth_300x": (dict(CASES["config2shape_5kb_300x"], indel_every=300), 1),
    "umi_duplex_config4": (CASES["config4shape_1kb_2000x_duplex"], 1),
    "iontorrent": (dict(region_len=3000, depth=120, seed=21, indel_every=250), 2),
    "fuzz_weird": (None, 1),
}


def reads_of(name):
    kw, _ = INPUTS[name]
    if kw is None:                                                          # clipped, gapped, N-rich reads of every length (test_gpu_fuzz)
        from test_gpu_fuzz import weird_region
        return weird_region(5, n_frag=400)
    return synth.generate_region(**kw)


def zpos_of(rec):
    """zerobased_pos of every record: BASE records of refpos r belong to zerobased_pos r + 1, LINK records to r (both print VCF POS = it)"""
    return rec["refpos"].astype(np.int64) + (rec["symbol"] <= 5)


def compose(a, b, sites):
    """The records S must return: b's groups at the selected zerobased_pos values, a's elsewhere, in group order, germ_* re-based."""
    sel_a, sel_b = ~np.isin(zpos_of(a), sites), np.isin(zpos_of(b), sites)
    parts = [(a, np.nonzero(sel_a)[0]), (b, np.nonzero(sel_b)[0])]
    key = np.concatenate([2 * zpos_of(r)[i] + (r["symbol"][i] > 5) for r, i in parts])
    order = np.argsort(key, kind="stable")
    out = {}
    for f in a:
        v = np.concatenate([r[f][i] for r, i in parts])
        if f in ("germ_ref", "germ_alt1", "germ_alt2"):
            new = []
            for q, (r, i) in enumerate(parts):
                where = -np.ones(len(r["refpos"]), np.int64)
                where[i] = np.arange(len(i)) + sum(len(p[1]) for p in parts[:q])
                new.append(np.where(r[f][i] >= 0, where[np.maximum(r[f][i], 0)], -1))
            v = np.concatenate(new)
            inv = np.empty(len(order), np.int64)
            inv[order] = np.arange(len(order))
            v = np.where(v >= 0, inv[np.maximum(v, 0)], -1)
        out[f] = v[order]
    return out


def assert_same(s, want, what):
    assert len(s["refpos"]) == len(want["refpos"]), (what, len(s["refpos"]), len(want["refpos"]))
    bad = [f for f in want if not np.array_equal(s[f], want[f])]
    assert not bad, (what, bad[:6])


def pick_sites(rng, a, b, lo, hi, n=60):
    """Random positions of [lo, hi), positions where the all-out call has more records than the default one, and positions with a written
    record or a GERMLINE line at the default gate"""
    za, zb = zpos_of(a), zpos_of(b)
    extra = np.setdiff1d(np.unique(zb), np.unique(za[(a["keep"] == 1) | (a["germ_emit"] == 1)]))
    written = np.unique(za[(a["keep"] == 1) & (a["out"] == 1)])
    s = np.concatenate([rng.integers(lo, hi, n), rng.choice(extra, min(n, len(extra)), replace=False) if len(extra) else [],
                        rng.choice(written, min(n // 4, len(written)), replace=False) if len(written) else [], [lo, hi - 1]])
    s = s[(s >= lo) & (s < hi)]
    return np.unique(s.astype(np.int64))


@pytest.mark.parametrize("name", list(INPUTS))
def test_sites_equal_the_composition_of_default_and_all_out(name, gpu_lib):
    reads, platform = reads_of(name), INPUTS[name][1]
    R = run_region(gpu_lib, reads, platform=platform)
    rng = np.random.default_rng(len(name))
    lo, hi = reads["beg"] + 1, reads["end"] - 1
    a, b = R.score(), R.score(all_out=True)
    planes = {g: R.fetch(g).copy() for g in PLANES}
    sites = pick_sites(rng, a, b, lo, hi)
    assert len(sites) > 20 and len(a["refpos"]) > 0
    s = R.score(force_sites=sites)
    want = compose(a, b, sites)
    assert_same(s, want, "plain")
    assert len(s["refpos"]) > len(a["refpos"]) and (s["keep"] & s["out"]).sum() >= (a["keep"] & a["out"]).sum()
    # every other group is the default call's, even next to a site
    far = ~np.isin(zpos_of(s), sites)
    assert np.array_equal(np.unique(zpos_of(s)[far]), np.unique(zpos_of(a)[~np.isin(zpos_of(a), sites)]))
    # no sites = the default call; sites outside the range select nothing; -A with sites = -A
    assert_same(R.score(force_sites=[]), a, "empty list")
    assert_same(R.score(force_sites=[lo - 5, hi + 10, hi + 1000]), a, "outside")
    assert_same(R.score(all_out=True, force_sites=sites), b, "all_out")
    # kept_only: the groups the writer reads, of the same composition
    ka, kb = R.score(kept_only=True), R.score(all_out=True, kept_only=True)
    ks = R.score(kept_only=True, force_sites=sites)
    assert_same(ks, compose(ka, kb, sites), "kept_only")
    assert_same(ks, kept_groups(s)[1], "kept_only of S")
    # the record text: the default text with the selected positions' lines from the all-out text
    ta, tb, ts = (R.vcf_records("chrF", r).splitlines() for r in (a, b, s))
    pos = lambda l: int(l.split("\t")[1])                                   # noqa: E731
    want_text = sorted([l for l in ta if pos(l) not in set(sites.tolist())] + [l for l in tb if pos(l) in set(sites.tolist())], key=pos)
    assert ts == want_text
    # the planes: scoring with sites does not touch them
    assert all(np.array_equal(R.fetch(g), planes[g]) for g in PLANES)
    # release_state: the same records while the planes are zeroed behind the kernels
    s2 = R.score(force_sites=sites, release_state=True)
    assert_same(s2, want, "release_state")
    R.accumulate()
    assert all(np.array_equal(R.fetch(g), planes[g]) for g in PLANES)
    assert_same(R.score(force_sites=sites), want, "after re-accumulate")
    R.close()


def test_adjacent_tiles_with_base_at_pos_beg(gpu_lib):
    """Two score ranges [b0, b1) and [b1, b2) of one handle, the second with base_at_pos_beg: each composes on its own range, sites on both
    sides of the cut and on it."""
    reads = synth.generate_region(**dict(CASES["config2shape_5kb_300x"], indel_every=300))
    R = run_region(gpu_lib, reads)
    b0, b1, b2 = reads["beg"] + 200, reads["beg"] + 2500, reads["beg"] + 4800
    rng = np.random.default_rng(4)
    for pb, pe, bab in ((b0, b1, False), (b1, b2, True)):
        kw = dict(pos_beg=pb, pos_end=pe, base_at_pos_beg=bab)
        a, b = R.score(**kw), R.score(all_out=True, **kw)
        sites = np.unique(np.concatenate([pick_sites(rng, a, b, pb, pe, 40), [b1 - 1, b1, b1 + 1, b0 - 3, b2 + 3]]))
        want = compose(a, b, sites[(sites >= pb) & (sites < pe)])
        assert_same(R.score(force_sites=sites, **kw), want, (pb, pe))
        assert_same(R.score(force_sites=sites, kept_only=True, **kw), compose(R.score(kept_only=True, **kw), R.score(all_out=True, kept_only=True, **kw), sites), ("kept", pb, pe))
    R.close()


@pytest.mark.parametrize("name", list(INPUTS))
def test_sites_against_the_oracle_composition(name, oracle_lib, gpu_lib):
    reads, platform = reads_of(name), INPUTS[name][1]
    Ro, Rg = run_region(oracle_lib, reads, platform=platform), run_region(gpu_lib, reads, platform=platform)
    bad = diff_groups(Ro, Rg, PLANES)
    assert not bad, bad
    ao, bo = Ro.score(), Ro.score(all_out=True)
    sites = pick_sites(np.random.default_rng(7), ao, bo, reads["beg"] + 1, reads["end"] - 1)
    s = Rg.score(force_sites=sites)
    compare_records(compose(ao, bo, sites), s)
    assert not diff_groups(Ro, Rg, PLANES)                                  # planes fetched after S still equal the oracle's


# ---- the command line ----
TILE = 2000


def cli(args, timeout=300):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r


def body(path):
    """the lines of a VCF without the ## header lines (they hold the command line and the date)"""
    return [l for l in gzip.open(path, "rt").read().splitlines() if not l.startswith("##")]


def composed_text(default, allout, sites):
    pos = lambda l: int(l.split("\t")[1])                                   # noqa: E731
    head = [l for l in default if l.startswith("#")]
    assert head == [l for l in allout if l.startswith("#")]
    recs = [l for l in default if not l.startswith("#") and pos(l) not in sites] + [l for l in allout if not l.startswith("#") and pos(l) in sites]
    return head + sorted(recs, key=pos)


@pytest.fixture(scope="module")
def run_files(tmp_path_factory, gpu_lib):
    d = tmp_path_factory.mktemp("forcesites")
    reads = make_files(d, 1)
    bam, fa = str(d / "u1.bam"), str(d / "u1.fa")
    b0, b1 = reads["beg"], reads["beg"] + 6000
    common = [bam, "-f", fa, "-s", "S1", "--targets", "chrT:%d-%d" % (b0 + 1, b1), "--tile", TILE]
    default, allout = str(d / "a.vcf.gz"), str(d / "b.vcf.gz")
    cli(common + ["-o", default, "-t", "2"])
    cli(common + ["-o", allout, "-t", "2", "-A"])
    A, B = body(default), body(allout)
    rng = np.random.default_rng(11)
    pos = lambda l: int(l.split("\t")[1])                                   # noqa: E731
    a_pos, b_pos = {pos(l) for l in A if l[0] != "#"}, {pos(l) for l in B if l[0] != "#"}
    extra = sorted(b_pos - a_pos)
    borders = [b0 + k * TILE + o for k in range(1, 3) for o in (-1, 0, 1)]
    sites = sorted(set(rng.integers(b0 + 1, b1, 150).tolist()) | set(rng.choice(extra, 100, replace=False).tolist()) | set(borders) | set(sorted(a_pos)[::7]))
    assert len(sites) > 200
    bed = d / "s.bed"
    bed.write_text("".join("chrT\t%d\t%d\n" % (x - 1, x) for x in sites[::-1]))     # base x - 1 = VCF POS x
    vcf = d / "s.vcf"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join("chrT\t%d\t.\tN\t.\t.\t.\t.\n" % x for x in sites))
    return dict(d=d, common=common, A=A, B=B, sites=set(sites), bed=str(bed), vcf=str(vcf), bam=bam, fa=fa, b0=b0, b1=b1)


def test_cli_sites_are_the_default_run_with_all_out_lines_at_the_sites(run_files):
    f = run_files
    assert len(f["B"]) > 2 * len(f["A"])
    want = composed_text(f["A"], f["B"], f["sites"])
    assert want != f["A"]
    for extra, tag in ((["-t", "1", "--force-sites", f["bed"]], "bed1"), (["-t", "4", "--force-sites", f["bed"]], "bed4"),
                       (["-t", "2", "--force-sites=" + f["vcf"]], "vcf")):
        out = str(f["d"] / (tag + ".vcf.gz"))
        r = cli(f["common"] + ["-o", out] + extra)
        assert "force-output sites" in r.stderr
        assert body(out) == want, tag
    # with -A it changes nothing
    out = str(f["d"] / "ab.vcf.gz")
    cli(f["common"] + ["-o", out, "-A", "--force-sites", f["bed"]])
    assert body(out) == f["B"]


def test_cli_two_shards_joined_equal_one_process(run_files):
    f = run_files
    outs = []
    for i in range(2):
        out = str(f["d"] / ("sh%d.vcf.gz" % i))
        cli(f["common"] + ["-o", out, "--shard", "%d/2" % i, "--force-sites", f["vcf"]])
        outs.append(out)
    joined = str(f["d"] / "joined.vcf.gz")
    cli(["--concat", joined] + outs)
    assert body(joined) == composed_text(f["A"], f["B"], f["sites"])


def test_python_call_region_writes_the_command_line_text(run_files, gpu_lib):
    f = run_files
    p, g = resolved(f["bam"], ["--targets", "chrT:%d-%d" % (f["b0"] + 1, f["b1"]), "--tile", TILE])
    kw = dict(sample="S1", tile=TILE, params=p, group_params=g, molecule_tag=g.molecule_tag, disable_duplex=g.disable_duplex)
    want = composed_text(f["A"], f["B"], f["sites"])
    for tag, fs in (("obj", uio.Sites(f["bed"], ["chrT"])), ("list", sorted(f["sites"]))):
        out = str(f["d"] / ("py_%s.vcf.gz" % tag))
        pipeline.write_vcf(region.gpu_lib(), f["bam"], f["fa"], "chrT", f["b0"], f["b1"], out, force_sites=fs, **kw)
        assert body(out) == want, tag
