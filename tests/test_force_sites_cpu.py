"""Force-output sites without a device: --force-sites is a CLI option, its refusals come before any file or device is opened, the site
reader (uvcio_sites_*) takes BED and VCF(.gz), maps contigs through the BAM header, sorts and de-duplicates, and refuses unknown contigs
and malformed lines by line number; the per-tile fetch hands every site to exactly one tile of a run of fixed tiles."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from uvc_amd import _ffi, io as uio, pipeline

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
CONTIGS = ["chr1", "chr2", "chrM"]


def run(args, timeout=60):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def sites(path, contigs=CONTIGS):
    s = uio.Sites(str(path), contigs)
    return {name: s.fetch(tid).tolist() for tid, name in enumerate(contigs)}, s.n_sites


def test_help_lists_the_option_as_cli():
    r = run(["--help"])
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("  --force-sites ")]
    assert len(line) == 1 and line[0].split()[1] == "[CLI]", line


@pytest.mark.parametrize("args,what", [
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--force-sites", "s.bed", "--tumor-vcf", "t.vcf.gz"], "--tumor-vcf"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--tumor-vcf=t.vcf.gz", "--force-sites=s.bed"], "--tumor-vcf"),
    (["/only-print-vcf-header/", "--force-sites", "s.bed"], "/only-print-vcf-header/"),
    (["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz", "--force-sites", "s.bed"], "--normal-bam"),
    (["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz", "--force-sites", ""], "needs a path"),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, what):
    """None of the files exists and the machine may have no device: the refusal has to be the first thing that happens."""
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--force-sites" in r.stderr and what in r.stderr, r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "o.vcf.gz") and not os.path.exists(tmp_path / "n.vcf.gz")


def test_bed_every_base_is_a_site_sorted_and_unique(tmp_path):
    p = tmp_path / "s.bed"
    p.write_text("track name=x\n# comment\nbrowser position chr1\nchr2\t100\t103\tname\t0\t+\n"
                 "chr1 10 12\nchr1\t11\t13\n\nchrM\t0\t1\r\nchr2\t50\t50\nchr1\t5\t6\n")
    got, n = sites(p)
    # base x (0-based) -> the records of VCF POS x + 1 = zerobased_pos x + 1
    assert got == {"chr1": [6, 11, 12, 13], "chr2": [101, 102, 103], "chrM": [1]}
    assert n == 8


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_vcf_chrom_and_pos_only(tmp_path, kind):
    text = ("##fileformat=VCFv4.2\n##contig=<ID=chr1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
            "chr2\t500\t.\tA\tG\t.\t.\t.\nchr1\t20\trs1\tAC\tA\t30\tPASS\tX=1\nchr1\t7\t.\tG\t<NON_REF>\t.\t.\t.\nchr2\t500\t.\tA\tT\t.\t.\t.\n"
            "chr1\t20\t.\tA\tAT\t.\t.\t.\n")
    if kind == "plain":
        p = tmp_path / "s.vcf"
        p.write_text(text)
    elif kind == "gzip":
        p = tmp_path / "s.vcf.gz"
        with gzip.open(p, "wt") as f:
            f.write(text)
    else:
        p = tmp_path / "s.bgzf.vcf.gz"
        w = uio.BgzfWriter(str(p))
        w.write(text)
        w.close()
    got, n = sites(p)
    assert got == {"chr1": [7, 20], "chr2": [500], "chrM": []} and n == 3


def test_a_vcf_without_meta_lines_is_a_vcf(tmp_path):
    p = tmp_path / "s.txt"
    p.write_text("#CHROM\tPOS\tID\tREF\tALT\nchr1\t3\t.\tA\tC\n")
    assert sites(p)[0]["chr1"] == [3]


@pytest.mark.parametrize("name,text,where", [
    ("a.bed", "chr1\t1\t5\nchrX\t1\t2\n", "line 2"),
    ("b.bed", "chr1\t1\n", "line 1"),
    ("c.bed", "chr1\t1\t5\n\nchr1\t9\t3\n", "line 3"),
    ("d.bed", "chr1\t-1\t5\n", "line 1"),
    ("e.bed", "chr1\tx\t5\n", "line 1"),
    ("f.vcf", "##fileformat=VCFv4.2\n#CHROM\tPOS\nchr1\t0\n", "line 3"),
    ("g.vcf", "##fileformat=VCFv4.2\nchr1\t5\nchr9\t5\n", "line 3"),
    ("h.vcf", "##fileformat=VCFv4.2\nchr1\n", "line 2"),
    ("i.vcf", "##fileformat=VCFv4.2\nchr1\t12a\n", "line 2"),
])
def test_bad_lines_are_refused_by_line(tmp_path, name, text, where):
    p = tmp_path / name
    p.write_text(text)
    with pytest.raises(IOError) as e:
        uio.Sites(str(p), CONTIGS)
    assert where in str(e.value) and name in str(e.value), str(e.value)


def test_missing_file_is_refused(tmp_path):
    with pytest.raises(IOError):
        uio.Sites(str(tmp_path / "nope.bed"), CONTIGS)


def test_per_tile_split_gives_every_site_to_one_tile(tmp_path):
    """The fixed tiles of a run own [beg, end) each (zerobased_pos `end` belongs to the next tile): fetching each tile's range hands out
    every site of the run exactly once, whatever the tile size."""
    rng = np.random.default_rng(3)
    beg, end = 1000, 25000
    pos = np.concatenate([rng.integers(beg, end, 400), np.arange(beg, end, 1000), np.arange(beg, end, 1000) - 1, np.arange(beg, end, 1000) + 1])
    pos = pos[(pos >= beg) & (pos < end)]
    p = tmp_path / "s.vcf"
    p.write_text("##fileformat=VCFv4.2\n" + "".join("chr2\t%d\n" % x for x in rng.permutation(pos)))
    s = uio.Sites(str(p), CONTIGS)
    want = np.unique(pos)
    assert s.n_sites == len(want) and np.array_equal(s.fetch(1), want)
    for tile in (1000, 1777, 5000, 30000):
        tiles = pipeline.contig_tiles(beg, end, tile)
        parts = [s.fetch(1, t["beg"], t["end"]) for t in tiles]
        got = np.concatenate(parts)
        assert np.array_equal(got, want), tile
        assert all(((q >= t["beg"]) & (q < t["end"])).all() for q, t in zip(parts, tiles))
    assert len(s.fetch(0)) == 0 and len(s.fetch(7)) == 0 and len(s.fetch(1, 5000, 5000)) == 0


def test_request_fields_trail_the_struct():
    """The ctypes mirror ends in the two new fields, after every field the struct had before (the C ABI appends them)."""
    names = [f[0] for f in _ffi.UvcScoreRequest._fields_]
    assert names[-2:] == ["n_force_sites", "force_sites"] and names.index("tumor_ref_alt") == len(names) - 3
    assert _ffi.UvcScoreRequest.n_force_sites.offset % 8 == 0 and C.sizeof(_ffi.UvcScoreRequest) == _ffi.UvcScoreRequest.force_sites.offset + 8


def test_request_sorts_and_dedups_sites():
    from uvc_amd import region
    req, keep = region.Region.make_request(force_sites=[30, 10, 20, 10])
    assert req.n_force_sites == 3 and list(keep[-1]) == [10, 20, 30] and req.force_sites == keep[-1].ctypes.data
    req, keep = region.Region.make_request()
    assert req.n_force_sites == 0 and not req.force_sites
