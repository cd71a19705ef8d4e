"""uvc1-mi355x with parameters off their defaults writes what the Python chain (uvc_amd/pipeline.py) writes with the same parameters, and
something else than its default run: every option below reaches the device.  The parameters of the Python side are the ones the command
line resolved (--print-params), so the comparison covers the path from the option to the kernels, not the resolution itself
(tests/test_cli_params_cpu.py checks that)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from param_moves import MOVES
import bamwriter
from test_pipeline import make_files, make_tn_files
from uvc_amd import _ffi, group, io as uio, pipeline, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
TILE = 2000


def cli(args, timeout=300):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r.stdout


def resolved(bam, args):
    """(UvcParams, UvcGroupParams) as the command line resolves `args` for `bam`"""
    p = _ffi.UvcParams()
    region.gpu_lib().call("params_default", C.byref(p))
    g = group.default_params(region.gpu_lib(), 0, 1)
    rows = {r["name"]: r for r in region.param_table()}
    for line in cli([bam, "--print-params"] + args).splitlines():
        name, v = line.split("=", 1)
        setattr(p if rows[name]["owner"] == "params" else g, name, int(v) if rows[name]["kind"] == "int" else float(v))
    g.inferred_sequencing_platform = p.inferred_sequencing_platform
    return p, g


def body(path):
    return [l for l in gzip.open(path, "rt").read().splitlines() if not l.startswith("##")]


def make_amplicon_files(d, n_amp=8, pairs=150, ins=280, beg=30000, L=150):
    """A BAM the family pass takes for an amplicon assay: every fragment of an amplicon has the same two ends; an SNV in a third of them.
    Returns the span [beg, end) that holds the amplicons."""
    rng = np.random.default_rng(17)
    chrom_len = beg + n_amp * 400 + 5000
    ref = rng.integers(0, 4, chrom_len).astype(np.uint8)
    recs = []
    for a in range(n_amp):
        s = beg + 400 * a
        snv = s + 140
        for k in range(pairs):
            for mate in (0, 1):
                pos = s if mate == 0 else s + ins - L
                b = ref[pos:pos + L].copy()
                alt = (k % 3 == 0 and pos <= snv < pos + L)
                if alt:
                    b[snv - pos] = (ref[snv] + 1) % 4
                recs.append(dict(tid=0, pos=pos, qname="a%d_%d" % (a, k), flag=1 | 2 | (0x40 | 0x20 if mate == 0 else 0x80 | 0x10), mapq=60, cigar=[(0, L)],
                                 bases=b, quals=np.full(L, 35, np.uint8), mtid=0, mpos=(s + ins - L if mate == 0 else s), tlen=(ins if mate == 0 else -ins), nm=int(alt)))
    recs.sort(key=lambda r: r["pos"])
    bamwriter.write_bam(str(d / "amp.bam"), [("chrA", chrom_len)], recs)
    bamwriter.write_fasta(str(d / "amp.fa"), [("chrA", "".join("ACGT"[i] for i in ref))])
    return beg - 100, beg + n_amp * 400 + 100


class Files:
    def __init__(self, d, umi, amplicon=False):
        if amplicon:
            beg, end = make_amplicon_files(d)
            self.bam, self.fa, self.chrom = str(d / "amp.bam"), str(d / "amp.fa"), "chrA"
        else:
            beg = make_files(d, umi)["beg"]
            end = beg + 6000
            self.bam, self.fa, self.chrom = str(d / ("u%d.bam" % umi)), str(d / ("u%d.fa" % umi)), "chrT"
        self.d, self.b0, self.b1 = d, beg, end
        self.n = 0

    def target(self):
        return "%s:%d-%d" % (self.chrom, self.b0 + 1, self.b1)

    def cli_body(self, args):
        self.n += 1
        out = str(self.d / ("c%d.vcf.gz" % self.n))
        cli([self.bam, "-f", self.fa, "-o", out, "-s", "S1", "--targets", self.target(), "--tile", TILE, "-t", "2"] + args)
        return body(out)

    def py_body(self, args, assay_type=0):
        p, g = resolved(self.bam, ["--targets", self.target(), "--tile", TILE] + args)
        self.n += 1
        out = str(self.d / ("p%d.vcf.gz" % self.n))
        pipeline.write_vcf(region.gpu_lib(), self.bam, self.fa, self.chrom, self.b0, self.b1, out, sample="S1", tile=TILE, params=p, group_params=g,
                           molecule_tag=g.molecule_tag, disable_duplex=g.disable_duplex, all_out=bool(p.should_output_all), assay_type=assay_type)
        return body(out)


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_lib):
    d = tmp_path_factory.mktemp("cliparams")
    f = {umi: Files(d, umi) for umi in (0, 1)}
    default = {umi: f[umi].cli_body([]) for umi in (0, 1)}
    for umi in (0, 1):
        assert default[umi] == f[umi].py_body([]) and len(default[umi]) > 20
    return f, default


def arg(v):
    return repr(v) if isinstance(v, float) else str(v)


# one move of each output class of the ledger (tests/param_moves.py), on the input of that move
CLASS_MOVES = [
    ("planes", 0, "fam_thres_highBQ_snv"),
    ("gate", 0, "min_altdp_thres"),
    ("records", 0, "vqual"),
    ("families", 0, "group.kept_aln_max_isize"),
    ("alleles", 1, "fam_thres_dup1add"),
    ("hap", 0, "phasing_haplotype_max_count"),
    ("vcf", 0, "microadjust_alignment_tracklen_min"),
]


def move_args(key, umi):
    if key == "group.kept_aln_max_isize":   # the ledger's move (2^32 + 1) is not an int32: half of the fragments of the synthetic file instead
        return ["--kept-aln-max-isize", "350"]
    m = next(m for m in MOVES[key] if m.input == ("duplex" if umi else "plain"))
    out = []
    for c, v in m.companions.items():
        out += ["--" + c.replace("_", "-"), arg(v)]
    return out + ["--" + key.replace("group.", "").replace("_", "-"), arg(m.value)]


@pytest.mark.gpu
@pytest.mark.parametrize("cls,umi,key", CLASS_MOVES, ids=[c[0] for c in CLASS_MOVES])
def test_a_ledger_move_of_each_output_class(files, cls, umi, key):
    f, default = files
    args = move_args(key, umi)
    got = f[umi].cli_body(args)
    assert got == f[umi].py_body(args)
    assert got != default[umi], args


@pytest.mark.gpu
@pytest.mark.parametrize("umi,args", [(1, ["--molecule-tag", "1"]), (1, ["--disable-duplex", "1"]), (0, ["--all-germline-out", "--outvar-flag", "63"]),
                                      (0, ["--sequencing-platform", "2"])],
                         ids=["molecule-tag", "disable-duplex", "all-germline-out", "sequencing-platform"])
def test_mode_switches(files, umi, args):
    f, default = files
    got = f[umi].cli_body(args)
    assert got == f[umi].py_body(args)
    assert got != default[umi], args


@pytest.mark.gpu
def test_assay_type(files, tmp_path):
    """--assay-type overrides the per-region inference (main.cpp:510-511), which takes the synthetic files for captures and the amplicon file
    for an amplicon assay.  On Illumina the platform step makes the PCR and the capture minimum ABQ equal (CmdLineArgs.cpp:125-130); a higher
    value on the side the override chooses makes it visible (main.cpp:526-527): AMPLICON on the captures, CAPTURE on the amplicons."""
    f, _ = files
    pcr = ["--syserr-minABQ-pcr-snv", "400", "--syserr-minABQ-pcr-indel", "400"]
    for umi in (0, 1):
        inferred = f[umi].cli_body(pcr)
        for assay in (1, 2):
            got = f[umi].cli_body(pcr + ["--assay-type", assay])
            assert got == f[umi].py_body(pcr, assay_type=assay)
            assert (got != inferred) if assay == 2 else (got == inferred)
    amp = Files(tmp_path, 0, amplicon=True)
    cap = ["--syserr-minABQ-cap-snv", "400", "--syserr-minABQ-cap-indel", "400"]
    inferred = amp.cli_body(cap)
    assert len([l for l in inferred if not l.startswith("#")]) > 5
    for assay in (1, 2):
        got = amp.cli_body(cap + ["--assay-type", assay])
        assert got == amp.py_body(cap, assay_type=assay)
        assert (got != inferred) if assay == 1 else (got == inferred)


@pytest.mark.gpu
def test_fifteen_ledger_moves_at_once(files):
    f, default = files
    rows = {r["name"]: r for r in region.param_table()}
    cand = sorted((k, i) for k, ms in MOVES.items() for i, m in enumerate(ms)
                  if m.input == "plain" and k in rows and rows[k]["settable"] and k not in ("should_output_all", "vqual")
                  and all(c in rows and rows[c]["settable"] for c in m.companions))
    rng = np.random.default_rng(2024)
    pick = [cand[j] for j in sorted(rng.choice(len(cand), size=15, replace=False))]
    setting = {}
    for k, i in pick:
        for c, v in MOVES[k][i].companions.items():
            setting.setdefault(c, v)
    for k, i in pick:
        setting[k] = MOVES[k][i].value
    args = []
    for k, v in setting.items():
        args += ["--" + k.replace("_", "-"), arg(v)]
    got = f[0].cli_body(args)
    assert got == f[0].py_body(args)
    assert got != default[0], args


@pytest.mark.gpu
def test_normal_pass_with_a_moved_normal_side_parameter(tmp_path, gpu_lib):
    """bin/uvcTN.sh: the tumor pass, then the normal pass with --tumor-vcf and the normal side's parameters forwarded"""
    rd = make_tn_files(tmp_path)
    tb, nb, fa = str(tmp_path / "tumor.bam"), str(tmp_path / "normal.bam"), str(tmp_path / "tn.fa")
    b0 = rd["tumor"]["beg"]
    target = "chrT:%d-%d" % (b0 + 1, b0 + 5000)
    tv = str(tmp_path / "T.vcf.gz")
    tumor_params = ["--tn-is-paired", "1", "--fam-thres-highBQ-snv", "27"]
    cli([tb, "-f", fa, "-o", tv, "-s", "TUM", "--targets", target, "--tile", TILE, "-t", "2"] + tumor_params)
    bodies = {}
    for name, moved in (("default", []), ("moved", ["--tn-syserr-norm-devqual", "-1.0", "--bias-thres-aLRI1NT-perc", "100"])):
        args = ["--tn-is-paired", "1", "--tumor-vcf", tv] + moved
        nv = str(tmp_path / ("N_%s.vcf.gz" % name))
        cli([nb, "-f", fa, "-o", nv, "-s", "NOR", "--targets", target, "--tile", TILE, "-t", "2"] + args)
        bodies[name] = body(nv)
        p, g = resolved(nb, ["--targets", target, "--tile", TILE] + args)
        assert p.tumor_vcf_is_provided == 1 and p.tn_is_paired == 1
        T = uio.TumorVcf(tv, ["chrT"])
        py = str(tmp_path / ("P_%s.vcf.gz" % name))
        pipeline.write_vcf(gpu_lib, nb, fa, "chrT", b0, b0 + 5000, py, sample="NOR", tile=TILE, params=p, group_params=g, tumor_vcf=T)
        T.close()
        assert bodies[name] == body(py), name
    assert bodies["moved"] != bodies["default"]
