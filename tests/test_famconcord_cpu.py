"""The family concordance report without a device: the restatement of the contract (tests/famconcord_restatement.py) against rows computed by
hand for constructed families, the row's section table against include/uvc_famconcord.def, the text of the store (uvcio_famconcord_*,
uvc_amd.io.FamilyConcordance) for a given row, and the command line's option: listed, refused in pair mode and with --shard / --repeat,
and probed before a device is opened."""
import collections
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bamwriter
import famconcord_restatement as fr
from famconcord_cases import Builder, I, M
from uvc_amd import _ffi, io as uio, region, synth

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
E = _ffi.ENUMS
LINK_M, LINK_I1 = 6, 12
S, L = 10, 10          # every read of the hand-computed cases: 10 reference bases at region offset 10 (unless the case says otherwise)


def restated(b, oracle_lib, ranges=None, platform=1):
    reads = b.reads()
    P = region.default_params(oracle_lib, platform=platform)
    return fr.restate(reads, P, platform, [ranges or [(reads["beg"], reads["end"] + 1)]])[0]


def check(row, want):
    got = {int(i): int(row[i]) for i in np.flatnonzero(row)}
    want = {k: v for k, v in want.items() if v}
    assert got == want, (sorted(set(got.items()) - set(want.items())), sorted(set(want.items()) - set(got.items())))


def plain_unit(W, ref, s, n, k, skip=()):
    """What a unit of n fragments, each one 10-base read at offset s that agrees with the reference, adds (depth bin k): its span is
    [s, s + 10 + n), bases vote at the 10 read positions, LINK_M from the second on.  skip: read offsets the caller tallies itself."""
    W[fr.C["units_seen"]] += 1; W[fr.C["unit_positions"]] += L + n
    W[fr.C["base_no_vote"]] += n; W[fr.C["link_no_vote"]] += n + 1
    for i in range(L):
        if i in skip:
            continue
        r = int(ref[s + i])
        W[fr.base_cell(0, k, r, r)] += n; W[fr.base_pos_cell(0, k, 0)] += 1; W[fr.base_pos_cell(0, k, 1)] += 1
    W[fr.link_cell(k, LINK_M, LINK_M)] += n * (L - 1); W[fr.link_pos_cell(k, 0)] += L - 1; W[fr.link_pos_cell(k, 1)] += L - 1


def test_three_fragments_with_one_dissenting_base(oracle_lib):
    b = Builder(60, 1); b.family(0x1)
    b.read(S, [(M, L)]); b.read(S, [(M, L)]); b.read(S, [(M, L)], subst={4: 1})
    W = collections.Counter()
    plain_unit(W, b.ref, S, 3, 2, skip=(4,))
    r4 = int(b.ref[S + 4])
    W[fr.base_cell(0, 2, r4, r4)] += 2; W[fr.base_cell(0, 2, r4, (r4 + 1) % 4)] += 1; W[fr.base_pos_cell(0, 2, 0)] += 1
    check(restated(b, oracle_lib), W)


def test_a_two_to_two_tie_goes_to_the_smaller_symbol(oracle_lib):
    b = Builder(60, 2); b.family(0x1)
    for k in range(4):
        b.read(S, [(M, L)], subst=({4: 1} if k >= 2 else {}))
    W = collections.Counter()
    plain_unit(W, b.ref, S, 4, 3, skip=(4,))
    r4 = int(b.ref[S + 4]); alt = (r4 + 1) % 4; cs = min(r4, alt); rc = 0 if cs == r4 else 1
    W[fr.base_cell(rc, 3, cs, r4)] += 2; W[fr.base_cell(rc, 3, cs, alt)] += 2; W[fr.base_pos_cell(rc, 3, 0)] += 1
    check(restated(b, oracle_lib), W)


def test_a_quality_zero_base_casts_no_vote(oracle_lib):
    b = Builder(60, 3); b.family(0x1)
    b.read(S, [(M, L)]); b.read(S, [(M, L)]); b.read(S, [(M, L)], quals={4: 0})
    W = collections.Counter()
    plain_unit(W, b.ref, S, 3, 2, skip=(4,))
    r4 = int(b.ref[S + 4])
    W[fr.base_cell(0, 1, r4, r4)] += 2; W[fr.base_pos_cell(0, 1, 0)] += 1; W[fr.base_pos_cell(0, 1, 1)] += 1      # two votes: the bin of 2
    check(restated(b, oracle_lib), W)


def test_an_insertion_in_one_of_four_fragments(oracle_lib):
    b = Builder(60, 4); b.family(0x1)
    for k in range(3):
        b.read(S, [(M, L)])
    b.read(S, [(M, 5), (I, 1), (M, 5)], nm=1)
    W = collections.Counter()
    plain_unit(W, b.ref, S, 4, 3)
    # at read offset 5 the InDel read carries LINK_I1 and no LINK_M (its second M run begins there): 3 : 1, not unanimous
    W[fr.link_cell(3, LINK_M, LINK_M)] -= 1; W[fr.link_cell(3, LINK_M, LINK_I1)] += 1; W[fr.link_pos_cell(3, 1)] -= 1
    check(restated(b, oracle_lib), W)


def test_a_duplex_pair_that_agrees(oracle_lib):
    b = Builder(60, 5); b.family(0x3)
    for st in (0, 0, 1, 1):
        b.read(S, [(M, L)], strand=st)
    W = collections.Counter()
    plain_unit(W, b.ref, S, 2, 1); plain_unit(W, b.ref, S, 2, 1)
    for i in range(L):
        r = int(b.ref[S + i]); W[fr.dup_base_cell(r, r, r)] += 1
    W[fr.dup_link_cell(0, 0)] += L - 1
    W[fr.C["duplex_no_vote"]] += 2 + 3         # the family's span is [S, S + 12): BASE has no vote on the last two, LINK on the first as well
    check(restated(b, oracle_lib), W)


def test_a_duplex_pair_that_disagrees_c_to_t(oracle_lib):
    b = Builder(60, 6, ref_at={S + 4: 1}); b.family(0x3)
    b.read(S, [(M, L)], strand=0); b.read(S, [(M, L)], strand=1, subst={4: 2})
    W = collections.Counter()
    plain_unit(W, b.ref, S, 1, 0); plain_unit(W, b.ref, S, 1, 0, skip=(4,))
    W[fr.base_cell(1, 0, 3, 3)] += 1; W[fr.base_pos_cell(1, 0, 0)] += 1; W[fr.base_pos_cell(1, 0, 1)] += 1         # the strand-1 unit: consensus T on a C
    for i in range(L):
        r = int(b.ref[S + i]); W[fr.dup_base_cell(r, r, 3 if i == 4 else r)] += 1
    assert W[fr.dup_base_cell(1, 1, 3)] == 1
    W[fr.dup_link_cell(0, 0)] += L - 1
    W[fr.C["duplex_no_vote"]] += 1 + 2
    check(restated(b, oracle_lib), W)


def test_duplex_strands_that_overlap_only_partly(oracle_lib):
    b = Builder(60, 7); b.family(0x3)
    b.read(S, [(M, L)], strand=0); b.read(S + 6, [(M, L)], strand=1)
    W = collections.Counter()
    plain_unit(W, b.ref, S, 1, 0); plain_unit(W, b.ref, S + 6, 1, 0)
    NB, NL = fr.NBASE, fr.NLINK
    for j in range(17):                        # the family's span [S, S + 17)
        r = int(b.ref[S + j])
        v0, v1 = (r if j <= 9 else NB), (r if 6 <= j <= 15 else NB)
        if (v0, v1) == (NB, NB): W[fr.C["duplex_no_vote"]] += 1
        else: W[fr.dup_base_cell(r, v0, v1)] += 1
        l0, l1 = (0 if 1 <= j <= 9 else NL), (0 if 7 <= j <= 15 else NL)
        if (l0, l1) == (NL, NL): W[fr.C["duplex_no_vote"]] += 1
        else: W[fr.dup_link_cell(l0, l1)] += 1
    assert W[fr.C["duplex_no_vote"]] == 3
    row = restated(b, oracle_lib)
    check(row, W)
    # rows of disjoint position sets add, and a range list picks its positions
    reads = b.reads()
    cut = reads["beg"] + S + 8
    P = region.default_params(oracle_lib)
    a, c, one = fr.restate(reads, P, 1, [[(reads["beg"], cut)], [(cut, reads["end"] + 1)], [(cut, cut + 1)]])
    assert np.array_equal(a + c, row) and one[fr.C["unit_positions"]] == 2 and one[fr.C["units_seen"]] == 0 and a[fr.C["units_seen"]] == 2


def test_the_row_is_the_table_of_the_def_file_everywhere():
    assert _ffi.FAMCONC_SECTIONS == fr.SECTIONS and region.FAMILY_CONCORDANCE == [n for n, _, _ in fr.SECTIONS]
    assert E["UVC_FAMCONC_ROW"] == fr.ROW == 1429 and E["UVC_FAMCONC_NBIN"] == fr.NBIN and E["UVC_FAMCONC_NBASE"] == fr.NBASE and E["UVC_FAMCONC_NLINK"] == fr.NLINK
    assert [E["UVC_FAMCONC_" + n] for n, _, _ in fr.SECTIONS] == list(range(E["UVC_NFAMCONC"]))
    assert [E["UVC_FAMCONC_" + n.upper()] for n, _, _ in fr.SECTIONS] == [f for _, f, _ in fr.SECTIONS]
    assert [E["UVC_FAMCONCC_" + n] for n in fr.COUNTER_NAMES] == list(range(7)) and E["UVC_FAMCONCC_reserved"] == 7 and E["UVC_NFAMCONCC"] == 16
    assert _ffi.FAMCONC_COUNTERS == fr.COUNTER_NAMES + ["reserved"]
    assert [fr.depth_bin(ct) for ct in (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 33, 10 ** 6)] == [0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 7, 7, 7]
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_family_concordance_section_name.restype, dll.uvcgpu_family_concordance_section_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_family_concordance_section_name(i).decode() for i in range(E["UVC_NFAMCONC"])] == region.FAMILY_CONCORDANCE
    assert dll.uvcgpu_family_concordance_section_name(-1) is None and dll.uvcgpu_family_concordance_section_name(E["UVC_NFAMCONC"]) is None


# ------------------------------------------------------------------------------------------------ the store
BINS = ["1", "2", "3", "4", "5-7", "8-15", "16-31", "32+"]


def test_the_text_of_a_hand_built_row(tmp_path):
    row = np.zeros(fr.ROW, np.int64)
    row[fr.base_cell(0, 2, 1, 1)] = 9000000000; row[fr.base_cell(0, 2, 1, 3)] = 7; row[fr.base_cell(1, 7, 5, 0)] = 2
    row[fr.base_pos_cell(0, 2, 0)] = 11; row[fr.base_pos_cell(0, 2, 1)] = 5
    row[fr.link_cell(4, LINK_M, LINK_M)] = 40; row[fr.link_cell(4, LINK_M, LINK_I1)] = 3; row[fr.link_pos_cell(4, 0)] = 8
    row[fr.dup_base_cell(1, 1, 3)] = 6; row[fr.dup_base_cell(2, 6, 2)] = 1; row[fr.dup_link_cell(0, 1)] = 4; row[fr.dup_link_cell(8, 0)] = 2
    for i, n in enumerate(fr.COUNTER_NAMES):
        row[fr.C[n]] = 100 + i
    half = row // 2
    plain, gz = tmp_path / "f.tsv", tmp_path / "f.tsv.gz"
    with uio.FamilyConcordance() as s:
        s.add(half); s.add(row - half)         # rows add
        s.write(plain); s.write(gz)
        with pytest.raises(ValueError):
            s.add(row[:-1])
        for path in (tmp_path / "no_such_dir" / "f.tsv", tmp_path / "no_such_dir" / "f.tsv.gz"):
            with pytest.raises(IOError, match="cannot create"):
                s.write(path)
    text = plain.read_text()
    lines = text.splitlines()
    assert lines[0] == "##family_concordance_sections=" + ",".join("%s:%d:%d" % s for s in fr.SECTIONS)
    assert lines[1] == "##family_concordance_bins=" + ",".join(BINS)
    assert lines[2] == "#counter\tcount" and lines[3:10] == ["%s\t%d" % (n, 100 + i) for i, n in enumerate(fr.COUNTER_NAMES)]
    summary = [l for l in lines if l.startswith("#summary\t")]
    assert summary[0] == "#summary\tkind\tbin\tminority_votes\tvotes" and len(summary) == 1 + 16
    assert "#summary\tBASE\t3\t7\t9000000007" in summary and "#summary\tBASE\t32+\t2\t2" in summary and "#summary\tLINK\t5-7\t3\t43" in summary and "#summary\tBASE\t1\t0\t0" in summary
    cells = [l for l in lines[10:] if not l.startswith("#")]                # behind the counters: one line per cell that is not 0
    assert cells == ["BASE\tREF\t3\tC\tC\t9000000000", "BASE\tREF\t3\tC\tT\t7", "BASE\tALT\t32+\tNN\tA\t2", "BASE_POS\tREF\t3\t11\t5",
                     "LINK\t5-7\tM\tM\t40", "LINK\t5-7\tM\tI1\t3", "LINK_POS\t5-7\t8\t0",
                     "DUPLEX_BASE\tC\tC\tT\t6", "DUPLEX_BASE\tG\tNONE\tG\t1", "DUPLEX_LINK\tM\tD3P\t4", "DUPLEX_LINK\tNONE\tM\t2"]
    assert gzip.open(gz, "rt").read() == text
    assert open(gz, "rb").read()[12:16] == b"BC\x02\x00"                    # block-gzipped: the BGZF extra field


# ------------------------------------------------------------------------------------------------ the command line
OUT = ["--family-concordance-out", "f.tsv"]
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_option_as_cli(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    line = [l for l in r.stdout.splitlines() if l.startswith("  --family-concordance-out ")]
    assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == 'default=""', line


@pytest.mark.parametrize("args,both", [
    (PAIR + OUT, ("--family-concordance-out cannot go with --normal-bam", "writes no family concordance report")),
    (BASE + OUT + ["--shard", "1/2"], ("--family-concordance-out", "--shard", "every shard would write a part of the row")),
    (BASE + ["--family-concordance-out=f.tsv", "--repeat=2"], ("--family-concordance-out", "--repeat", "every tile would be counted that many times")),
    (["/only-print-vcf-header/"] + OUT, ("--family-concordance-out", "/only-print-vcf-header/")),
    (BASE + ["--family-concordance-out="], ("--family-concordance-out", "needs a path")),
])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_an_unwritable_path_fails_before_a_device_is_opened(tmp_path):
    """A real BAM and FASTA, so that the run gets as far as its outputs: the probe of the report's path ends it, in front of the device's
    initialisation (which this test's machine may not survive) and of the VCF."""
    reads = synth.generate_region(seed=3, region_len=400, depth=8, beg=2000)
    chrom_len = reads["end"] + 500
    rng = np.random.default_rng(1)
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, chrom_len))
    bam, fa = str(tmp_path / "p.bam"), str(tmp_path / "p.fa")
    bamwriter.write_bam(bam, [("chrA", chrom_len)], bamwriter.records_from_reads(reads, tid=0))
    bamwriter.write_fasta(fa, [("chrA", seq[:reads["beg"]] + reads["refseq"] + seq[reads["end"]:])])
    before = sorted(os.listdir(tmp_path))
    r = run([bam, "-f", fa, "-o", tmp_path / "o.vcf.gz", "--devices", "0", "-t", "1", "--family-concordance-out", tmp_path / "no_such_dir" / "f.tsv"], tmp_path)
    assert r.returncode == 2 and "--family-concordance-out: cannot create" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before            # no VCF either
