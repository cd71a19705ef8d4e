"""What of the site-reads report (uvcgpu_region_site_reads, uvcio_sitereads_*, uvc1-mi355x --site-reads-out) runs without a GPU: the restatement
of the definitions (tests/sitereads_restatement.py) on hand-made alignments against rows worked out by hand here, the text of the store for
a small hand-made tile line for line, the struct mirrors and names, and the refusals and --help of the command line."""
import ctypes as C
import os
import subprocess

import numpy as np

import sitereads_restatement as sr
from test_bq_correction import make_reads
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
M, I, D, N, S, H, P, EQ, X = range(9)
BEG, REF_LEN = 1_000_000, 400
REF = [int(v) for v in np.random.default_rng(0).integers(0, 4, REF_LEN)]   # the reference string of make_reads


def query_len(cigar):
    return sum(n for op, n in cigar if op in (M, I, S, EQ, X))


# offset, flag, CIGAR, mapq: the alignments of the issue.  The base of query index j of alignment k is (k + j) % 4, its quality 10 + j.
HAND = [
    (10, 0x0, [(M, 5), (I, 2), (M, 5)], 60),              # 0  site on the anchor (14) and behind it (15)
    (40, 0x10, [(M, 5), (D, 3), (M, 5)], 60),             # 1  site on the anchor (44) and inside the deletion (45..47)
    (70, 0x80, [(M, 5), (I, 2), (D, 3), (M, 5)], 60),     # 2  both events at one anchor (74)
    (100, 0x90, [(M, 5), (N, 100), (M, 5)], 60),          # 3  sites 105..204 lie inside the N: no row, no count
    (220, 0x0, [(M, 5), (N, 100), (I, 2), (M, 5)], 60),   # 4  the insertion's anchor 324 lies inside the N: dropped
    (340, 0x0, [(S, 1), (I, 2), (M, 5)], 60),             # 5  the anchor 339 lies in front of pos: no row
    (350, 0x0, [(M, 3), (I, 1), (P, 1), (I, 1), (M, 3)], 60),   # 6  the lengths add, ins_q is the first
    (360, 0x0, [(M, 5), (I, 2), (S, 3)], 60),             # 7  an insertion behind the last aligned base
    (370, 0x90, [(H, 2), (EQ, 3), (X, 2), (M, 2), (H, 2)], 60),   # 8  = and X ops, hard clips, a reverse R2 read
    (380, 0x0, [(D, 5)], 60),                             # 9  l_qseq 0: adds nothing
    (385, 0x0, [(M, 5)], 29),                             # 10 just below the gate of 30
    (385, 0x10, [(M, 5)], 30),                            # 11 at the gate
]


def hand_made_reads():
    specs = []
    for k, (off, flag, cigar, _) in enumerate(HAND):
        n = query_len(cigar)
        specs.append((off, flag, cigar, [(k + j) % 4 for j in range(n)], [10 + j for j in range(n)]))
    r = make_reads(specs, beg=BEG, ref_len=REF_LEN)
    r["mapq"] = np.array([m for _, _, _, m in HAND], np.uint8)
    return r


def rows_of(rows, read):
    """(position offset, q, kind, quality, ins_q, ins_len, del_len) of one alignment's rows; `site` is an index into the dense list"""
    return [(int(r["site"]), int(r["q"]), int(r["obs"]) & 0xFF, int(r["obs"]) >> 8, int(r["ins_q"]), int(r["ins_len"]), int(r["del_len"])) for r in rows[rows["read"] == read]]


def base(k, q):
    return (k + q) % 4


def test_restatement_on_the_hand_made_alignments():
    reads = hand_made_reads()
    rs = sr.Restatement(reads)
    dense = np.arange(BEG, BEG + REF_LEN + 1)
    rows, counts = rs.site_reads(dense, 0, 0)
    assert rows.dtype == sr.ROW and rows.dtype.itemsize == 32 and counts.shape == (REF_LEN + 1, 8) and not rows["reserved"].any()
    assert (np.diff(rows["read"].astype(np.int64) * 1000 + rows["site"]) > 0).all()           # ascending by (read, site)
    # 0: 5M2I5M at 10: query 0..4 at 10..14, the insertion (query 5, 6) on the row of 14, query 7..11 at 15..19
    assert rows_of(rows, 0) == [(10 + j, j, base(0, j), 10 + j, -1, 0, 0) for j in range(4)] + [(14, 4, base(0, 4), 14, 5, 2, 0)] + \
        [(15 + j, 7 + j, base(0, 7 + j), 17 + j, -1, 0, 0) for j in range(5)]
    # 1: 5M3D5M at 40: the deletion is announced on the row of 44; 45..47 are kind 5 with the base in front of the op (query 4)
    assert rows_of(rows, 1) == [(40 + j, j, base(1, j), 10 + j, -1, 0, 0) for j in range(4)] + [(44, 4, base(1, 4), 14, -1, 0, 3)] + \
        [(45 + j, 4, 5, 14, -1, 0, 0) for j in range(3)] + [(48 + j, 5 + j, base(1, 5 + j), 15 + j, -1, 0, 0) for j in range(5)]
    # 2: 5M2I3D5M at 70: both events on the row of 74
    r2 = rows_of(rows, 2)
    assert r2[4] == (74, 4, base(2, 4), 14, 5, 2, 3) and r2[5:8] == [(75 + j, 6, 5, 16, -1, 0, 0) for j in range(3)] and len(r2) == 13
    assert r2[8] == (78, 7, base(2, 7), 17, -1, 0, 0)
    # 3: 5M100N5M at 100: nothing inside the N
    r3 = rows_of(rows, 3)
    assert [t[0] for t in r3] == list(range(100, 105)) + list(range(205, 210)) and r3[5][1] == 5
    assert not counts[105:205].any() and not ((rows["site"] >= 105) & (rows["site"] < 205)).any()
    # 4: 5M100N2I5M at 220: the insertion is dropped
    r4 = rows_of(rows, 4)
    assert [t[0] for t in r4] == list(range(220, 225)) + list(range(325, 330)) and all(t[4:] == (-1, 0, 0) for t in r4) and r4[5][1] == 7
    # 5: 1S2I5M at 340: the anchor 339 is not covered; query 3..7 at 340..344
    assert rows_of(rows, 5) == [(340 + j, 3 + j, base(5, 3 + j), 13 + j, -1, 0, 0) for j in range(5)] and not counts[339].any()
    # 6: 3M1I1P1I3M at 350: one row with ins_len 2 and the first inserted base's index
    r6 = rows_of(rows, 6)
    assert r6[2] == (352, 2, base(6, 2), 12, 3, 2, 0) and r6[3] == (353, 5, base(6, 5), 15, -1, 0, 0) and len(r6) == 6
    # 7: 5M2I3S at 360: the insertion on the last aligned base
    r7 = rows_of(rows, 7)
    assert r7[4] == (364, 4, base(7, 4), 14, 5, 2, 0) and len(r7) == 5
    # 8: 2H3=2X2M2H at 370, reverse R2: query 0..6 at 370..376
    assert rows_of(rows, 8) == [(370 + j, j, base(8, j), 10 + j, -1, 0, 0) for j in range(7)]
    # 9: l_qseq 0
    assert not (rows["read"] == 9).any() and not counts[380:385].any()
    # 10, 11: the mapq gate
    assert len(rows_of(rows, 10)) == 5 and len(rows_of(rows, 11)) == 5 and counts[385:390, :4].sum() == 10
    g_rows, g_counts = rs.site_reads(dense, 30, 0)
    assert not (g_rows["read"] == 10).any() and len(rows_of(g_rows, 11)) == 5 and g_counts[385:390, :4].sum() == 5 and len(g_rows) == len(rows) - 5
    # the counts: every kind of column 0..5 is the rows of that kind; column 6 / 7 the rows with an event
    for k in range(6):
        assert np.array_equal(counts[:, k], np.bincount(rows["site"][(rows["obs"] & 0xFF) == k], minlength=len(dense)))
    assert counts[:, 6].sum() == 4 and counts[[14, 74, 352, 364], 6].tolist() == [1, 1, 1, 1] and counts[:, 7].sum() == 2 and counts[[44, 74], 7].tolist() == [1, 1]
    assert counts[:, 5].sum() == 6
    # alt_only: the deletions, the rows with events and the bases that differ from the reference; the counts do not move
    a_rows, a_counts = rs.site_reads(dense, 0, 1)
    assert np.array_equal(a_counts, counts)
    kind, pos = rows["obs"] & 0xFF, rows["site"]
    ref = np.array(REF + [4])[pos]
    want = (kind == 5) | (rows["ins_len"] > 0) | (rows["del_len"] > 0) | ((kind <= 3) & (ref <= 3) & (kind != ref))
    assert np.array_equal(a_rows, rows[want]) and 6 + 5 < len(a_rows) < len(rows)
    # the region's last position has no reference base: a list of that site alone
    rows1, counts1 = rs.site_reads([BEG + REF_LEN], 0, 0)
    assert len(rows1) == 0 and not counts1.any()
    # a sparse list: the site index is the index into the list
    rows2, counts2 = rs.site_reads([BEG + 14, BEG + 15, BEG + 44, BEG + 46, BEG + 150, BEG + 339], 0, 1)
    assert [(int(r["site"]), int(r["read"]), int(r["ins_len"]), int(r["del_len"]), int(r["obs"]) & 0xFF) for r in rows2 if r["ins_len"] or r["del_len"] or (r["obs"] & 0xFF) == 5] == \
        [(0, 0, 2, 0, base(0, 4)), (2, 1, 0, 3, base(1, 4)), (3, 1, 0, 0, 5)]
    assert counts2[4].sum() == 0 and counts2[5].sum() == 0 and counts2[0].sum() == 2 and counts2[0, 6] == 1


def test_struct_mirrors_and_names():
    E = _ffi.ENUMS
    assert C.sizeof(_ffi.UvcSiteRead) == 32 and C.sizeof(_ffi.UvcSiteReadsRequest) == 8 and region.SITE_READ.itemsize == 32
    assert [n for n, _ in _ffi.UvcSiteRead._fields_] == sr.FIELDS == list(region.SITE_READ.names)
    assert region.SITE_READ_KINDS == sr.KINDS and E["UVC_SITEREAD_DEL"] == sr.DEL and E["UVC_SITEREAD_NCOL"] == sr.NCOL
    assert E["UVC_SITEREAD_COL_INS"] == sr.COL_INS and E["UVC_SITEREAD_COL_DEL_AFTER"] == sr.COL_DEL_AFTER
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_site_read_kind_name.restype, dll.uvcgpu_site_read_kind_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_site_read_kind_name(i).decode() for i in range(6)] == sr.KINDS
    assert dll.uvcgpu_site_read_kind_name(-1) is None and dll.uvcgpu_site_read_kind_name(6) is None
    assert hasattr(dll, "uvcgpu_region_site_reads")


# ------------------------------------------------------------------------------------------------ the store's text
def small_tile(fam_ids=(7, 7, 7, 3, 9)):
    """Five alignments of three families on three sites of chr1; rows as a call with alt_only = 0 could return them."""
    f7a, f7b, f7c, f3, f9 = fam_ids
    reads = dict(flag=np.array([99, 147, 83, 0, 16], np.uint16), mapq=np.array([60, 60, 50, 40, 30], np.uint8), l_qseq=np.full(5, 10, np.int32),
                 fam_id=np.array([f7a, f7b, f7c, f3, f9], np.int32), fam_strand=np.array([0, 0, 1, 0, 0], np.uint8), frag_id=np.array([0, 0, 1, 0, 0], np.int32),
                 bases=np.array([(a + j) % 4 for a in range(5) for j in range(10)], np.uint8), seq_off=np.arange(5, dtype=np.int64) * 10)
    qnames = ["r1", "r1", "r2", "r0", "r3"]
    rows = np.array([(0, 0, 2, 1 | 30 << 8, -1, 0, 0, 0), (0, 1, 3, 1 | 31 << 8, -1, 0, 0, 0), (0, 2, 4, 1 | 32 << 8, -1, 0, 0, 0), (0, 3, 5, 2 | 20 << 8, 6, 2, 3, 0),
                     (1, 3, 9, 0 | 12 << 8, -1, 0, 0, 0), (0, 4, 0, 5 | 25 << 8, -1, 0, 0, 0), (1, 4, 5, 3 | 11 << 8, -1, 0, 0, 0)], dtype=sr.ROW)
    counts = np.array([[0, 3, 1, 0, 0, 1, 1, 1], [1, 0, 0, 1, 0, 0, 0, 0], [0] * 8], np.int32)
    return [99, 104, 200], "ATG", counts, rows, reads, qnames


WANT_TEXT = """##site_reads_min_mapq=5
##site_reads_alt_only=0
#S\tcontig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tDEL\tINS\tDEL_after
#A\tcontig\tpos\tallele\treads\tfragments\tfamilies\tfamilies_both_strands
#R\tcontig\tpos\tobs\tqual\tcycle\tclass\tmapq\tqname\tflag\tfamily\tstrand\tins\tdel
S\tchr1\t100\tA\t5\t0\t3\t1\t0\t0\t1\t1\t1
A\tchr1\t100\tC\t3\t2\t1\t1
A\tchr1\t100\tDEL\t1\t1\t1\t0
A\tchr1\t100\t+CG\t1\t1\t1\t0
A\tchr1\t100\t-3\t1\t1\t1\t0
R\tchr1\t100\tG\t20\t5\tR1_fwd\t40\tr0\t0\t1\t0\tCG\t3
R\tchr1\t100\tC\t30\t2\tR1_fwd\t60\tr1\t99\t2\t0\t.\t0
R\tchr1\t100\tC\t31\t6\tR2_rev\t60\tr1\t147\t2\t0\t.\t0
R\tchr1\t100\tC\t32\t5\tR1_rev\t50\tr2\t83\t2\t1\t.\t0
R\tchr1\t100\tDEL\t25\t9\tR1_rev\t30\tr3\t16\t3\t0\t.\t0
S\tchr1\t105\tT\t2\t1\t0\t0\t1\t0\t0\t0\t0
A\tchr1\t105\tA\t1\t1\t1\t0
A\tchr1\t105\tT\t1\t1\t1\t0
R\tchr1\t105\tA\t12\t9\tR1_fwd\t40\tr0\t0\t1\t0\t.\t0
R\tchr1\t105\tT\t11\t4\tR1_rev\t30\tr3\t16\t2\t0\t.\t0
S\tchr1\t201\tG\t0\t0\t0\t0\t0\t0\t0\t0\t0
S\tchr2\t50\t.\t0\t0\t0\t0\t0\t0\t0\t0\t0
"""


def store_text(tmp_path, name, fam_ids, listed_first):
    sites, ref, counts, rows, reads, qnames = small_tile(fam_ids)
    with uio.SiteReads(region.SITE_READ_KINDS, region.READ_CLASSES, min_mapq=5, alt_only=False) as st:
        if listed_first:   # as the command line does: every listed site with its reference base, then the tiles without
            st.add(0, "chr1", sites, ref)
            st.add(1, "chr2", [49])
            st.add(0, "chr1", sites, None, counts, rows, reads, qnames)
        else:
            st.add(0, "chr1", sites, ref, counts, rows, reads, qnames)
            st.add(1, "chr2", [49])
        st.write(tmp_path / name)
    return open(tmp_path / name).read()


def test_store_text_line_for_line(tmp_path):
    got = store_text(tmp_path, "a.tsv", (7, 7, 7, 3, 9), False)
    assert got.splitlines() == WANT_TEXT.splitlines() and got == WANT_TEXT
    # the family column is a rank by (qname, flag): other ids of the same grouping, and the order of the adds, leave the bytes alone
    assert store_text(tmp_path, "b.tsv", (100, 100, 100, 200, 5), True) == WANT_TEXT
    # .gz: the same text, block-gzipped
    import gzip
    sites, ref, counts, rows, reads, qnames = small_tile()
    with uio.SiteReads(region.SITE_READ_KINDS, region.READ_CLASSES, 5, False) as st:
        st.add(0, "chr1", sites, ref, counts, rows, reads, qnames)
        st.add(1, "chr2", [49])
        st.write(tmp_path / "c.tsv.gz")
    assert gzip.open(tmp_path / "c.tsv.gz", "rt").read() == WANT_TEXT and open(tmp_path / "c.tsv.gz", "rb").read()[12:16] == b"BC\x02\x00"


# ------------------------------------------------------------------------------------------------ command line
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--site-reads-out", "s.tsv", "--site-reads-sites", "sites.bed"]


def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_options_as_cli_with_their_defaults(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in (("--site-reads-out", '""'), ("--site-reads-sites", '""'), ("--site-reads-min-mapq", "0"), ("--site-reads-alt-only", "1")):
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


def test_cli_refusals_before_any_file_or_device(tmp_path):
    cases = [
        (BASE + OUT + ["--normal-bam", "n.bam"], ["--site-reads-out", "--normal-bam", "site reads report"]),
        (BASE + OUT + ["--shard", "1/2"], ["--site-reads-out", "--shard 1/2"]),
        (BASE + OUT + ["--repeat", "3"], ["--site-reads-out", "--repeat 3"]),
        (["/only-print-vcf-header/"] + OUT, ["--site-reads-out", "/only-print-vcf-header/"]),
        (BASE + ["--site-reads-sites", "sites.bed"], ["--site-reads-sites needs --site-reads-out"]),
        (BASE + ["--site-reads-min-mapq", "20"], ["--site-reads-min-mapq needs --site-reads-out"]),
        (BASE + ["--site-reads-alt-only", "0"], ["--site-reads-alt-only needs --site-reads-out"]),
        (BASE + ["--site-reads-out", "s.tsv"], ["--site-reads-out needs --site-reads-sites"]),
        (BASE + ["--site-reads-out", ""] + OUT[2:], ["--site-reads-out needs a path"]),
        (BASE + OUT[:2] + ["--site-reads-sites", ""], ["--site-reads-sites needs a path"]),
        (BASE + OUT + ["--site-reads-min-mapq", "256"], ["--site-reads-min-mapq", "'256'"]),
        (BASE + OUT + ["--site-reads-min-mapq", "-1"], ["--site-reads-min-mapq", "'-1'"]),
        (BASE + OUT + ["--site-reads-min-mapq", "3.5"], ["--site-reads-min-mapq", "'3.5'"]),
        (BASE + OUT + ["--site-reads-min-mapq", "true"], ["--site-reads-min-mapq", "'true'"]),
        (BASE + OUT + ["--site-reads-alt-only", "2"], ["--site-reads-alt-only", "'2'"]),
        (BASE + OUT + ["--site-reads-alt-only", "yes"], ["--site-reads-alt-only", "'yes'"]),
    ]
    for args, words in cases:
        r = run(args, tmp_path)
        assert r.returncode == 2 and all(w in r.stderr for w in words), (args, r.returncode, r.stderr)
        assert os.listdir(tmp_path) == [], args
    # true / false are values of --site-reads-alt-only, as for --merge-regions: these get as far as the missing BAM
    for v in ("true", "false", "1", "0"):
        r = run(BASE + OUT + ["--site-reads-alt-only", v], tmp_path)
        assert r.returncode != 0 and "--site-reads" not in r.stderr, (v, r.stderr)
