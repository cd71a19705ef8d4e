"""The clip sites without a device: the restatement of the definitions (tests/clipsites_restatement.py) on hand-made alignments with every
expected word written out, the struct mirrors and the section table against the header, the store of the reader library
(uvcio_clipsites_*) line for line, and the command line options with their refusals, which come before any file or device is opened."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import clipsites_restatement as cr
from test_bq_correction import make_reads
from uvc_amd import _ffi, io as uio, region

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
OUT = ["--clip-sites-out", "c.tsv"]
SUB_OPTS = [("--clip-sites-min-clip", "10"), ("--clip-sites-min-reads", "3"), ("--clip-sites-min-mapq", "0"), ("--clip-sites-reads", "0")]
M, I, D, N, S, H = 0, 1, 2, 3, 4, 5
BEG, REF_LEN = 1_000_000, 400
NPOS = REF_LEN + 1
WHOLE = [(BEG, BEG + NPOS)]
A_, C_, G_, T_ = 0, 1, 2, 3


def reads_of(specs, mapq=None, fam=None):
    """make_reads of the BQ-correction test from (offset, flag, cigar[, query bases]); bases default to A, qualities to 30.  fam: per read
    (fam_id, fam_strand, frag_id)."""
    full = []
    for sp in specs:
        off, flag, cg = sp[:3]
        L = sum(ln for op, ln in cg if op in (M, I, S))
        b = list(sp[3]) if len(sp) > 3 else [A_] * L
        assert len(b) == L, (cg, len(b), L)
        full.append((off, flag, cg, b, [30] * L))
    r = make_reads(full, beg=BEG, ref_len=REF_LEN)
    if mapq is not None:
        r["mapq"] = np.array(mapq, np.uint8)
    if fam is not None:
        r["fam_id"], r["fam_strand"], r["frag_id"] = (np.array([f[k] for f in fam], t) for k, t in ((0, np.int32), (1, np.uint8), (2, np.int32)))
        r["n_fams"] = int(max(f[0] for f in fam)) + 1
        r["fam_dflag"] = np.zeros(r["n_fams"], np.uint8)
    return r


def site(rng, pos, side, reads, fwd, supp, sec, hard, len_sum, len_max, mapq_sum, spanning, votes):
    """One expected row; votes: {(k, code): n}."""
    row = np.zeros(cr.ROW, np.int64)
    row[:12] = [rng, BEG + pos, side, reads, fwd, supp, sec, hard, len_sum, len_max, mapq_sum, spanning]
    for (k, c), n in votes.items():
        row[cr.VOTE + k * cr.NCODE + c] = n
    return row


def check(got, totals, rows, reads):
    t, r, e = got
    assert t.tolist() == totals + [0] * (8 - len(totals)), t.tolist()
    want = np.array(rows, np.int64).reshape(-1, cr.ROW)
    assert r.shape == want.shape, (r[:, :12].tolist(), want[:, :12].tolist())
    assert np.array_equal(r, want), [(int(i), int(j), int(r[i, j]), int(want[i, j])) for i, j in np.argwhere(r != want)]
    assert e.tolist() == [list(x) for x in reads], e.tolist()


CLIP10 = [A_, C_, G_, T_, A_, C_, G_, T_, A_, C_]


def basic_reads():
    """10S90M, 90M10S, 5H10S85M, 85M10S5H (reverse, supplementary), 12S76M12S and a 300M read that spans five of the six junctions."""
    return reads_of([
        (100, 0, [(S, 10), (M, 90)], CLIP10 + [A_] * 90),
        (100, 0, [(M, 90), (S, 10)], [A_] * 90 + CLIP10),
        (200, 0, [(H, 5), (S, 10), (M, 85)], CLIP10 + [A_] * 85),
        (200, 0x810, [(M, 85), (S, 10), (H, 5)], [A_] * 85 + CLIP10),
        (300, 0, [(S, 12), (M, 76), (S, 12)], [T_] * 12 + [A_] * 76 + [G_] * 11 + [4]),
        (50, 0, [(M, 300)]),
    ], mapq=[60, 50, 40, 30, 20, 10])


def test_the_basic_shapes_hard_clips_flags_and_spanning():
    rs = cr.Restatement(basic_reads())
    left10 = {(k, CLIP10[9 - k]): 1 for k in range(10)}      # LEFT: vote k is the clipped base 9 - k, outward from the junction
    right10 = {(k, CLIP10[k]): 1 for k in range(10)}
    rows = [
        site(0, 100, 0, 1, 1, 0, 0, 0, 10, 10, 60, 1, left10),
        site(0, 190, 1, 1, 1, 0, 0, 0, 10, 10, 50, 1, right10),
        site(0, 200, 0, 1, 1, 0, 0, 1, 15, 15, 40, 1, left10),                          # 5H10S: len 15, the hard-clipped bases have no vote
        site(0, 285, 1, 1, 0, 1, 0, 1, 15, 15, 30, 1, right10),                         # reverse and supplementary
        site(0, 300, 0, 1, 1, 0, 0, 0, 12, 12, 20, 1, {(k, T_): 1 for k in range(12)}),
        site(0, 376, 1, 1, 1, 0, 0, 0, 12, 12, 20, 0, {**{(k, G_): 1 for k in range(11)}, (11, 4): 1}),   # behind the 300M read's end (350); an N base is code 4
    ]
    reads = [(0, 0, 10, 0), (1, 1, 10, 0), (2, 2, 10, 5), (3, 3, 10, 5), (4, 4, 12, 0), (5, 4, 12, 0)]
    check(rs.run(WHOLE, 0, 10, 1), [6, 6, 0, 0, 6], rows, reads)
    # min_clip 13: the 12-base clips are short, the 10S clips too; 5H10S and 10S5H (15) stay
    check(rs.run(WHOLE, 0, 13, 1), [6, 2, 0, 4, 2], [rows[2], rows[3]], [(0, 2, 10, 5), (1, 3, 10, 5)])
    # min_mapq 35: three alignments are counted; the 300M read no longer spans
    r2 = [rows[0].copy(), rows[1].copy(), rows[2].copy()]
    for r in r2:
        r[11] = 0
    check(rs.run(WHOLE, 35, 10, 1), [3, 3, 0, 0, 3], r2, [(0, 0, 10, 0), (1, 1, 10, 0), (2, 2, 10, 5)])
    # min_reads 2: no site; the events are still totals
    check(rs.run(WHOLE, 0, 10, 2), [6, 6, 0, 0, 0], [], [])


def odd_reads():
    """3S2I95M (the insertion sits between the clip and the first aligned op), a CIGAR of 50S alone, a clip of min_clip and one of
    min_clip - 1 at one boundary, and 5M3S2M (a clip between aligned ops)."""
    return reads_of([
        (10, 0, [(S, 3), (I, 2), (M, 95)], [C_, G_, T_] + [A_] * 97),
        (20, 0, [(S, 50)]),
        (150, 0, [(S, 10), (M, 20)], [G_] * 30),
        (150, 0, [(S, 9), (M, 20)], [G_] * 29),
        (250, 0, [(M, 5), (S, 3), (M, 2)]),
    ])


def test_insertion_behind_a_clip_no_aligned_op_min_clip_and_inner_clips():
    rs = cr.Restatement(odd_reads())
    rows3 = [site(0, 10, 0, 1, 1, 0, 0, 0, 3, 3, 60, 0, {(0, T_): 1, (1, G_): 1, (2, C_): 1}),
             site(0, 150, 0, 2, 2, 0, 0, 0, 19, 10, 120, 0, {**{(k, G_): 2 for k in range(9)}, (9, G_): 1})]
    check(rs.run(WHOLE, 0, 3, 1), [5, 3, 0, 0, 3], rows3, [(0, 0, 3, 0), (1, 2, 10, 0), (1, 3, 9, 0)])
    # min_clip 10: 3S and 9S exist and are short; 50S alone and the inner 3S are no events at all
    check(rs.run(WHOLE, 0, 10, 1), [5, 1, 0, 2, 1], [site(0, 150, 0, 1, 1, 0, 0, 0, 10, 10, 60, 0, {(k, G_): 1 for k in range(10)})], [(0, 2, 10, 0)])


def long_clip_reads():
    """RIGHT clips of 31, 32, 33 and 60 bases and a LEFT clip of 60: base i of a clip is i % 4, with one N in front of the LEFT clip's last 32."""
    clip = lambda n: [i % 4 for i in range(n)]                                            # noqa: E731
    left = clip(60)
    left[27] = 4                                                                              # c[27] = vote 32: not counted
    return reads_of([(10 + 70 * j, 0, [(M, 20), (S, n)], [A_] * 20 + clip(n)) for j, n in enumerate((31, 32, 33, 60))] + [(330, 0x10, [(S, 60), (M, 20)], left + [A_] * 20)])


def test_the_vote_is_cut_at_32():
    t, rows, e = cr.Restatement(long_clip_reads()).run(WHOLE, 0, 10, 1)
    assert t.tolist() == [5, 5, 0, 0, 5, 0, 0, 0] and rows[:, 1].tolist() == [BEG + 30, BEG + 100, BEG + 170, BEG + 240, BEG + 330] and rows[:, 2].tolist() == [1, 1, 1, 1, 0]
    assert rows[:, 8].tolist() == [31, 32, 33, 60, 60] and rows[:, 4].tolist() == [1, 1, 1, 1, 0]
    vote = rows[:, cr.VOTE:].reshape(5, 32, 5)
    assert vote.sum((1, 2)).tolist() == [31, 32, 32, 32, 32]
    for j in range(4):                                                                        # RIGHT: vote k = c[k] = k % 4
        assert all(vote[j, k, k % 4] == 1 for k in range(min(32, (31, 32, 33, 60)[j])))
    assert all(vote[4, k, (59 - k) % 4] == 1 for k in range(32)) and vote[4, :, 4].sum() == 0   # LEFT: vote k = c[59 - k]; the N at c[27] is vote 32
    assert cr.consensus(rows[0]) == (31, "".join("ACGT"[k % 4] for k in range(31)))
    assert cr.consensus(rows[4]) == (32, "".join("ACGT"[i % 4] for i in range(28, 60)))      # in reference direction: c[28 .. 60)


def vote_reads():
    """Five reads share the RIGHT boundary 190 with one clipped string, but read 4 differs at k = 2 (4 of 5: upper case) and reads 3 and 4
    differ at k = 5 (3 of 5: lower case); two reads at the RIGHT boundary 300 disagree at k = 0 (a tie: the smaller code, lower case) and
    agree on an N at k = 1; a LEFT and a RIGHT site share p = 240."""
    s = [A_, C_, G_, T_, A_, C_, G_, T_, A_, C_]
    v4 = list(s); v4[2] = T_; v4[5] = A_
    v3 = list(s); v3[5] = A_
    return reads_of([(100, 0, [(M, 90), (S, 10)], [A_] * 90 + c) for c in (s, s, s, v3, v4)]
                    + [(280, 0, [(M, 20), (S, 10)], [A_] * 20 + [C_, 4] + [G_] * 8), (290, 0, [(M, 10), (S, 10)], [A_] * 10 + [A_, 4] + [G_] * 8)]
                    + [(230, 0, [(M, 10), (S, 12)], [A_] * 10 + [T_] * 12), (240, 0x10, [(S, 11), (M, 10)], [C_] * 11 + [A_] * 10)])


def test_majority_lower_case_tie_and_both_sides_at_one_position():
    t, rows, e = cr.Restatement(vote_reads()).run(WHOLE, 0, 10, 1)
    assert t.tolist() == [9, 9, 0, 0, 9, 0, 0, 0]
    assert [(int(r[1]) - BEG, int(r[2]), int(r[3])) for r in rows] == [(190, 1, 5), (240, 0, 1), (240, 1, 1), (300, 1, 2)]
    v = rows[0, cr.VOTE:].reshape(32, 5)
    assert v[2].tolist() == [0, 0, 4, 1, 0] and v[5].tolist() == [2, 3, 0, 0, 0] and v[0].tolist() == [5, 0, 0, 0, 0] and v[10:].sum() == 0
    assert cr.consensus(rows[0]) == (10, "ACGTAcGTAC")
    assert cr.consensus(rows[1]) == (11, "C" * 11) and cr.consensus(rows[2]) == (12, "T" * 12)
    v = rows[3, cr.VOTE:].reshape(32, 5)
    assert v[0].tolist() == [1, 1, 0, 0, 0] and v[1].tolist() == [0, 0, 0, 0, 2]
    assert cr.consensus(rows[3]) == (10, "aN" + "G" * 8)
    assert rows[:, 11].tolist() == [0, 0, 0, 0]                                               # an alignment that ends at p does not span it: [280, 300) and [290, 300) at 300
    assert e.tolist() == [[0, 0, 10, 0], [0, 1, 10, 0], [0, 2, 10, 0], [0, 3, 10, 0], [0, 4, 10, 0], [3, 5, 10, 0], [3, 6, 10, 0], [2, 7, 12, 0], [1, 8, 11, 0]]


def edge_reads():
    """Events at p - beg of 0 and npos - 1, an event inside no range, and spanning across a D op."""
    return reads_of([
        (0, 0, [(S, 10), (M, 20)]),                         # LEFT at x = 0
        (REF_LEN - 20, 0, [(M, 20), (S, 10)]),              # RIGHT at x = npos - 1 = 400
        (100, 0, [(M, 10), (D, 50), (M, 10), (S, 10)]),     # RIGHT at 170; spans 101..169, the deleted positions included
        (120, 0, [(S, 10), (M, 10)]),                       # LEFT at 120, inside the D op of the read above
        (105, 0, [(M, 10), (N, 40), (M, 10)]),              # spans 106..164
    ])


def test_region_edges_ranges_and_spanning_across_a_deletion():
    rs = cr.Restatement(edge_reads())
    none = {(k, A_): 1 for k in range(10)}
    rows = [site(0, 0, 0, 1, 1, 0, 0, 0, 10, 10, 60, 0, none), site(0, 120, 0, 1, 1, 0, 0, 0, 10, 10, 60, 2, none),
            site(0, 170, 1, 1, 1, 0, 0, 0, 10, 10, 60, 0, none), site(0, REF_LEN, 1, 1, 1, 0, 0, 0, 10, 10, 60, 0, none)]
    check(rs.run(WHOLE, 0, 10, 1), [5, 4, 0, 0, 4], rows, [(0, 0, 10, 0), (3, 1, 10, 0), (2, 2, 10, 0), (1, 3, 10, 0)])
    # three ranges, one of a single position: 170 lies in none of them; the range index follows the site
    ranges = [(BEG, BEG + 1), (BEG + 120, BEG + 121), (BEG + 171, BEG + NPOS)]
    r2 = [rows[0].copy(), rows[1].copy(), rows[3].copy()]
    r2[1][0], r2[2][0] = 1, 2
    check(rs.run(ranges, 0, 10, 1), [5, 3, 1, 0, 3], r2, [(0, 0, 10, 0), (2, 1, 10, 0), (1, 3, 10, 0)])


def test_an_event_outside_the_region_adds_its_total_alone():
    """Only the restatement can hold such an alignment: set_reads refuses a read that leaves the region."""
    r = reads_of([(REF_LEN - 19, 0, [(M, 20), (S, 10)]), (-5, 0, [(S, 10), (D, 2), (M, 20)])])     # p - beg = npos, and p - beg = -3
    check(cr.Restatement(r).run(WHOLE, 0, 10, 1), [2, 0, 2, 0, 0], [], [])


HAND_MADE = [basic_reads, odd_reads, long_clip_reads, vote_reads, edge_reads]   # the sets the device test runs as well


# ------------------------------------------------------------------------------------------------ layout and names
def test_struct_mirrors_section_names_and_def_against_the_header():
    E = _ffi.ENUMS
    assert E["UVC_CLIPSITE_ROW"] == 176 == cr.ROW and E["UVC_CLIPSITE_NTOTAL"] == 8 and E["UVC_CLIPSITE_NCONS"] == 32 == cr.NCONS and E["UVC_CLIPSITE_NCODE"] == 5
    assert [n for n, _, _ in _ffi.CLIPSITE_SECTIONS] == cr.SECTIONS + ["reserved", "VOTE"]
    assert [(f, w) for _, f, w in _ffi.CLIPSITE_SECTIONS] == [(k, 1) for k in range(12)] + [(12, 4), (16, 160)]
    assert [E["UVC_CLIPSITE_" + n] for n, _, _ in _ffi.CLIPSITE_SECTIONS] == list(range(E["UVC_NCLIPSITE"]))
    assert _ffi.CLIPSITE_TOTALS == cr.TOTALS and E["UVC_CLIPSITE_LEFT"] == 0 and E["UVC_CLIPSITE_RIGHT"] == 1
    assert C.sizeof(_ffi.UvcClipSitesRequest) == 16 and [n for n, _ in _ffi.UvcClipSitesRequest._fields_] == ["min_mapq", "min_clip", "min_reads", "want_reads"]
    assert C.sizeof(_ffi.UvcClipRead) == 16 and region.CLIP_READ.names == ("site", "read", "soft_len", "hard_len") and region.CLIP_READ.itemsize == 16
    dll = C.CDLL(_ffi.gpu_library_path())
    dll.uvcgpu_clip_site_section_name.restype, dll.uvcgpu_clip_site_section_name.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_clip_site_section_name(i).decode() for i in range(E["UVC_NCLIPSITE"])] == [n for n, _, _ in _ffi.CLIPSITE_SECTIONS]
    assert dll.uvcgpu_clip_site_section_name(-1) is None and dll.uvcgpu_clip_site_section_name(E["UVC_NCLIPSITE"]) is None
    assert hasattr(dll, "uvcgpu_region_clip_sites")


# ------------------------------------------------------------------------------------------------ the store
def store_reads():
    """Site (190, R): five events of three families -- family 0 on both strands (two fragments on strand 0, one on strand 1), family 1 and
    family 2 on one strand each; site (300, R): two events of one fragment's two reads."""
    r = vote_reads()
    fam = [(0, 0, 0), (0, 0, 1), (0, 1, 2), (1, 0, 3), (2, 1, 4), (3, 0, 5), (3, 0, 5), (4, 0, 6), (5, 0, 7)]
    r["fam_id"], r["fam_strand"], r["frag_id"] = (np.array([f[k] for f in fam], t) for k, t in ((0, np.int32), (1, np.uint8), (2, np.int32)))
    r["flag"] = np.array([99, 147, 99, 163, 83, 99, 147, 0, 16], np.uint16)
    r["mapq"] = np.array([60, 59, 58, 57, 56, 55, 54, 53, 52], np.uint8)
    r["qnames"] = ["q3", "q1", "q7", "q2", "q0", "qa", "qa", "qb", "qc"]
    return r


@pytest.mark.parametrize("with_reads", [0, 1])
def test_store_text_line_for_line(tmp_path, with_reads):
    r = store_reads()
    totals, rows, ev = cr.Restatement(r).run(WHOLE, 0, 10, 1)
    events = np.zeros(len(ev), region.CLIP_READ)
    for k, n in enumerate(region.CLIP_READ.names):
        events[n] = ev[:, k]
    late = events[np.isin(ev[:, 0], (2, 3))].copy()
    late["site"] -= 2
    with uio.ClipSites(0, 10, 1, with_reads) as s:
        s.add(19, "chrS", rows[2:], late, r, r["qnames"])                                       # two calls, the later sites first
        s.add(19, "chrS", rows[:2], events[np.isin(ev[:, 0], (0, 1))], r, r["qnames"])
        s.add(19, "chrS", rows[:1])                                                             # a site of two overlapping targets is kept once: the equal row changes nothing,
        fewer = rows[:1].copy()
        fewer[0, cr.W["reads"]] -= 1
        s.add(19, "chrS", fewer)                                                                # ... and neither does a smaller one
        with pytest.raises(ValueError):
            s.add(19, "chrS", rows[:, :100])
        plain, gz = tmp_path / "c.tsv", tmp_path / "c.tsv.gz"
        s.write(plain)
        s.write(gz)
        with pytest.raises(Exception, match="cannot create"):
            s.write(tmp_path / "no_such_dir" / "c.tsv")
    P = BEG + 1
    want = ["##clip_sites_min_mapq=0", "##clip_sites_min_clip=10", "##clip_sites_min_reads=1", "##clip_sites_reads=%d" % with_reads,
            "#S\tcontig\tpos\tside\treads\tfwd\tsupp\tsecondary\thard\tlen_sum\tlen_max\tmapq_sum\tspanning\tfragments\tfamilies\tfamilies_both_strands\tcons_len\tcons",
            "#R\tcontig\tpos\tside\tqname\tflag\tmapq\tsoft_len\thard_len\tfamily_rank\tstrand"]
    S190 = "S\tchrS\t%d\tR\t5\t3\t0\t0\t0\t50\t10\t290\t0\t5\t3\t1\t10\tACGTAcGTAC" % (P + 190)
    # families of (190, R): 0 = {q3/99, q1/147, q7/99} -> least (q1, 147); 1 = {q2/163}; 2 = {q0/83}: ranks 2, 3, 1
    R190 = ["R\tchrS\t%d\tR\tq0\t83\t56\t10\t0\t1\t1", "R\tchrS\t%d\tR\tq1\t147\t59\t10\t0\t2\t0", "R\tchrS\t%d\tR\tq3\t99\t60\t10\t0\t2\t0", "R\tchrS\t%d\tR\tq7\t99\t58\t10\t0\t2\t1",
            "R\tchrS\t%d\tR\tq2\t163\t57\t10\t0\t3\t0"]
    S240L = "S\tchrS\t%d\tL\t1\t0\t0\t0\t0\t11\t11\t52\t0\t1\t1\t0\t11\tCCCCCCCCCCC" % (P + 240)
    S240R = "S\tchrS\t%d\tR\t1\t1\t0\t0\t0\t12\t12\t53\t0\t1\t1\t0\t12\tTTTTTTTTTTTT" % (P + 240)
    S300 = "S\tchrS\t%d\tR\t2\t1\t0\t0\t0\t20\t10\t109\t0\t1\t1\t0\t10\taNGGGGGGGG" % (P + 300)
    want.append(S190)
    if with_reads:
        want += [l % (P + 190) for l in R190]
    want.append(S240L)
    if with_reads:
        want.append("R\tchrS\t%d\tL\tqc\t16\t52\t11\t0\t1\t0" % (P + 240))
    want.append(S240R)
    if with_reads:
        want.append("R\tchrS\t%d\tR\tqb\t0\t53\t12\t0\t1\t0" % (P + 240))
    want.append(S300)
    if with_reads:
        want += ["R\tchrS\t%d\tR\tqa\t99\t55\t10\t0\t1\t0" % (P + 300), "R\tchrS\t%d\tR\tqa\t147\t54\t10\t0\t1\t0" % (P + 300)]
    text = plain.read_text()
    assert text.splitlines() == want
    assert text.endswith("\n") and gzip.open(gz, "rt").read() == text and open(gz, "rb").read()[12:16] == b"BC\x02\x00"
    assert text == cr.report_text([(19, "chrS", rows, ev, r)], 0, 10, 1, with_reads)


# ------------------------------------------------------------------------------------------------ command line
def run(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=str(cwd))


def test_help_lists_the_five_options_with_their_defaults(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in [("--clip-sites-out", '""')] + SUB_OPTS:
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)


PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]


@pytest.mark.parametrize("args,both", [
    (PAIR + OUT, ("--clip-sites-out", "--normal-bam")),
    (PAIR + ["--clip-sites-min-clip", "5"], ("--clip-sites-min-clip", "--normal-bam")),
    (BASE + OUT + ["--shard", "1/2"], ("--clip-sites-out", "--shard")),
    (BASE + OUT + ["--repeat", "2"], ("--clip-sites-out", "--repeat")),
    (["/only-print-vcf-header/"] + OUT, ("--clip-sites-out", "/only-print-vcf-header/")),
] + [(BASE + [g, "1"], (g, "--clip-sites-out")) for g, _ in SUB_OPTS])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("opt,bad", [("--clip-sites-min-clip", b) for b in ("0", "-5", "true", "1.5", "x", "", "1,2", "3e10")]
                         + [("--clip-sites-min-reads", b) for b in ("0", "-1", "false", "2.5", "x", "")]
                         + [("--clip-sites-min-mapq", b) for b in ("-1", "256", "true", "1.5", "x", "")]
                         + [("--clip-sites-reads", b) for b in ("2", "-1", "yes", "0.5", "")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The other reports and what they allow are not refused: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--coverage-out", "c2.tsv", "--read-profile-out", "r.tsv", "--merge-regions", "2000", "--score-mem-mb", "64", "--devices", "0", "-t", "2", "--shard", "0/1",
                          "--repeat", "1", "--clip-sites-min-clip", "20", "--clip-sites-min-reads", "1", "--clip-sites-min-mapq", "30", "--clip-sites-reads", "true"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--clip-sites" not in r.stderr, r.stderr
    r = run(BASE + ["--clip-sites-out="], tmp_path)
    assert r.returncode == 2 and "--clip-sites-out" in r.stderr
