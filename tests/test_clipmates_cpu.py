"""Clip-site mates without a GPU: the restatement of the definitions (tests/clipmates_restatement.py) on a hand-written set with every
expected word written out, the row tables of include/uvc_clipmates.def and their Python mirrors against the header, the P and M lines of
the report store line for line (and the file without them byte for byte as before), and the command line's refusals and --help."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clipmates_restatement as cm
import clipsites_restatement as cr
from test_bq_correction import make_reads
from uvc_amd import _ffi, io as uio

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BEG, REF_LEN, TID = 2_000_000, 4000, 3
M_OP = 0
OC, SS, FAR = cm.OTHER_CONTIG, cm.SAME_STRAND, cm.FAR
FWD, REV = 0x61, 0x91          # a forward first read whose mate is reverse; a reverse second read whose mate is forward


def pair_reads(specs, ref_len=REF_LEN, fam=None):
    """specs: (pos offset, flag, length, mpos, mt[, mapq]) -> (reads dict of the region [BEG, BEG + ref_len) on contig TID, mtid column);
    every alignment is `length`M with bases A.  fam: per read (fam_id, fam_strand, frag_id)."""
    r = make_reads([(s[0], s[1], [(M_OP, s[2])], [0] * s[2], [30] * s[2]) for s in specs], beg=BEG, ref_len=ref_len)
    r["tid"] = TID
    r["mpos"] = np.array([s[3] for s in specs], np.int32)
    r["mapq"] = np.array([s[5] if len(s) > 5 else 60 for s in specs], np.uint8)
    if fam is not None:
        r["fam_id"], r["fam_strand"], r["frag_id"] = (np.array([f[k] for f in fam], t) for k, t in ((0, np.int32), (1, np.uint8), (2, np.int32)))
        r["n_fams"] = int(max(f[0] for f in fam)) + 1
        r["fam_dflag"] = np.zeros(r["n_fams"], np.uint8)
    return r, np.array([s[4] for s in specs], np.int32)


def site_rows(sites):
    """sites: (pos, side) in any order -> clip-site rows ascending by (pos, side), and for every given site its row's index"""
    order = sorted(range(len(sites)), key=lambda i: sites[i])
    rows = np.zeros((len(sites), cr.ROW), np.int64)
    for k, i in enumerate(order):
        rows[k, cr.W["pos"]], rows[k, cr.W["side"]], rows[k, cr.W["reads"]] = sites[i][0], sites[i][1], 3
    index = {i: k for k, i in enumerate(order)}
    return rows, [index[i] for i in range(len(sites))]


HAND_REQ = dict(min_mapq=0, window=100, overhang=5, min_dist=1000, max_gap=50, min_pairs=2)


def hand_made():
    """A RIGHT site at BEG + 500 with forward witnesses on contig 7 in two clusters split by a gap of max_gap + 1, a concordant pair, a
    supplementary line and a mate-unmapped read; a RIGHT site at BEG + 560 that one of those reads faces too; a LEFT site at BEG + 900 with
    same-strand and far witnesses."""
    specs = [
        (400, FWD, 50, 10_000, 7, 60),              # 0  site 0, cluster 0
        (402, FWD, 50, 10_030, 7, 50),              # 1  site 0, cluster 0
        (404, FWD, 50, 10_081, 7, 40),              # 2  site 0, cluster 1: 10 081 - 10 030 = max_gap + 1
        (406, FWD, 50, 10_100, 7, 30),              # 3  site 0, cluster 1
        (408, FWD, 50, BEG + 600, TID),             # 4  concordant at site 0
        (445, FWD, 50, 10_090, 7),                  # 5  ends at BEG + 495: faces site 0 (cluster 1) and site 1 (a cluster of one)
        (400, FWD | 0x800, 50, 10_000, 7),          # 6  supplementary: not a pair read
        (400, FWD | 0x8, 50, 10_000, 7),            # 7  mate unmapped: not a pair read
        (900, REV | 0x20, 50, BEG + 950, TID),      # 8  site 2, same strand
        (910, REV | 0x20, 50, BEG + 960, TID),      # 9  site 2, same strand
        (920, REV, 50, BEG + 920 - 1000, TID),      # 10 site 2, far: |mpos - pos| = min_dist
        (930, REV, 50, BEG - 100, TID),             # 11 site 2, far
    ]
    reads, mtid = pair_reads(specs)
    rows, _ = site_rows([(BEG + 500, cm.RIGHT), (BEG + 560, cm.RIGHT), (BEG + 900, cm.LEFT)])
    return reads, mtid, rows


def test_the_restatement_on_the_hand_written_set():
    reads, mtid, rows = hand_made()
    totals, sr, cl, wit = cm.run(reads, rows, mtid, TID, **HAND_REQ)
    assert totals.tolist() == [10, 11, 1, 10, 5, 4, 2, 0]
    assert sr.tolist() == [[0, 6, 1, 5, 0, 0, 2, 2], [1, 1, 0, 1, 0, 0, 1, 0], [2, 4, 0, 0, 2, 2, 2, 2]]
    assert cl.tolist() == [
        # site mtid strand mpos_min mpos_max pairs other_contig same_strand far mapq_sum first reserved
        [0, 7, 1, 10_000, 10_030, 2, 2, 0, 0, 110, 0, 0],
        [0, 7, 1, 10_081, 10_100, 3, 3, 0, 0, 130, 2, 0],
        [2, TID, 0, BEG - 100, BEG - 80, 2, 0, 0, 2, 120, 6, 0],
        [2, TID, 1, BEG + 950, BEG + 960, 2, 0, 2, 0, 120, 8, 0],
    ]
    assert wit.tolist() == [[0, 0, 0, OC], [0, 1, 0, OC], [0, 2, 1, OC], [0, 5, 1, OC], [0, 3, 1, OC], [1, 5, -1, OC], [2, 11, 2, FAR], [2, 10, 2, FAR], [2, 8, 3, SS], [2, 9, 3, SS]]
    # the gap exactly max_gap joins the two clusters of site 0; min_pairs 1 keeps the cluster of one; mtid None: every mate on TID
    t2, sr2, cl2, _ = cm.run(reads, rows, mtid, TID, **dict(HAND_REQ, max_gap=51, min_pairs=1))
    assert sr2[:, cm.SW["clusters"]].tolist() == [1, 1, 2] and t2.tolist()[4:7] == [4, 4, 3] and cl2[0].tolist() == [0, 7, 1, 10_000, 10_100, 5, 5, 0, 0, 240, 0, 0]
    t3, sr3, cl3, _ = cm.run(reads, rows, None, TID, **HAND_REQ)
    assert sr3[0].tolist() == [0, 6, 1, 0, 0, 5, 2, 2] and t3.tolist()[:4] == [10, 11, 1, 10] and cl3[0, cm.CW["mtid"]] == TID


def test_def_tables_and_python_mirrors_against_the_header():
    E = _ffi.ENUMS
    assert [n for n, _, _ in _ffi.CLIPMATE_SITE_WORDS] == cm.SITE_WORDS and [n for n, _, _ in _ffi.CLIPMATE_CLUSTER_WORDS] == cm.CLUSTER_WORDS
    assert [E["UVC_CLIPMSITE_" + n] for n in cm.SITE_WORDS] == list(range(cm.SITE_ROW)) and E["UVC_NCLIPMSITE"] == E["UVC_CLIPMATE_SITE_ROW"] == cm.SITE_ROW
    assert [E["UVC_CLIPMCLUS_" + n] for n in cm.CLUSTER_WORDS] == list(range(cm.ROW)) and E["UVC_NCLIPMCLUS"] == E["UVC_CLIPMATE_ROW"] == cm.ROW
    assert [(f, w) for _, f, w in _ffi.CLIPMATE_SITE_WORDS] == [(k, 1) for k in range(cm.SITE_ROW)] and [(f, w) for _, f, w in _ffi.CLIPMATE_CLUSTER_WORDS] == [(k, 1) for k in range(cm.ROW)]
    assert _ffi.CLIPMATE_TOTALS == cm.TOTALS and E["UVC_CLIPMATE_NTOTAL"] == cm.NTOTAL
    assert _ffi.CLIPMATE_CLASSES == cm.CLASSES and [E["UVC_CLIPMATE_" + n] for n in cm.CLASSES] == [0, 1, 2, 3] and E["UVC_NCLIPMATECLASS"] == 4
    hdr = open(os.path.join(_ffi.ROOT, "include", "uvcgpu.h")).read()
    req = re.search(r"typedef struct UvcClipMatesRequest \{ int32_t ([^;]*); \}", hdr).group(1).replace(" ", "").split(",")
    assert req == [n for n, _ in _ffi.UvcClipMatesRequest._fields_] == ["tid", "min_mapq", "window", "overhang", "min_dist", "max_gap", "min_pairs", "want_reads"]
    row = re.search(r"typedef struct UvcClipMate \{ int32_t ([^;]*); \}", hdr).group(1).replace(" ", "").split(",")
    assert row == [n for n, _ in _ffi.UvcClipMate._fields_] == ["site", "read", "cluster", "klass"]
    assert C.sizeof(_ffi.UvcClipMatesRequest) == 32 and C.sizeof(_ffi.UvcClipMate) == 16
    # the names the library gives are those of the tables (the library loads without a GPU)
    dll = C.CDLL(_ffi.gpu_library_path())
    for fn, names in (("uvcgpu_clip_mate_site_name", cm.SITE_WORDS), ("uvcgpu_clip_mate_cluster_name", cm.CLUSTER_WORDS), ("uvcgpu_clip_mate_class_name", cm.CLASSES)):
        f = getattr(dll, fn)
        f.restype, f.argtypes = C.c_char_p, [C.c_int32]
        assert [f(k).decode() for k in range(len(names))] == names and f(-1) is None and f(len(names)) is None
    assert hasattr(dll, "uvcgpu_region_clip_mates")


# ------------------------------------------------------------------------------------------------ the store
import test_clipsites_cpu as cscpu  # noqa: E402
import clipjunctions_restatement as cj  # noqa: E402
from uvc_amd import region  # noqa: E402

NAMES = ["chrA", "chrB", "chrC"]
MREQ = (400, 5, 1000, 50, 2)


def store_input():
    """The four sites and nine reads of the clip-site store test ((190, R) (240, L) (240, R) (300, R); families 0..5), with hand-made
    results of a mate call: site 0 has two kept clusters, site 1 none, site 2 no facing read, site 3 one."""
    r = cscpu.store_reads()
    totals, rows, ev = cr.Restatement(r).run(cscpu.WHOLE, 0, 10, 1)
    events = np.zeros(len(ev), region.CLIP_READ)
    for k, n in enumerate(region.CLIP_READ.names):
        events[n] = ev[:, k]
    site_rows = np.array([[0, 9, 3, 4, 0, 2, 3, 2], [1, 2, 1, 0, 1, 0, 1, 0], [2, 0, 0, 0, 0, 0, 0, 0], [3, 3, 0, 3, 0, 0, 1, 1]], np.int64)
    clusters = np.array([[0, 1, 1, 4999, 5120, 4, 4, 0, 0, 230, 0, 0],          # reads 0 1 2 4: family 0 on both strands (three fragments), family 2
                         [0, 19, 0, 77, 77, 2, 0, 0, 2, 111, 4, 0],           # reads 3 7: families 1 and 4
                         [3, 7, 0, 10, 30, 3, 3, 0, 0, 161, 7, 0]], np.int64)  # reads 5 6 8: family 3 (one fragment) and family 5; contig 7 has no name
    wit = np.array([(0, 0, 0, OC), (0, 1, 0, OC), (0, 2, 0, OC), (0, 4, 0, OC), (0, 3, 1, FAR), (0, 7, 1, FAR), (1, 8, -1, SS), (3, 5, 2, OC), (3, 6, 2, OC), (3, 8, 2, OC)], np.int64)
    return r, rows, ev, events, site_rows, clusters, wit


def as_mates(site_rows, clusters, wit):
    w = np.zeros(len(wit), region.CLIP_MATE)
    for k, n in enumerate(region.CLIP_MATE.names):
        w[n] = wit[:, k]
    return site_rows, clusters, w


def mate_text(P):
    return {(190, "R"): ["P\tchrS\t%d\tR\t9\t3\t4\t0\t2\t3\t2" % (P + 191), "M\tchrS\t%d\tR\tchrB\t5000\t5121\t-\t4\t4\t0\t0\t230\t4\t2\t1" % (P + 191), "M\tchrS\t%d\tR\t.\t78\t78\t+\t2\t0\t0\t2\t111\t2\t2\t0" % (P + 191)],
            (240, "L"): ["P\tchrS\t%d\tL\t2\t1\t0\t1\t0\t1\t0" % (P + 241)],
            (240, "R"): ["P\tchrS\t%d\tR\t0\t0\t0\t0\t0\t0\t0" % (P + 241)],
            (300, "R"): ["P\tchrS\t%d\tR\t3\t0\t3\t0\t0\t1\t1" % (P + 301), "M\tchrS\t%d\tR\t.\t11\t31\t+\t3\t3\t0\t0\t161\t2\t2\t0" % (P + 301)]}


@pytest.mark.parametrize("with_reads", [0, 1])
@pytest.mark.parametrize("with_junctions", [0, 1])
def test_store_text_with_mates_line_for_line(tmp_path, with_reads, with_junctions):
    r, rows, ev, events, site_rows, clusters, wit = store_input()
    jrows = np.zeros((4, cj.ROW), np.int64)
    jrows[:, cj.W["site"]] = range(4)
    jrows[:, [cj.W[n] for n in ("best_mm", "second_mm", "partner", "strand", "len", "mate")]] = -1
    # a late call with the sites 2 and 3 alone comes first: its cluster and witness rows index its own rows
    late_ev = events[np.isin(ev[:, 0], (2, 3))].copy()
    late_ev["site"] -= 2
    late = (site_rows[2:].copy(), clusters[2:].copy(), wit[wit[:, 0] >= 2].copy())
    late[0][:, 0] -= 2
    late[1][:, cm.CW["site"]] -= 2
    late[1][:, cm.CW["first"]] -= 7
    late[2][:, 0] -= 2
    late[2][:, 2] -= 2
    with uio.ClipSites(0, 10, 1, with_reads) as s:
        if with_junctions:
            s.set_junctions(3, 8, 2, 500, 7)
        s.set_mates(*MREQ, contig_names=NAMES)
        s.add(19, "chrS", rows[2:], late_ev, r, r["qnames"], junctions=jrows[:2] if with_junctions else None, mates=as_mates(*late))
        s.add(19, "chrS", rows, events, r, r["qnames"], junctions=jrows if with_junctions else None, mates=as_mates(site_rows, clusters, wit))
        fewer = rows[:1].copy()
        fewer[0, cr.W["reads"]] -= 1
        s.add(19, "chrS", fewer, mates=as_mates(np.array([[0, 1, 1, 0, 0, 0, 0, 0]], np.int64), clusters[:0], wit[:0]))   # a smaller site row loses, and its P line with it
        with pytest.raises(ValueError):
            s.add(19, "chrS", rows, mates=as_mates(site_rows[:2], clusters, wit))
        plain, gz = tmp_path / "c.tsv", tmp_path / "c.tsv.gz"
        s.write(plain)
        s.write(gz)
    calls = [(19, "chrS", rows, ev, r)]
    base = (cj.report_text(calls, 0, 10, 1, with_reads, junctions=[jrows], request=(3, 8, 2, 500, 7)) if with_junctions else cr.report_text(calls, 0, 10, 1, with_reads)).splitlines()
    n_head = 9 if with_junctions else 4
    want = base[:n_head] + ["##clip_sites_mate_window=400", "##clip_sites_mate_overhang=5", "##clip_sites_mate_min_dist=1000", "##clip_sites_mate_max_gap=50", "##clip_sites_mate_min_pairs=2"]
    want += base[n_head:n_head + 2 + with_junctions] + [cm.P_COLUMNS, cm.M_COLUMNS]
    lines = mate_text(cscpu.BEG)
    body = base[n_head + 2 + with_junctions:]
    for k, line in enumerate(body):
        want.append(line)
        f = line.split("\t")
        if f[0] == ("J" if with_junctions else "S"):
            want += lines[(int(f[2]) - 1 - cscpu.BEG, f[3])]
    text = plain.read_text()
    assert text.splitlines() == want
    assert sum(l.startswith("M\t") for l in want) == 3 and sum(l.startswith("P\t") for l in want) == 4 and text.endswith("\n")
    import gzip
    assert gzip.open(gz, "rt").read() == text
    assert text == cm.report_text("\n".join(base) + "\n", calls, NAMES, [(site_rows, clusters, wit)], MREQ)


@pytest.mark.parametrize("with_reads", [0, 1])
def test_store_text_with_mates_off_is_todays(tmp_path, with_reads):
    r, rows, ev, events, site_rows, clusters, wit = store_input()
    with uio.ClipSites(0, 10, 1, with_reads) as s:                                              # no set_mates: the rows of a mate call change nothing
        s.add(19, "chrS", rows, events, r, r["qnames"], mates=as_mates(site_rows, clusters, wit))
        s.write(tmp_path / "a.tsv")
    with uio.ClipSites(0, 10, 1, with_reads) as s:
        s.add(19, "chrS", rows, events, r, r["qnames"])
        s.write(tmp_path / "b.tsv")
    with uio.ClipSites(0, 10, 1, with_reads) as s:                                              # set_mates, sites without mate rows: the header lines alone
        s.set_mates(contig_names=NAMES)
        s.add(19, "chrS", rows, events, r, r["qnames"])
        s.write(tmp_path / "c.tsv")
    today = cr.report_text([(19, "chrS", rows, ev, r)], 0, 10, 1, with_reads)
    assert (tmp_path / "a.tsv").read_text() == today == (tmp_path / "b.tsv").read_text()
    c = (tmp_path / "c.tsv").read_text().splitlines()
    assert [l for l in c if not l.startswith(("##clip_sites_mate_", "#P\t", "#M\t"))] == today.splitlines() and len(c) == len(today.splitlines()) + 7
    assert all(l in c for l in cm.mate_header(500, 5, 1000, 500, 2))


# ------------------------------------------------------------------------------------------------ command line
BASE, OUT, run = cscpu.BASE, cscpu.OUT, cscpu.run
ON = ["--clip-sites-mates", "1"]
M_OPTS = [("--clip-sites-mate-window", "500"), ("--clip-sites-mate-overhang", "5"), ("--clip-sites-mate-min-dist", "1000"), ("--clip-sites-mate-max-gap", "500"), ("--clip-sites-mate-min-pairs", "2")]


def test_help_lists_the_six_options_with_their_defaults(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in [("--clip-sites-mates", "0")] + M_OPTS:
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)
    assert "tile border" in r.stdout


@pytest.mark.parametrize("args,both", [(BASE + ON, ("--clip-sites-mates", "--clip-sites-out"))]
                         + [(BASE + [g, v], (g, "--clip-sites-out")) for g, v in M_OPTS]
                         + [(BASE + OUT + [g, v], (g, "--clip-sites-mates 1")) for g, v in M_OPTS]
                         + [(BASE + OUT + ["--clip-sites-mates", "0", g, v], (g, "--clip-sites-mates 1")) for g, v in M_OPTS[:2]]
                         + [(cscpu.PAIR + ON, ("--clip-sites-mates", "--normal-bam")), (BASE + OUT + ON + ["--shard", "1/2"], ("--clip-sites-out", "--shard"))])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("opt,bad", [("--clip-sites-mates", b) for b in ("2", "-1", "yes", "0.5", "")]
                         + [("--clip-sites-mate-window", b) for b in ("0", "-1", "true", "1.5", "x", "", "3e10")]
                         + [("--clip-sites-mate-overhang", b) for b in ("-1", "0.5", "x", "")]
                         + [("--clip-sites-mate-min-dist", b) for b in ("0", "-2", "2.5", "x", "")]
                         + [("--clip-sites-mate-max-gap", b) for b in ("-1", "1.5", "x", "", "1,2")]
                         + [("--clip-sites-mate-min-pairs", b) for b in ("0", "-1", "0.5", "x", "")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + ON + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The options with their report are not refused: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--merge-regions", "2000", "--devices", "0", "-t", "2", "--clip-sites-reads", "1", "--clip-sites-junctions", "1", "--clip-sites-mates", "true", "--clip-sites-mate-window", "1", "--clip-sites-mate-overhang", "0", "--clip-sites-mate-min-dist", "1",
                          "--clip-sites-mate-max-gap", "0", "--clip-sites-mate-min-pairs", "1"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--clip-sites" not in r.stderr, r.stderr
