"""The clip-site junctions without a device: the restatement of the definitions (tests/clipjunctions_restatement.py) on hand-written cases
with every expected word written out, the section table and the struct mirrors against the header, the J lines of the store of the reader
library (uvcio_clipsites_set_junctions / _add_junctions) line for line, the store's text with junctions off against today's, and the
command line options with their refusals, which come before any file or device is opened."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import clipjunctions_restatement as cj
import clipsites_restatement as cr
import test_clipsites_cpu as cpu
from uvc_amd import _ffi, io as uio, region

BEG = 1000
LEFT, RIGHT = cj.LEFT, cj.RIGHT
COMP = {0: 3, 1: 2, 2: 1, 3: 0}
# 240 bases; the events: a deletion of [60, 100), a tandem duplication of [130, 150), an inversion of [170, 210)
REF = ("GTCAGGTACCTTAGCGATCCATGGCTAAGTCCGATTACGCAGGTTCAAGCTTGGATCCAA" "TGCTAGGCTTAACCGTAGCATCGGATATCCGTAAGCTTGC" "AGTCCATGGTACGATCGGCTAAGCTAGCAT" "CGGATTACCGTAGCTAACGG"
       "TTAGCCATAGGCTAAGTCCG" "ATCGGTACCATGGCAATCGCGTATTAGCCGATGGCTTAAC" "GGATCAGCTTACGGTACCAATGCGTCAAGG")
assert len(REF) == 240


def site(x, side, q):
    """A site row at BEG + x whose vote k has three votes for q[k]."""
    row = np.zeros(cr.ROW, np.int64)
    row[cr.W["pos"]], row[cr.W["side"]], row[cr.W["reads"]] = BEG + x, side, 3
    for k, c in enumerate(q):
        row[cr.VOTE + k * cr.NCODE + c] = 3
    return row


def fwd(ref, xs):
    return [cj.CODE[ref[x]] for x in xs]


def rev(ref, xs):
    return [COMP[cj.CODE[ref[x]]] for x in xs]


def junction(s, qlen, cmp_len, status, best_mm=-1, n_best=0, second=-1, partner=-1, strand=-1, klass=cj.NONE, ln=-1, mate=-1, hist=()):
    return [s, qlen, cmp_len, status, best_mm, n_best, second, partner, strand, klass, ln, mate] + list(hist) + [0] * (cj.NHIST - len(hist)) + [0, 0, 0, 0]


def check(got, totals, rows):
    t, j = got
    assert t.tolist() == totals + [0] * (cj.NTOTAL - len(totals)), t.tolist()
    want = np.array(rows, np.int64).reshape(-1, cj.ROW)
    assert j.shape == want.shape and np.array_equal(j, want), [(int(a), int(b), int(j[a, b]), int(want[a, b])) for a, b in np.argwhere(j != want)]


def event_rows():
    """Both ends of the deletion, of the duplication and of the inversion (its outer reads and the inverted segment's), 20 clipped bases each."""
    return np.stack([
        site(60, RIGHT, fwd(REF, range(100, 120))),          # 0: aligned up to 60, the clip continues at 100
        site(100, LEFT, fwd(REF, range(59, 39, -1))),        # 1: aligned from 100, the clip ends at 59
        site(130, LEFT, fwd(REF, range(149, 129, -1))),      # 2: aligned from 130 (the second copy), the clip is the end of the first copy
        site(150, RIGHT, fwd(REF, range(130, 150))),         # 3: aligned up to 150, the clip is the second copy
        site(170, LEFT, rev(REF, range(210, 230))),          # 4: the inverted segment's read, aligned from 170, clipped into what follows 210
        site(170, RIGHT, rev(REF, range(209, 189, -1))),     # 5: aligned up to 170, the clip runs down from 209 on the other strand
        site(210, LEFT, rev(REF, range(170, 190))),          # 6: aligned from 210, the clip is the segment's begin on the other strand
        site(210, RIGHT, rev(REF, range(169, 149, -1))),     # 7: the inverted segment's read, aligned up to 210
    ])


def test_deletion_duplication_and_inversion_with_both_ends():
    one = [1]
    check(cj.run(REF, BEG, event_rows()), [8, 8, 8, 8, 8], [
        junction(0, 20, 20, 2, 0, 1, -1, BEG + 100, 0, cj.DEL, 40, 1, one),
        junction(1, 20, 20, 2, 0, 1, -1, BEG + 60, 0, cj.DEL, 40, 0, one),
        junction(2, 20, 20, 2, 0, 1, -1, BEG + 150, 0, cj.DUP, 20, 3, one),
        junction(3, 20, 20, 2, 0, 1, -1, BEG + 130, 0, cj.DUP, 20, 2, one),
        junction(4, 20, 20, 2, 0, 1, -1, BEG + 210, 1, cj.INV, 40, 6, one),
        junction(5, 20, 20, 2, 0, 1, -1, BEG + 210, 1, cj.INV, 40, 7, one),
        junction(6, 20, 20, 2, 0, 1, -1, BEG + 170, 1, cj.INV, 40, 4, one),
        junction(7, 20, 20, 2, 0, 1, -1, BEG + 170, 1, cj.INV, 40, 5, one),
    ])


def test_gates_holes_mismatches_and_status():
    rows = event_rows()[[0, 1]]
    rows[0, cr.VOTE + 5 * cr.NCODE:cr.VOTE + 6 * cr.NCODE] = [0, 0, 0, 0, 3]                 # k = 5: the winner is code 4
    rows[0, cr.VOTE + 6 * cr.NCODE:cr.VOTE + 7 * cr.NCODE] = 0
    rows[0, cr.VOTE + 6 * cr.NCODE + (cj.CODE[REF[106]] + 1) % 4] = 1                         # k = 6: one vote, for a wrong base
    k7 = cj.CODE[REF[107]]
    rows[0, cr.VOTE + 7 * cr.NCODE + k7], rows[0, cr.VOTE + 7 * cr.NCODE + (k7 + 1) % 4] = 3, 2   # k = 7: 3 of 5, 9 < 10
    rows[1, cr.VOTE + 2 * cr.NCODE:cr.VOTE + 3 * cr.NCODE] = 0
    rows[1, cr.VOTE + 2 * cr.NCODE + (cj.CODE[REF[57]] + 2) % 4] = 3                          # k = 2 of the LEFT site: a wrong base, compared
    check(cj.run(REF, BEG, rows, min_votes=2, min_len=17, max_mismatch=1), [2, 2, 2, 2, 2], [
        junction(0, 20, 17, 2, 0, 1, -1, BEG + 100, 0, cj.DEL, 40, 1, [1]),
        junction(1, 20, 20, 2, 1, 1, -1, BEG + 60, 0, cj.DEL, 40, 0, [0, 1])])
    check(cj.run(REF, BEG, rows, min_votes=2, min_len=18, max_mismatch=0), [2, 1, 0, 0, 0], [       # 17 compared: not searched; one mismatch: not placed
        junction(0, 20, 17, 0), junction(1, 20, 20, 1)])
    check(cj.run(REF, BEG, rows, min_votes=1, min_len=18, max_mismatch=1, max_dist=39), [2, 2, 0, 0, 0], [   # min_votes 1: k = 6 is compared (and differs); 40 > max_dist
        junction(0, 20, 18, 1), junction(1, 20, 20, 1)])
    check(cj.run(REF, BEG, rows, min_votes=1, min_len=18, max_mismatch=1, max_dist=40, mate_slop=0), [2, 2, 2, 2, 2], [
        junction(0, 20, 18, 2, 1, 1, -1, BEG + 100, 0, cj.DEL, 40, 1, [0, 1]), junction(1, 20, 20, 2, 1, 1, -1, BEG + 60, 0, cj.DEL, 40, 0, [0, 1])])
    check(cj.run(REF, BEG, rows[:0]), [0], [])


# 160 bases; [40, 44) = [90, 94) = ACGT: a deletion of [40, 90) or of [44, 94), the same sample -- the aligner extends both alignments over
# the four bases, so the two ends lie at 44 (RIGHT) and 90 (LEFT), four apart from each other's partner
MH = "TTGGCAATCCGGATTAGCCATAGGCTTAACGGTCAGGCTA" "ACGT" "GATTCCGGTAAGCTTGCATCCGGATAGCTAGGCTTAACCGGATTGC" "ACGT" "CCATGGTTAACCGGTATTCGGCATTAGCCGGATACCGTAGGCTTAAGGCCTTAGCGATCGGTCAAG"
assert len(MH) == 160 and MH[40:44] == MH[90:94] == "ACGT"


def test_microhomology_moves_the_ends_apart():
    rows = np.stack([site(44, RIGHT, fwd(MH, range(94, 114))), site(90, LEFT, fwd(MH, range(39, 19, -1)))])
    check(cj.run(MH, BEG, rows, mate_slop=10), [2, 2, 2, 2, 2], [
        junction(0, 20, 20, 2, 0, 1, -1, BEG + 94, 0, cj.DEL, 50, 1, [1]), junction(1, 20, 20, 2, 0, 1, -1, BEG + 40, 0, cj.DEL, 50, 0, [1])])
    check(cj.run(MH, BEG, rows, mate_slop=4), [2, 2, 2, 2, 2], [
        junction(0, 20, 20, 2, 0, 1, -1, BEG + 94, 0, cj.DEL, 50, 1, [1]), junction(1, 20, 20, 2, 0, 1, -1, BEG + 40, 0, cj.DEL, 50, 0, [1])])
    check(cj.run(MH, BEG, rows, mate_slop=3), [2, 2, 2, 2, 0], [
        junction(0, 20, 20, 2, 0, 1, -1, BEG + 94, 0, cj.DEL, 50, -1, [1]), junction(1, 20, 20, 2, 0, 1, -1, BEG + 40, 0, cj.DEL, 50, -1, [1])])


# ------------------------------------------------------------------------------------------------ layout and names
def test_def_file_struct_mirror_and_names_against_the_header():
    E = _ffi.ENUMS
    assert E["UVC_CLIPJUNC_ROW"] == 24 == cj.ROW and E["UVC_CLIPJUNC_NTOTAL"] == 8 == cj.NTOTAL and E["UVC_CLIPJUNC_NHIST"] == 8 == cj.NHIST
    assert [n for n, _, _ in _ffi.CLIPJUNC_SECTIONS] == cj.SECTIONS + ["hist", "reserved"]
    assert [(f, w) for _, f, w in _ffi.CLIPJUNC_SECTIONS] == [(k, 1) for k in range(12)] + [(12, 8), (20, 4)] and cj.HIST == 12
    assert [E["UVC_CLIPJUNC_" + n] for n, _, _ in _ffi.CLIPJUNC_SECTIONS] == list(range(E["UVC_NCLIPJUNC"]))
    assert _ffi.CLIPJUNC_TOTALS == cj.TOTALS and _ffi.CLIP_CLASSES == cj.CLASSES
    assert [E["UVC_CLIPJUNC_" + n] for n in ("NOT_SEARCHED", "NOT_PLACED", "PLACED")] == [cj.NOT_SEARCHED, cj.NOT_PLACED, cj.PLACED]
    assert C.sizeof(_ffi.UvcClipJunctionsRequest) == 20 and [n for n, _ in _ffi.UvcClipJunctionsRequest._fields_] == ["min_votes", "min_len", "max_mismatch", "max_dist", "mate_slop"]
    dll = C.CDLL(_ffi.gpu_library_path())
    for fn in (dll.uvcgpu_clip_junction_section_name, dll.uvcgpu_clip_class_name):
        fn.restype, fn.argtypes = C.c_char_p, [C.c_int32]
    assert [dll.uvcgpu_clip_junction_section_name(i).decode() for i in range(E["UVC_NCLIPJUNC"])] == [n for n, _, _ in _ffi.CLIPJUNC_SECTIONS]
    assert [dll.uvcgpu_clip_class_name(i).decode() for i in range(E["UVC_NCLIPCLASS"])] == cj.CLASSES
    assert dll.uvcgpu_clip_junction_section_name(-1) is None and dll.uvcgpu_clip_junction_section_name(E["UVC_NCLIPJUNC"]) is None and dll.uvcgpu_clip_class_name(5) is None
    assert hasattr(dll, "uvcgpu_region_clip_junctions") and hasattr(region.Region, "clip_junctions")


# ------------------------------------------------------------------------------------------------ the store
def store_input():
    r = cpu.store_reads()
    totals, rows, ev = cr.Restatement(r).run(cpu.WHOLE, 0, 10, 1)
    events = np.zeros(len(ev), region.CLIP_READ)
    for k, n in enumerate(region.CLIP_READ.names):
        events[n] = ev[:, k]
    assert [(int(x[cr.W["pos"]]) - cpu.BEG, int(x[cr.W["side"]])) for x in rows] == [(190, 1), (240, 0), (240, 1), (300, 1)]
    P = cpu.BEG
    jrows = np.array([junction(0, 10, 9, 2, 1, 1, 3, P + 299, 0, cj.DEL, 109, 3, [0, 1, 0, 2]),          # placed, mated with (300, R)
                      junction(1, 11, 11, 0),                                                           # not searched
                      junction(2, 12, 12, 1),                                                           # searched, not placed
                      junction(3, 10, 8, 2, 0, 2, 0, P + 20, 1, cj.INV, 280, -1, [2])], np.int64)       # placed twice, no mate
    return r, rows, ev, events, jrows


J_LINES = {(190, "R"): "J\tchrS\t%d\tR\t10\t9\t2\t1\t1\t3\t%d\t+\tDEL\t109\t%d\tR" % (cpu.BEG + 191, cpu.BEG + 300, cpu.BEG + 301),
           (240, "L"): "J\tchrS\t%d\tL\t11\t11\t0\t.\t0\t.\t.\t.\tNONE\t.\t.\t." % (cpu.BEG + 241),
           (240, "R"): "J\tchrS\t%d\tR\t12\t12\t1\t.\t0\t.\t.\t.\tNONE\t.\t.\t." % (cpu.BEG + 241),
           (300, "R"): "J\tchrS\t%d\tR\t10\t8\t2\t0\t2\t0\t%d\t-\tINV\t280\t.\t." % (cpu.BEG + 301, cpu.BEG + 21)}


@pytest.mark.parametrize("with_reads", [0, 1])
def test_store_text_with_junctions_line_for_line(tmp_path, with_reads):
    r, rows, ev, events, jrows = store_input()
    late = events[np.isin(ev[:, 0], (2, 3))].copy()
    late["site"] -= 2
    late_j = jrows[2:].copy()
    late_j[:, cj.W["site"]] -= 2
    with uio.ClipSites(0, 10, 1, with_reads) as s:
        s.set_junctions(3, 8, 2, 500, 7)
        s.add(19, "chrS", rows[2:], late, r, r["qnames"], junctions=late_j)                     # two calls, the later sites first; the mate is an index of its call
        s.add(19, "chrS", rows, events, r, r["qnames"], junctions=jrows)                        # ... the second holds all four: equal site rows keep the first report
        fewer, other = rows[:1].copy(), jrows[:1].copy()
        fewer[0, cr.W["reads"]] -= 1
        other[0, cj.W["status"]], other[0, cj.W["mate"]] = 1, -1
        s.add(19, "chrS", fewer, junctions=other)                                               # a smaller site row loses, and its J line with it
        with pytest.raises(ValueError):
            s.add(19, "chrS", rows, junctions=jrows[:2])
        plain, gz = tmp_path / "c.tsv", tmp_path / "c.tsv.gz"
        s.write(plain)
        s.write(gz)
    base = cr.report_text([(19, "chrS", rows, ev, r)], 0, 10, 1, with_reads).splitlines()
    want = base[:4] + ["##clip_sites_junction_min_votes=3", "##clip_sites_junction_min_len=8", "##clip_sites_junction_max_mismatch=2", "##clip_sites_junction_max_dist=500", "##clip_sites_junction_slop=7"] + base[4:6]
    want.append("#J\tcontig\tpos\tside\tquery_len\tcmp_len\tstatus\tbest_mm\tn_best\tsecond_mm\tpartner_pos\tstrand\tclass\tlen\tmate_pos\tmate_side")
    for line in base[6:]:
        want.append(line)
        f = line.split("\t")
        if f[0] == "S":
            want.append(J_LINES[(int(f[2]) - 1 - cpu.BEG, f[3])])
    # the third J line of the late call has mate -1; the one of site (300, R) is the late call's (it came first): both equal the full call's
    text = plain.read_text()
    assert text.splitlines() == want
    assert sum(l.startswith("J\t") for l in want) == 4 and text.endswith("\n") and gzip.open(gz, "rt").read() == text
    assert text == cj.report_text([(19, "chrS", rows, ev, r)], 0, 10, 1, with_reads, junctions=[jrows], request=(3, 8, 2, 500, 7))


@pytest.mark.parametrize("with_reads", [0, 1])
def test_store_text_with_junctions_off_is_todays(tmp_path, with_reads):
    r, rows, ev, events, jrows = store_input()
    with uio.ClipSites(0, 10, 1, with_reads) as s:                                              # no set_junctions: junction rows change nothing
        s.add(19, "chrS", rows, events, r, r["qnames"], junctions=jrows)
        s.write(tmp_path / "a.tsv")
    with uio.ClipSites(0, 10, 1, with_reads) as s:
        s.add(19, "chrS", rows, events, r, r["qnames"])
        s.write(tmp_path / "b.tsv")
    with uio.ClipSites(0, 10, 1, with_reads) as s:                                              # set_junctions, sites without junction rows: the header lines alone
        s.set_junctions()
        s.add(19, "chrS", rows, events, r, r["qnames"])
        s.write(tmp_path / "c.tsv")
    today = cr.report_text([(19, "chrS", rows, ev, r)], 0, 10, 1, with_reads)
    assert (tmp_path / "a.tsv").read_text() == today == (tmp_path / "b.tsv").read_text() == cj.report_text([(19, "chrS", rows, ev, r)], 0, 10, 1, with_reads)
    c = (tmp_path / "c.tsv").read_text().splitlines()
    assert [l for l in c if not l.startswith(("##clip_sites_junction_", "#J\t"))] == today.splitlines() and len(c) == len(today.splitlines()) + 6
    assert "##clip_sites_junction_min_votes=2" in c and "##clip_sites_junction_min_len=16" in c and "##clip_sites_junction_max_mismatch=1" in c and "##clip_sites_junction_max_dist=0" in c and "##clip_sites_junction_slop=10" in c


# ------------------------------------------------------------------------------------------------ command line
BASE, OUT, run = cpu.BASE, cpu.OUT, cpu.run
ON = ["--clip-sites-junctions", "1"]
J_OPTS = [("--clip-sites-junction-min-len", "16"), ("--clip-sites-junction-max-mismatch", "1"), ("--clip-sites-junction-min-votes", "2"), ("--clip-sites-junction-max-dist", "0"), ("--clip-sites-junction-slop", "10")]


def test_help_lists_the_six_options_with_their_defaults(tmp_path):
    r = run(["--help"], tmp_path)
    assert r.returncode == 0
    for opt, dflt in [("--clip-sites-junctions", "0")] + J_OPTS:
        line = [l for l in r.stdout.splitlines() if l.startswith("  %s " % opt)]
        assert len(line) == 1 and line[0].split()[1] == "[CLI]" and line[0].split()[2] == "default=" + dflt, (opt, line)
    assert "same region" in r.stdout or "only inside the region" in r.stdout


@pytest.mark.parametrize("args,both", [(BASE + ON, ("--clip-sites-junctions", "--clip-sites-out"))]
                         + [(BASE + [g, v], (g, "--clip-sites-out")) for g, v in J_OPTS]
                         + [(BASE + OUT + [g, v], (g, "--clip-sites-junctions")) for g, v in J_OPTS]
                         + [(BASE + OUT + ["--clip-sites-junctions", "0", g, v], (g, "--clip-sites-junctions")) for g, v in J_OPTS[:2]]
                         + [(cpu.PAIR + ON, ("--clip-sites-junctions", "--normal-bam")), (BASE + OUT + ON + ["--shard", "1/2"], ("--clip-sites-out", "--shard"))])
def test_refusals_come_before_any_file_or_device(tmp_path, args, both):
    r = run(args, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert all(w in r.stderr for w in both), r.stderr
    assert "cannot open" not in r.stderr and "no HIP device" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("opt,bad", [("--clip-sites-junctions", b) for b in ("2", "-1", "yes", "0.5", "")]
                         + [("--clip-sites-junction-min-len", b) for b in ("0", "33", "-1", "true", "1.5", "x", "")]
                         + [("--clip-sites-junction-max-mismatch", b) for b in ("-1", "8", "false", "0.5", "x", "")]
                         + [("--clip-sites-junction-min-votes", b) for b in ("0", "-2", "true", "2.5", "x", "", "3e10")]
                         + [("--clip-sites-junction-max-dist", b) for b in ("-1", "1.5", "x", "", "3e10")]
                         + [("--clip-sites-junction-slop", b) for b in ("-1", "0.5", "x", "", "1,2")])
def test_malformed_values_are_refused(tmp_path, opt, bad):
    r = run(BASE + OUT + ON + [opt + "=" + bad], tmp_path)
    assert r.returncode == 2 and opt in r.stderr, (bad, r.stderr)
    assert os.listdir(tmp_path) == []


def test_allowed_companions_get_past_the_option_checks(tmp_path):
    """The options with their report are not refused: the run fails on the missing BAM."""
    r = run(BASE + OUT + ["-R", "p.bed", "--merge-regions", "2000", "--devices", "0", "-t", "2", "--clip-sites-reads", "1", "--clip-sites-junctions", "true", "--clip-sites-junction-min-len", "32", "--clip-sites-junction-max-mismatch", "7",
                          "--clip-sites-junction-min-votes", "1", "--clip-sites-junction-max-dist", "100000", "--clip-sites-junction-slop", "0"], tmp_path)
    assert r.returncode == 2 and "in.bam" in r.stderr and "--clip-sites" not in r.stderr, r.stderr
