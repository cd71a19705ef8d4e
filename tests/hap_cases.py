"""Planted link structures on real reads, beside tests/edge_reads.py::planted_haplotypes (one haplotype, every read the same list): reads
placed by hand (Placer / add_read) on a small background of tests/test_gpu_fuzz.py::weird_region, so that the lists of the fragment and family
passes nest, tie, run over the per-position budget, and cross the quality thresholds of is_var_of_highBQ on both platforms.
tests/test_hap_cpu.py holds the preconditions (each case is what it claims to be, judged on tests/hap_restatement.py) and the oracle against the
restatement; tests/test_gpu_hap.py compares the HIP path with the oracle.

Every case is a dict: reads, placed, platform, and the facts its precondition reads."""
import functools

import numpy as np

from uvc_amd import region
from edge_reads import I, M, Placer
from param_moves import oracle_vcf_text
from test_gpu_fuzz import weird_region

BEG = 1_000_000
READ_LEN = 150
A_OFF, B_OFF, C_OFF = 20, 70, 120            # read offsets of the three SNV sites; the insertion stands directly in front of B
D_OFF, D_QUAL = 140, 10                      # a fourth SNV of low quality on the AB fragments: in their list only once bias_thres_highBQ is moved down


def _plant(P, ref, start, sites, ins=0, qual=37, site_qual=None, reverse=False, dflag=0, same_family=False, mate_of_last=False, length=READ_LEN, shift=1, name="hap"):
    """One alignment of `length` reference bases at region offset `start`: the alternative base (reference + shift) at the read offsets `sites`,
    an insertion of `ins` bases in front of B_OFF, quality `qual` everywhere but `site_qual` = {offset: quality} (offset "ins": the inserted
    bases and both neighbours)."""
    ops = [(M, B_OFF), (I, ins), (M, length - B_OFF)] if ins else [(M, length)]
    i = P.add(name, start, ops, qual=qual, nm=len(sites) + ins, reverse=reverse, dflag=dflag, mate_of_last=mate_of_last)
    r = P.reads
    so = int(r["seq_off"][i])
    q_of = lambda off: off + (ins if off >= B_OFF else 0)
    for off in sites:
        r["bases"][so + q_of(off)] = (ref[start + off] + shift) % 4
    if ins:
        r["bases"][so + B_OFF: so + B_OFF + ins] = (0, 2, 1)[:ins]           # every read inserts the same bases
    for off, q in (site_qual or {}).items():
        if off == "ins":
            r["quals"][so + B_OFF - 1: so + B_OFF + ins + 1] = q
        else:
            r["quals"][so + q_of(off)] = q
    if same_family:                                                            # joins the family of the read before it
        r["fam_id"][i] -= 1; r["n_fams"] -= 1; r["fam_dflag"] = r["fam_dflag"][:-1]; P.fam -= 1
    return i


def _background(seed, ref_len, n_frag=20):
    reads = weird_region(seed, n_frag=n_frag, ref_len=ref_len, beg=BEG)
    ref = np.array(["ACGT".index(c) for c in reads["refseq"]])
    return reads, ref


# (name, sites, insertion, forward, reverse) of the one-read fragments; the fragments of the families below count at the bq level as well.  At
# the default parameters ABiB and ABC tie at the third place (phasing_haplotype_max_detail_cnt 3), the insertion with B alone is over the budget
# of phasing_haplotype_max_count 8 (B was counted nine times before it), AC has two reads (< phasing_haplotype_min_ad + 2), AB has five
# (< 4 + 2: gone once phasing_haplotype_min_ad is 4), and A alone makes no list.
ABC = (A_OFF, B_OFF, C_OFF)
NESTED_GROUPS = (("ABiBC", ABC, 1, 5, 4), ("ABiB", (A_OFF, B_OFF), 1, 4, 4), ("BC", (B_OFF, C_OFF), 0, 4, 3), ("ABC", ABC, 0, 7, 7),
                 ("AB", (A_OFF, B_OFF), 0, 2, 3), ("BiBC", (B_OFF, C_OFF), 1, 3, 2), ("BiB", (B_OFF,), 1, 2, 2), ("AC", (A_OFF, C_OFF), 0, 1, 1), ("A", (A_OFF,), 0, 2, 1))
NESTED_START = 300
# UMI families (dflag 0x3): (insertion, [sites of every fragment]), each once per strand.  One fragment: in fq, not in f2q (fam_thres_dup1add 2).
# Four fragments of which one lacks C: 75 % < fam_thres_dup1perc 80 at C only, so the f2q list is the fq list without C.  Five fragments of
# which one lacks C: 80 %, in f2q until fam_thres_dup1perc is moved to 100.
NESTED_FAMILIES = ((1, [ABC]), (1, [ABC, ABC]), (1, [ABC, ABC]), (0, [(B_OFF, C_OFF)] * 3), (0, [(B_OFF, C_OFF)] * 3), (1, [ABC, ABC, ABC, (A_OFF, B_OFF)]),
                   (1, [ABC, (A_OFF, B_OFF), ABC, ABC]), (1, [ABC] * 4), (1, [ABC, ABC, (A_OFF, B_OFF), ABC, ABC]))


def _nested_reads(seed, snv_qual=37, ins_qual=None):
    """snv_qual: the quality of the SNVs at B and C (A keeps 37); ins_qual: of the inserted base and its neighbours in the ABiB fragments"""
    reads, ref = _background(seed, 1200)
    P = Placer(reads, seed * 10)
    sq = lambda sites, ins: {o: snv_qual for o in sites if o != A_OFF}
    for name, sites, ins, n_fw, n_rv in NESTED_GROUPS:
        for k in range(n_fw + n_rv):
            low = {D_OFF: min(D_QUAL, snv_qual)} if name == "AB" else {"ins": ins_qual} if name == "ABiB" and ins_qual is not None else {}
            _plant(P, ref, NESTED_START, sites + tuple(o for o in low if o != "ins"), ins=ins, site_qual={**sq(sites, ins), **low}, reverse=(k >= n_fw), name=name)
    for ins, members in NESTED_FAMILIES:
        for strand in (0, 1):
            for j, sites in enumerate(members):
                _plant(P, ref, NESTED_START, sites, ins=ins, site_qual=sq(sites, ins), reverse=bool(strand), dflag=0x3, same_family=(j > 0), name="family of %d" % len(members))
    return reads, P


def nested_sites():
    p0 = BEG + NESTED_START
    return dict(A=p0 + A_OFF, B=p0 + B_OFF, C=p0 + C_OFF, D=p0 + D_OFF)


@functools.lru_cache(maxsize=None)
def nested():
    reads, P = _nested_reads(51)
    return dict(reads=reads, placed=P.placed, platform=1, sites=nested_sites())


@functools.lru_cache(maxsize=None)
def iontorrent(platform):
    """The nested reads with the SNVs at B and C at quality 5 and the insertion of the ABiB fragments between bases of quality 2: on Illumina a
    LINK symbol always counts and a base needs con_qual >= bias_thres_highBQ, on Ion Torrent the base always counts and the LINK symbol needs
    con_qual + 3 (families: max(confam_qual + 3, avgBQ)) >= bias_thres_highBQ, which the platform's defaults lower to 7."""
    reads, P = _nested_reads(52, snv_qual=5, ins_qual=2)
    return dict(reads=reads, placed=P.placed, platform=platform, sites=nested_sites())


THRESHOLD_START = 200
THRESHOLD_QUALS = (17, 18, 19, 20, 21, 22)
THRESHOLD_PAIRS = ((37, 18), (37, 17), (30, 11), (30, 10), (41, 21), (41, 22))     # (quality of the SNV in R1, of the other base in R2): 19, 20, 19, 20, 20, 19


@functools.lru_cache(maxsize=None)
def threshold():
    """One haplotype A, B, C with the base quality of A walked across bias_thres_highBQ (20): one-read fragments with A at 17 .. 22, and R1 / R2
    pairs that overlap at A and disagree there, so that con_qual = 2 * con - tot = q1 - q2 lands on 19 and on 20.  Below the threshold the list
    is (B, C), from it on (A, B, C)."""
    reads, ref = _background(53, 900)
    P = Placer(reads, 530)
    for k, q in enumerate(THRESHOLD_QUALS * 2):
        _plant(P, ref, THRESHOLD_START, ABC, site_qual={A_OFF: q}, reverse=(k >= len(THRESHOLD_QUALS)), name="A at %d" % q)
    for k, (q1, q2) in enumerate(THRESHOLD_PAIRS * 2):
        rev = k >= len(THRESHOLD_PAIRS)
        _plant(P, ref, THRESHOLD_START, ABC, site_qual={A_OFF: q1}, reverse=rev, name="R1 A at %d" % q1)
        # R2 begins 10 bases in front of A and carries another alternative base there
        _plant(P, ref, THRESHOLD_START + A_OFF - 10, (10,), site_qual={10: q2}, mate_of_last=True, length=60, shift=2, name="R2 other base at %d" % q2)
    return dict(reads=reads, placed=P.placed, platform=1, site_A=BEG + THRESHOLD_START + A_OFF, want_con_qual=sorted(set(THRESHOLD_QUALS) | {a - b for a, b in THRESHOLD_PAIRS}))


EDGE_LEN = 400


@functools.lru_cache(maxsize=None)
def edges():
    """A haplotype with one SNV on the region's first position and one on the last position a read may cover, on reads as long as the region; at
    either end a fragment of several short alignments that mismatch everywhere and begin or end with an insertion: its bound of mutated symbols
    (mismatching bases + InDel ops) is above twice its span, so the 2 * span clamp of the event slot is in force, and on the right its span
    (which grows by one per alignment) runs over the region's end."""
    reads, ref = _background(54, EDGE_LEN, n_frag=10)
    P = Placer(reads, 540)
    last = EDGE_LEN - 2                                   # a read ends at or before the region's end - 1
    for k in range(8):
        _plant(P, ref, 0, (0, 50, last), reverse=bool(k % 2), length=last + 1, name="edge to edge")
    for k in range(4):
        _plant(P, ref, 0, (0, 50), reverse=bool(k % 2), length=120, name="left part")
        _plant(P, ref, last - 99, (49, 99), reverse=bool(k % 2), length=100, name="right part")
    for side, start in (("left", 0), ("right", last - 2)):
        for j in range(4):
            ops = [(I, 1), (M, 3), (I, 1)]
            i = P.add("%s stack" % side, start, ops, qual=37, nm=5, mate_of_last=(j > 0), stack=side)
            so = int(reads["seq_off"][i])
            reads["bases"][so + 1: so + 4] = (ref[start: start + 3] + 1) % 4
    return dict(reads=reads, placed=P.placed, platform=1, first=BEG, last=BEG + last)


# Moved parameters on `nested`: every move changes the links against the default run (tests/test_hap_cpu.py)
NESTED_MOVES = (("fam_thres_dup1add", 3), ("fam_thres_dup1perc", 100), ("bias_thres_highBQ", 1), ("bias_thres_highBQ", 38), ("phasing_haplotype_max_count", 0),
                ("phasing_haplotype_max_count", 2), ("phasing_haplotype_min_ad", 0), ("phasing_haplotype_min_ad", 4), ("phasing_haplotype_max_detail_cnt", 0),
                ("phasing_haplotype_max_detail_cnt", 1), ("phasing_haplotype_max_detail_cnt", -1))

CASES = {"nested": nested, "threshold": threshold, "iontorrent_as_illumina": lambda: iontorrent(1), "iontorrent": lambda: iontorrent(2), "edges": edges}


# ---- what the tests of both files read from a handle ----
def params_of(lib, platform, setting=None):
    P = region.default_params(lib, platform=platform)
    for k, v in (setting or {}).items():
        assert hasattr(P, k), k
        setattr(P, k, v)
    return P


def oracle_tags(R):
    """{(refpos, symbol): (bHap, cHap, c2Hap)} of the record lines the oracle writes at the default gate ("" where VCF has ".")"""
    out = {}
    for rec in oracle_vcf_text(R):
        fixed, tier2, spec = rec.split("\x1e")
        if tier2 == "-1":              # a position-level line
            continue
        tags = {}
        for line in spec.split("\n"):
            f = line.split("\t")
            if len(f) == 3:
                tags[f[0]] = f[2]
        symbol = int(tags["VTI"].split("\x1f")[1])
        out[(int(fixed.split("\t")[1]) - (1 if symbol <= 5 else 0), symbol)] = (tags["bHap"], tags["cHap"], tags["c2Hap"])
    return out


def product_tags(R):
    """the same from the VCF text of the HIP path (Region.vcf_records of the default-gate records)"""
    out = {}
    for line in R.vcf_records("chrP", R.score()).splitlines():
        c = line.split("\t")
        if c[4].startswith("<N") or c[4].startswith("<ADD"):
            continue
        f = dict(zip(c[8].split(":"), c[9].split(":")))
        symbol = int(f["VTI"].split(",")[1])
        out[(int(c[1]) - (1 if symbol <= 5 else 0), symbol)] = tuple("" if f[k] == "." else f[k] for k in ("bHap", "cHap", "c2Hap"))
    return out
