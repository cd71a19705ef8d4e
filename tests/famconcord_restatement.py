"""Independent Python restatement of uvcgpu_region_family_concordance, written from the contract in include/uvcgpu.h (not from the kernels):
the votes con_u(p) of every family-strand unit come from the restated family pass (tests/p45_restatement.py: fragment_cov ->
update_by_filtering with thresholds (fam_thres_highBQ_snv, 0)), the row is tallied from them sentence by sentence.

The offsets below are the header's numbers; tests/test_famconcord_cpu.py holds them against include/uvc_famconcord.def."""
import numpy as np

from p2_restatement import read_events
from p3_restatement import BASE_A, BASE_NN, BASE_T, LINK_M, LINK_NN, fill_consensus
from p45_restatement import Cov, families, fragment_cov, update_by_filtering

NBIN, NBASE, NLINK = 8, 6, 8
BASE, BASE_POS, LINK, LINK_POS, DUP_BASE, DUP_LINK, COUNTERS, ROW = 0, 576, 608, 1120, 1136, 1332, 1413, 1429
SECTIONS = [("base", BASE, 2 * NBIN * NBASE * NBASE), ("base_pos", BASE_POS, 2 * NBIN * 2), ("link", LINK, NBIN * NLINK * NLINK), ("link_pos", LINK_POS, NBIN * 2),
            ("dup_base", DUP_BASE, 4 * (NBASE + 1) * (NBASE + 1)), ("dup_link", DUP_LINK, (NLINK + 1) * (NLINK + 1)), ("counters", COUNTERS, 16)]
COUNTER_NAMES = ["units_seen", "unit_positions", "base_no_vote", "link_no_vote", "base_no_ref", "duplex_no_vote", "duplex_base_no_ref"]
C = {n: COUNTERS + i for i, n in enumerate(COUNTER_NAMES)}
BIN_EDGES = [1, 2, 3, 4, 5, 8, 16, 32]          # the smallest vote total of each bin


def depth_bin(ct):
    return max(k for k, lo in enumerate(BIN_EDGES) if ct >= lo)


def base_cell(refclass, k, cs, s): return BASE + ((refclass * NBIN + k) * NBASE + cs) * NBASE + s
def base_pos_cell(refclass, k, j): return BASE_POS + (refclass * NBIN + k) * 2 + j
def link_cell(k, cs, s): return LINK + (k * NLINK + (cs - LINK_M)) * NLINK + (s - LINK_M)
def link_pos_cell(k, j): return LINK_POS + k * 2 + j
def dup_base_cell(ref, v0, v1): return DUP_BASE + (ref * (NBASE + 1) + v0) * (NBASE + 1) + v1
def dup_link_cell(v0, v1): return DUP_LINK + v0 * (NLINK + 1) + v1


def unit_votes(reads, frs, P, rtr, ip, baq, codes, prep, thres, proton, region_end):
    """One unit (its fragments as lists of read indices) -> (beg, end, con): the span as the family pass walks it, clamped to the region, and
    the vote counts con.c[p - con.beg][symbol]."""
    b, e = 2 ** 31 - 1, 0
    for fr in frs:
        for k in fr:
            _, aln, *_ = read_events(reads, k, P, rtr, ip, baq, codes, prep, thres, proton, with_bias=False)
            b = min(b, int(reads["pos"][k])); e = max(e, aln["endpos"]) + 1
    padded_ignored = bool(int(P.microadjust_padded_deletion_flag) & (0x2 if proton else 0x1))
    con = Cov(b, e)
    for fr in frs:
        update_by_filtering(con, fragment_cov(reads, fr, P, rtr, ip, baq, codes, prep, thres, proton), (int(P.fam_thres_highBQ_snv), 0), padded_ignored, True)
    return b, min(e, region_end), con


def all_unit_votes(reads, P, rtr, ip, baq, codes, prep, thres, proton):
    """[(fam, dflag, {strand: (beg, end, con)})] in read order: the expensive part, shared by every range list of one input."""
    region_end = int(reads["end"]) + 1
    out = []
    for fam, units in families(reads):
        out.append((fam, int(reads["fam_dflag"][fam]),
                    {st: unit_votes(reads, frs, P, rtr, ip, baq, codes, prep, thres, proton, region_end) for st, frs in units.items() if frs}))
    return out


def concordance_row(reads, votes, P, codes, proton, ranges):
    """The row of `ranges` ((pos_beg, pos_end) pairs) from all_unit_votes' result.  codes: the reference symbols of [beg, end)."""
    beg = int(reads["beg"])
    row = np.zeros(ROW, dtype=np.int64)
    padded_ignored = bool(int(P.microadjust_padded_deletion_flag) & (0x2 if proton else 0x1))
    inside = np.zeros(int(reads["end"]) + 1 - beg, dtype=bool)
    for a, b in ranges:
        inside[a - beg:b - beg] = True

    def ref_of(p):                               # None: no reference symbol, or not A/C/G/T
        x = p - beg
        return int(codes[x]) if x < len(codes) and int(codes[x]) <= BASE_T else None

    for fam, dflag, units in votes:
        for strand, (ub, ue, con) in units.items():
            for p in range(ub, ue):
                if not inside[p - beg]:
                    continue
                row[C["unit_positions"]] += 1
                if p == ub:
                    row[C["units_seen"]] += 1
                v = con.c[p - con.beg]
                cs, cc, ct = fill_consensus(v, BASE_A, BASE_NN, False)
                if ct == 0:
                    row[C["base_no_vote"]] += 1
                elif ref_of(p) is None:
                    row[C["base_no_ref"]] += 1
                else:
                    k, rc = depth_bin(ct), (0 if cs == ref_of(p) else 1)
                    for s in range(BASE_A, BASE_NN + 1):
                        row[base_cell(rc, k, cs, s)] += int(v[s])
                    row[base_pos_cell(rc, k, 0)] += 1
                    if cc == ct:
                        row[base_pos_cell(rc, k, 1)] += 1
                cs, cc, ct = fill_consensus(v, LINK_M, LINK_NN, False)
                if ct == 0:
                    row[C["link_no_vote"]] += 1
                else:
                    k = depth_bin(ct)
                    for s in range(LINK_M, LINK_NN + 1):
                        row[link_cell(k, cs, s)] += int(v[s])
                    row[link_pos_cell(k, 0)] += 1
                    if cc == ct:
                        row[link_pos_cell(k, 1)] += 1
        if (dflag & 0x2) and 0 in units and 1 in units:
            lo, hi = min(units[0][0], units[1][0]), max(units[0][1], units[1][1])
            for p in range(lo, hi):
                if not inside[p - beg]:
                    continue
                vb, vl = [NBASE, NBASE], [NLINK, NLINK]          # none
                for j in (0, 1):
                    ub, ue, con = units[j]
                    if not ub <= p < ue:
                        continue
                    v = con.c[p - con.beg]
                    cs, cc, ct = fill_consensus(v, BASE_A, BASE_T if padded_ignored else BASE_NN, False)
                    if max(2 * cc, ct) - ct >= 1:
                        vb[j] = cs - BASE_A
                    cs, cc, ct = fill_consensus(v, LINK_M, LINK_NN, False)
                    if max(2 * cc, ct) - ct >= 1:
                        vl[j] = cs - LINK_M
                if vb == [NBASE, NBASE]:
                    row[C["duplex_no_vote"]] += 1
                elif ref_of(p) is None:
                    row[C["duplex_base_no_ref"]] += 1
                else:
                    row[dup_base_cell(ref_of(p), vb[0], vb[1])] += 1
                if vl == [NLINK, NLINK]:
                    row[C["duplex_no_vote"]] += 1
                else:
                    row[dup_link_cell(vl[0], vl[1])] += 1
    return row


def restated_inputs(reads, P, platform, is_normal=False):
    """The tracks, the read preparation and the thresholds the way tests/test_p45_cpu.py gets them -> kwargs of all_unit_votes."""
    from prep_restatement import prep_sets, thres_sets
    from rtr_cases import python_tracks
    rtr, baq = python_tracks(reads["refseq"], smax=P.indel_str_repeatsize_max, vmax=P.indel_vntr_repeatsize_max, bq_max=P.indel_BQ_max,
                             slip_rate=P.indel_polymerase_slip_rate, del_to_ins=P.indel_del_to_ins_err_ratio, polymerase_size=P.indel_polymerase_size,
                             str_phred_per_region=P.indel_str_phred_per_region, nonstr_phred_per_base=P.indel_nonSTR_phred_per_base)
    codes = np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(c.upper(), 4) for c in reads["refseq"]], dtype=np.int32)
    prep = prep_sets(reads, P, rtr, baq[0], np.append(codes, 4))
    thres, ip = thres_sets(prep, rtr[3], P, is_normal=is_normal, iontorrent=(platform == 2))
    return dict(rtr=rtr, ip=ip, baq=baq[0], codes=codes, prep=prep, thres=thres, proton=(platform == 2))


def restate(reads, P, platform, range_lists):
    """-> [row of every range list]; the votes are evaluated once."""
    kw = restated_inputs(reads, P, platform)
    votes = all_unit_votes(reads, P, **kw)
    return [concordance_row(reads, votes, P, kw["codes"], kw["proton"], ranges) for ranges in range_lists]
