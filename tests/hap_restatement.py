"""Independent Python restatement, written from the reference text (not from oracle/ and not from uvc_hap.cpp), of the haplotype links
(SURVEY row a12): the list-making rules of the fragment pass (main.hpp:2720-2737) and of the family pass (main.hpp:3491-3521), updateHapMap
(main.hpp:3596-3663), and the phase strings of FORMAT/bHap, cHap, c2Hap (mutform2count4vec_to_simplemut2indices, main.cpp:82-97;
mutform2count4map_to_phase, main.hpp:5380-5404).  Plain Python integers, tuples and dicts.

A list ("mutform", std::basic_string<std::pair<refpos, AlignmentSymbol>>) is a tuple of (position, symbol) tuples.  Python compares tuples
as basic_string::compare does: element by element with the pair's operator<, and a proper prefix is the smaller one.

tests/test_hap_host_cpu.py holds uvc_amd/csrc/uvc_hap.cpp against update_hap_map and phase_string; tests/test_hap_cpu.py holds the oracle's
links and VCF tags against all four."""
import numpy as np

from p2_restatement import update_by_aln
from p3_restatement import fragment_pass
from p45_restatement import family_passes
from prep_restatement import prep_sets, thres_sets
from rtr_cases import python_tracks

SIZE_T = 1 << 64
# SYMBOL_TO_DESC_ARR, main_conversion.hpp:336-346
SYMBOL_TO_DESC_ARR = ("A", "C", "G", "T", "N", "*", "<LR>", "<LD3P>", "<LD2>", "<LD1>", "<LI3P>", "<LI2>", "<LI1>", "*")
BASE_NN = 5


def lists_to_map(per_object, pick):
    """mutform2count4map of main.hpp:2734-2737 / 3514-3521: per_object = [(strand, [(epos, symbol, ...), ...])] as the restated passes hand them
    out; the entries `pick` keeps make the object's pos_symbol_string, which counts once for its strand when it has more than one pair."""
    out = {}
    for strand, entries in per_object:
        form = tuple((int(e[0]), int(e[1])) for e in entries if pick(e))
        if len(form) > 1:
            out.setdefault(form, [0, 0])[strand] += 1
    return out


def chain(reads, P, platform=1, is_normal=False):
    """The restated inputs of the two passes for one region (tracks, prep, thresholds, P2), as tests/test_p3_cpu.py chains them."""
    rtr, baq = python_tracks(reads["refseq"], smax=P.indel_str_repeatsize_max, vmax=P.indel_vntr_repeatsize_max, bq_max=P.indel_BQ_max,
                             slip_rate=P.indel_polymerase_slip_rate, del_to_ins=P.indel_del_to_ins_err_ratio, polymerase_size=P.indel_polymerase_size,
                             str_phred_per_region=P.indel_str_phred_per_region, nonstr_phred_per_base=P.indel_nonSTR_phred_per_base)
    codes = np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(c.upper(), 4) for c in reads["refseq"]], dtype=np.int32)
    prep = prep_sets(reads, P, rtr, baq[0], np.append(codes, 4))
    proton = (platform == 2)
    thres, ip = thres_sets(prep, rtr[3], P, is_normal=is_normal, iontorrent=proton)
    return dict(rtr=rtr, baq=baq, codes=codes, prep=prep, thres=thres, ip=ip, proton=proton)


def fragment_objects(reads, P, ch):
    """[(strand, [(epos, con_symbol, con_qual, is_var_of_highBQ)])] per fragment: handed out by p3_restatement.fragment_pass, not computed a
    second time."""
    seg, bqsum = update_by_aln(reads, P, ch["rtr"], ch["ip"], ch["baq"][0], ch["baq"][1], ch["codes"], ch["prep"], ch["thres"], ch["proton"])
    haps = []
    fragment_pass(reads, P, ch["rtr"], ch["ip"], ch["baq"][0], ch["codes"], ch["prep"], ch["thres"], seg, bqsum, ch["proton"], haps=haps)
    return haps


def family_objects(reads, P, ch):
    """[(strand, [(epos, con_symbol, confam_qual, avgBQ, is_var_of_highBQ, in_f2q)])] per family-strand unit: handed out by
    p45_restatement.family_passes."""
    haps = []
    family_passes(reads, P, ch["rtr"], ch["ip"], ch["baq"][0], ch["baq"][1], ch["codes"], ch["prep"], ch["thres"], ch["proton"], haps=haps)
    return haps


def fragment_lists(fragments):
    """mutform2count4map_bq (main.hpp:2720-2737): {list: [forward, reverse]} over fragment_objects()."""
    return lists_to_map(fragments, pick=lambda e: e[3])


def family_lists(units):
    """(mutform2count4map_fq, mutform2count4map_f2q) of main.hpp:3491-3521 over family_objects(): the f2q list of a unit is the sub-list of
    its fq list at the positions where the unit's own consensus passes fam_thres_dup1add / fam_thres_dup1perc."""
    return lists_to_map(units, pick=lambda e: e[4]), lists_to_map(units, pick=lambda e: e[5])


def update_hap_map(counts_by_list, max_count, min_ad, max_detail_cnt, stats=None):
    """updateHapMap, main.hpp:3604-3662 -> [(list, (forward, reverse), (other forward, other reverse))].
    stats (optional dict) gains what the case generators of tests/test_hap_host_cpu.py count: ties, subsets, budget drops."""
    ret = []
    # 3606-3611: (total, list, [forward, reverse]) rows, std::sort over reverse iterators = descending
    rows = [(int(c[0]) + int(c[1]), form, (int(c[0]), int(c[1]))) for form, c in counts_by_list.items()]
    rows.sort(reverse=True)
    num_dst = min(int(max_detail_cnt) % SIZE_T, len(rows))                        # 3613: MIN((size_t)phasing_haplotype_max_detail_cnt, size)
    inc_fw, inc_rv = [0] * num_dst, [0] * num_dst
    for i in range(num_dst):                                                       # 3621-3641
        dst = rows[i][1]
        for j in range(i + 1, len(rows)):
            src = rows[j][1]
            if all(allele in src for allele in dst):                               # src_mutform.find(dst_allele) != npos for every allele
                inc_fw[i] += rows[j][2][0]; inc_rv[i] += rows[j][2][1]
    tsum = {}                                                                      # 3642: a fresh per-position counter over the region
    n_budget = 0
    for i, (tot, form, counts) in enumerate(rows):                                 # 3643-3661
        if counts[0] + counts[1] < min_ad + len(form):
            continue
        haplo_totDP = 0
        for pos, _symbol in form:
            tsum[pos] = tsum.get(pos, 0) + 1                                       # raised before the max_count test
            haplo_totDP += tsum[pos]
        if haplo_totDP > max_count * len(form):
            n_budget += 1
            continue
        ret.append((form, counts, (-1, -1) if i >= num_dst else (inc_fw[i], inc_rv[i])))
    if stats is not None:
        stats["tie_at_boundary"] = 0 < num_dst < len(rows) and rows[num_dst - 1][0] == rows[num_dst][0]
        stats["ties"] = any(a[0] == b[0] for a, b in zip(rows, rows[1:]))
        stats["subsets"] = any(inc_fw[i] + inc_rv[i] > 0 for i in range(num_dst))
        stats["budget_drops"] = n_budget
        stats["min_ad_drops"] = sum(1 for tot, form, c in rows if tot < min_ad + len(form))
    return ret


def phase_string(links, pos, symbol):
    """The FORMAT string of the record (pos, symbol): the links of mutform2count4vec_to_simplemut2indices (main.cpp:82-97) in index order through
    mutform2count4map_to_phase (main.hpp:5380-5404, pseudocount 1)."""
    indices = []
    for i, (form, counts, other) in enumerate(links):                              # main.cpp:87-95
        if counts[0] + counts[1] < 2:
            continue
        if (pos, symbol) in form:
            indices.append(i)
    out = ""
    for i in indices:                                                              # main.hpp:5387-5402
        form, counts, other = links[i]
        if counts[0] + counts[1] > 1:
            out += "("
            for p, s in form:
                mutpos = p + (1 if s <= BASE_NN else 0)                            # isSymbolSubstitution
                out += "(" + str(mutpos) + "&" + SYMBOL_TO_DESC_ARR[s] + ")"
            add = ("&&" + str(other[0] + counts[0]) + "&" + str(other[1] + counts[1])) if -1 < other[0] else ""
            out += "&" + str(counts[0]) + "&" + str(counts[1]) + add + ")"
    return out


def region_links(reads, P, platform=1, is_normal=False, objects=None):
    """The three link vectors of one region (bq, fq, f2q) from the restated lists, in the form Region.hap_links() returns.
    objects (optional dict) gains "fragments" and "units"."""
    ch = chain(reads, P, platform, is_normal)
    frs, units = fragment_objects(reads, P, ch), family_objects(reads, P, ch)
    if objects is not None:
        objects["fragments"], objects["units"] = frs, units
    fq, f2q = family_lists(units)
    a = (int(P.phasing_haplotype_max_count), int(P.phasing_haplotype_min_ad), int(P.phasing_haplotype_max_detail_cnt))
    return [update_hap_map(m, *a) for m in (fragment_lists(frs), fq, f2q)]
