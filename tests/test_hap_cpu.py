"""The haplotype links without a GPU: the oracle's link vectors (Region.hap_links) and the bHap / cHap / c2Hap values of its VCF
lines against tests/hap_restatement.py chained behind the restatements of the tracks, P1, P2, P3 and P4 / P5 -- no oracle value enters the
chain -- on the planted cases of tests/hap_cases.py, the three HAP_CASES of tests/test_vcf_text.py and planted_haplotypes of
tests/edge_reads.py.  Every planted case asserts first, on the restatement alone, that it is the case it claims to be."""
import functools

import pytest

from uvc_amd import synth
import edge_reads as er
import hap_cases as hc
import hap_restatement as hr
from hap_cases import oracle_tags, params_of
from test_vcf_text import HAP_CASES
from util import run_region

LEVELS = ("bq", "fq", "f2q")
LIST_PARAMS = ("fam_thres_dup1add", "fam_thres_dup1perc", "bias_thres_highBQ")      # what the lists depend on; the phasing_haplotype_* only enter update_hap_map


_objects = {}


def restated(lib, key, reads, platform, setting=None):
    """-> (links x 3, maps x 3, objects) of the restatement; the restated passes run once per (case, list parameters)."""
    P = params_of(lib, platform, setting)
    okey = (key, platform) + tuple(int(getattr(P, k)) for k in LIST_PARAMS)
    if okey not in _objects:
        ch = hr.chain(reads, P, platform)
        _objects[okey] = dict(fragments=hr.fragment_objects(reads, P, ch), units=hr.family_objects(reads, P, ch))
    obj = _objects[okey]
    fq, f2q = hr.family_lists(obj["units"])
    maps = [hr.fragment_lists(obj["fragments"]), fq, f2q]
    a = (int(P.phasing_haplotype_max_count), int(P.phasing_haplotype_min_ad), int(P.phasing_haplotype_max_detail_cnt))
    return [hr.update_hap_map(m, *a) for m in maps], maps, obj


def check_against_oracle(lib, key, reads, platform=1, setting=None, min_links=1):
    want, maps, obj = restated(lib, key, reads, platform, setting)
    R = run_region(lib, reads, params=params_of(lib, platform, setting))
    try:
        got = R.hap_links()
        for w, name in enumerate(LEVELS):
            assert got[w] == want[w], (key, setting, name, next((a, b) for a, b in zip(got[w] + [None], want[w] + [None]) if a != b))
        tags = oracle_tags(R)
    finally:
        R.close()
    n_linked = 0
    for (pos, symbol), values in tags.items():
        for w, name in enumerate(LEVELS):
            assert values[w] == hr.phase_string(want[w], pos, symbol), (key, setting, name, pos, symbol)
        n_linked += values[0] != ""
    assert sum(len(l) for l in want) >= min_links and (min_links == 0 or n_linked > 0), (key, setting, [len(l) for l in want], n_linked)
    return want, maps, obj


# ---- the generated inputs that have links already ----
@pytest.mark.parametrize("name", list(HAP_CASES))
def test_generated_regions(name, oracle_lib):
    kw = dict(HAP_CASES[name])
    kw["region_len"] = min(kw["region_len"], 1500)         # the same generators on a shorter region: the Python restatement of P2 .. P5 walks every base
    kw["depth"] = min(kw["depth"], 120)
    check_against_oracle(oracle_lib, name, synth.generate_region(**kw), min_links=3)


def test_planted_haplotypes(oracle_lib):
    check_against_oracle(oracle_lib, "planted_haplotypes", er.planted_haplotypes()["reads"], min_links=3)


# ---- the planted cases ----
NESTED_FORMS = {"ABiBC": ("A", "Bi", "B", "C"), "ABiB": ("A", "Bi", "B"), "BC": ("B", "C"), "ABC": ("A", "B", "C"), "AB": ("A", "B"), "BiBC": ("Bi", "B", "C"),
                "BiB": ("Bi", "B"), "AC": ("A", "C")}


def form_of(sites, names, maps_level):
    """the list of the planted sites `names` (e.g. "A", "Bi", "B", "C") as it stands in a map: the symbols are read from the map itself"""
    pos = [sites[n[0]] for n in names]
    for form in maps_level:
        if [p for p, s in form] == pos and all((s > 5) == (len(n) == 2) for (p, s), n in zip(form, names)):
            return form
    return None


def test_nested_is_what_it_claims_and_matches_the_oracle(oracle_lib):
    case = hc.nested()
    want, maps, obj = check_against_oracle(oracle_lib, "nested", case["reads"], min_links=8)
    S = case["sites"]
    bq = maps[0]
    f = {n: form_of(S, names, bq) for n, names in NESTED_FORMS.items()}
    assert all(v is not None for v in f.values()), f
    st = {}
    links = hr.update_hap_map(bq, 8, 1, 3, stats=st)
    written = {l[0]: l for l in links}
    assert st["tie_at_boundary"]                                                   # two lists tie in total at the third place ...
    rows = sorted(((sum(c), form) for form, c in bq.items()), reverse=True)
    assert {rows[2][1], rows[3][1]} == {f["ABiB"], f["ABC"]} and rows[2][1] == f["ABiB"]
    assert written[f["ABiB"]][2] != (-1, -1) and written[f["ABC"]][2] == (-1, -1)    # ... and the list order decides which one is detailed
    assert sum(bq[f["BiB"]]) >= 1 + 2 and f["BiB"] not in written and st["budget_drops"] >= 1      # dropped by phasing_haplotype_max_count
    assert f["BiB"] in {l[0] for l in hr.update_hap_map(bq, 100, 1, 3)}
    assert sum(bq[f["AC"]]) == 2 and f["AC"] not in written                         # fails phasing_haplotype_min_ad
    assert f["AC"] in {l[0] for l in hr.update_hap_map(bq, 8, 0, 3)}
    assert any(o[0] > 0 for form, fr, o in links if o != (-1, -1))                  # "other" support from the lists that contain a detailed one
    # families: one fragment -> fq only; 3 of 4 fragments at C -> the f2q list is the fq list without C
    units = [u for u in obj["units"] if any(e[0] == S["B"] for e in u[1])]
    n_sub = n_fq_only = 0
    for strand, entries in units:
        fq = [e[:2] for e in entries if e[4]]; f2q = [e[:2] for e in entries if e[5]]
        if len(fq) >= 2 and not f2q:
            n_fq_only += 1
        if f2q and f2q != fq:
            assert [e for e in fq if e[0] != S["C"]] == f2q, (fq, f2q)
            n_sub += 1
    assert n_fq_only >= 2 and n_sub == 4, (n_fq_only, n_sub)
    assert want[1] != want[2] and len(want[2]) >= 2


def test_threshold_con_qual_lands_on_both_sides(oracle_lib):
    case = hc.threshold()
    want, maps, obj = check_against_oracle(oracle_lib, "threshold", case["reads"], min_links=2)
    at_A = [(e[2], e[3]) for strand, entries in obj["fragments"] for e in entries if e[0] == case["site_A"]]
    quals = sorted({q for q, high in at_A})
    assert set(case["want_con_qual"]) <= set(quals), (quals, case["want_con_qual"])
    assert all(high == (q >= 20) for q, high in at_A)
    n19, n20 = sum(q == 19 for q, _ in at_A), sum(q == 20 for q, _ in at_A)
    assert n19 >= 8 and n20 >= 8, (n19, n20)                                        # one-read fragments and R1 / R2 pairs on both sides, both strands
    with_A = sum(sum(c) for form, c in maps[0].items() if any(p == case["site_A"] for p, s in form) and sum(c) > 1)
    without = sum(sum(c) for form, c in maps[0].items() if all(p != case["site_A"] for p, s in form) and sum(c) > 1)
    assert with_A >= 10 and without >= 10, (with_A, without)


def test_iontorrent_and_illumina_differ_at_both_levels(oracle_lib):
    res = {}
    for platform in (1, 2):
        case = hc.iontorrent(platform)
        res[platform] = check_against_oracle(oracle_lib, "iontorrent", case["reads"], platform=platform, min_links=1)
    S = hc.nested_sites()
    for w in (0, 1):
        a, b = res[1][1][w], res[2][1][w]
        planted = lambda m: {form: c for form, c in m.items() if sum(c) > 1 and all(p in S.values() for p, s in form)}
        assert planted(a) != planted(b) and planted(a) and planted(b), (w, planted(a), planted(b))
        assert res[1][0][w] != res[2][0][w]
    # Illumina keeps the insertion whatever its quality and no base of quality 5; Ion Torrent keeps every base and the insertion only where
    # con_qual + 3 >= bias_thres_highBQ (7 with the platform's defaults)
    assert all(s > 5 or p == S["A"] for form, c in res[1][1][0].items() if sum(c) > 1 for p, s in form if p in S.values())
    assert any(s <= 5 and p == S["C"] for form in res[2][1][0] for p, s in form)
    for platform in (1, 2):
        ins = [e for strand, entries in res[platform][2]["fragments"] for e in entries if e[0] == S["B"] and e[1] > 5]
        low, high = [e for e in ins if e[2] + 3 < 7], [e for e in ins if e[2] + 3 >= 7]
        assert len(low) == 8 and len(high) > 20, (platform, len(low), len(high))       # the eight ABiB fragments carry the low-quality insertion
        assert all(e[3] for e in high) and all(e[3] == (platform == 1) for e in low)
    units = [e for strand, entries in res[2][2]["units"] for e in entries if e[0] == S["B"] and e[1] > 5]
    assert units and all(e[4] == (max(e[2] + 3, e[3]) >= 7) for e in units)


def test_edges_first_and_last_position_and_the_clamped_slots(oracle_lib):
    case = hc.edges()
    want, maps, obj = check_against_oracle(oracle_lib, "edges", case["reads"], min_links=2)
    reads = case["reads"]
    assert case["first"] == reads["beg"] and case["last"] == reads["end"] - 2
    both = [l for l in want[0] if l[0][0][0] == case["first"] and l[0][-1][0] == case["last"]]
    assert both and sum(both[0][1]) >= 8
    for side in ("left", "right"):                                                  # the bound of k_hap_cand (mismatching bases + InDel ops) against 2 * span
        stack = [p for p in case["placed"] if p.get("stack") == side]
        bound = sum(3 + 2 for p in stack)
        beg = min(p["pos"] for p in stack)
        end = min(max(p["pos"] + 3 for p in stack) + len(stack), reads["end"])      # the end grows by one per alignment, clamped to the region
        assert len(stack) == 4 and bound > 2 * (end - beg), (side, bound, end - beg)
        if side == "right":
            assert max(p["pos"] + 3 for p in stack) + len(stack) > reads["end"]
    spans = [[e[0] for e in entries] for strand, entries in obj["fragments"]]       # the stacks' own lists: three SNVs at either end (an insertion at a read's end is no event)
    assert [case["first"] + k for k in range(3)] in spans and [case["last"] - 2 + k for k in range(3)] in spans


# ---- moved parameters on `nested` ----
@functools.lru_cache(maxsize=None)
def _default_links(lib):
    return restated(lib, "nested", hc.nested()["reads"], 1)[0]


@pytest.mark.parametrize("param,value", hc.NESTED_MOVES)
def test_moved_parameters_change_the_links_and_match_the_oracle(param, value, oracle_lib):
    want, maps, obj = check_against_oracle(oracle_lib, "nested", hc.nested()["reads"], setting={param: value}, min_links=0)
    assert want != _default_links(oracle_lib), (param, value)
    if param == "phasing_haplotype_max_detail_cnt" and value == -1:
        assert all(l[2] != (-1, -1) for links in want for l in links) and sum(len(l) for l in want) > 9       # the size_t cast: every link detailed
    if param == "phasing_haplotype_max_count" and value == 0:
        assert want == [[], [], []]
