"""uvc_amd/csrc/uvc_hap.cpp (the host half of the haplotype links: hash table over raw event words, partial sort, second sort of the rows
that pass min_ad, position budget) against tests/hap_restatement.py (updateHapMap and the phase strings once more, from the reference text).
tests/native/hap_host_main.cpp is built with the undefined-behaviour and address sanitizers as a stand-alone program and fed event buffers in
the device's format (uvc_hap.h) written by the encoder below; nothing is loaded into Python.

Every constructed case asserts first, on the restatement alone, that it is the case it claims to be."""
import os
import subprocess

import numpy as np
import pytest

from hap_restatement import phase_string, update_hap_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_, C_, G_, T_, D1, I1 = 0, 1, 2, 3, 9, 12
BEG, NPOS = 1000, 200
DEFAULTS = dict(max_count=8, min_ad=1, max_detail_cnt=3)


@pytest.fixture(scope="module")
def hap_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hap_host") / "hap_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "hap_host_main.cpp"), os.path.join(ROOT, "uvc_amd", "csrc", "uvc_hap.cpp")])
    return exe


# ---- the device format ----
def encode(maps, rng, beg=BEG, extra=()):
    """maps = [{list: [forward, reverse]}] x 3 (bq, fq, f2q) -> the event words.  One slot per object (fragment or unit): [strand | kind << 1 |
    slot_len << 8, count, words x slot_len].  Slots are longer than their counts (the rest holds words the host must not read as events), the
    three kinds come interleaved in arbitrary order, lists of count 0 and 1 are mixed in (`extra` = [(kind, strand, list)] plus generated
    ones), and an untouched tail of -1 words follows."""
    objs = [(kind, strand, form) for kind in range(3) for form, fr in maps[kind].items() for strand in (0, 1) for _ in range(fr[strand])]
    objs += list(extra)
    for _ in range(int(rng.integers(0, 4))):
        objs.append((int(rng.integers(0, 3)), int(rng.integers(0, 2)), ()))
    order = rng.permutation(len(objs)) if objs else []
    words = []
    for i in order:
        kind, strand, form = objs[i]
        slot_len = len(form) + int(rng.integers(0, 4))
        words += [strand | (kind << 1) | (slot_len << 8), len(form)]
        words += [((p - beg) << 4) | s for p, s in form]
        words += [int(rng.integers(0, NPOS) << 4) | int(rng.integers(0, 14)) for _ in range(slot_len - len(form))]
    return words + [-1] * int(rng.integers(0, 7))


def singles(rng, n=3):
    """lists of one event: never in a map (pos_symbol_string.size() > 1), but their (position, symbol) is asked for a string"""
    return [(int(rng.integers(0, 3)), int(rng.integers(0, 2)), ((BEG + int(rng.integers(0, NPOS)), int(rng.integers(0, 4))),)) for _ in range(n)]


def write_cases(path, cases):
    with open(path, "w") as fh:
        fh.write("%d\n" % len(cases))
        for c in cases:
            fh.write("%d %d %d %d %d %d\n" % (c["beg"], c["npos"], c["max_count"], c["min_ad"], c["max_detail_cnt"], len(c["words"])))
            fh.write(" ".join(map(str, c["words"])) + "\n")


def run_host(exe, path):
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-4000:]
    out, cur = [], None
    for line in r.stdout.splitlines():
        f = line.split(" ")
        if f[0] == "case":
            cur = dict(links=[[], [], []], strings={})
        elif f[0] == "L":
            v = list(map(int, f[1:]))
            n = v[5]
            assert len(v) == 6 + 2 * n
            cur["links"][v[0]].append((tuple((v[6 + 2 * k], v[7 + 2 * k]) for k in range(n)), (v[1], v[2]), (v[3], v[4])))
        elif f[0] == "S":
            cur["strings"][(int(f[1]), int(f[2]), int(f[3]))] = f[4]
        elif f[0] == "end":
            out.append(cur); cur = None
    return out


def seen_of(case):
    """every (position, symbol) of every slot, as tests/native/hap_host_main.cpp collects them"""
    w, at, seen = case["words"], 0, set()
    while at + 2 <= len(w) and w[at] >= 0:
        for k in range(w[at + 1]):
            seen.add((case["beg"] + (w[at + 2 + k] >> 4), w[at + 2 + k] & 15))
        at += 2 + (w[at] >> 8)
    return seen


def expect(case, stats=None):
    links = [update_hap_map(case["maps"][k], case["max_count"], case["min_ad"], case["max_detail_cnt"], stats=(stats[k] if stats else None)) for k in range(3)]
    strings = {}
    for k in range(3):
        for pos, sym in seen_of(case):
            s = phase_string(links[k], pos, sym)
            if s:
                strings[(k, pos, sym)] = s
    return dict(links=links, strings=strings)


def make(maps, rng, extra=(), **kw):
    p = dict(DEFAULTS, **kw)
    if isinstance(maps, dict):
        maps = [maps, {}, {}]
    return dict(beg=BEG, npos=NPOS, maps=maps, words=encode(maps, rng, extra=extra), **p)


def check(exe, tmp_path, cases, what=""):
    path = str(tmp_path / "cases.txt")
    write_cases(path, cases)
    got = run_host(exe, path)
    assert len(got) == len(cases)
    for i, (c, g) in enumerate(zip(cases, got)):
        w = expect(c)
        for k in range(3):
            assert g["links"][k] == w["links"][k], (what, i, c.get("name"), k, {q: c[q] for q in DEFAULTS}, c["maps"][k], g["links"][k], w["links"][k])
        assert g["strings"] == w["strings"], (what, i, c.get("name"), {q: c[q] for q in DEFAULTS})


def P(x): return BEG + x


def by_form(links):
    return {l[0]: l for l in links}


# ---- constructed cases ----
def test_ties_at_the_detail_boundary_are_decided_by_the_list_order(hap_host, tmp_path):
    rng = np.random.default_rng(1)
    top = ((P(5), A_), (P(9), C_))
    tied = [((P(10), A_), (P(20), C_)),                       # differs in the first position
            ((P(12), A_), (P(20), C_)),
            ((P(12), A_), (P(20), G_)),                       # in a symbol
            ((P(12), A_), (P(20), G_), (P(30), T_))]          # and a list behind its own proper prefix
    m = {top: [5, 4]}
    for k, f in enumerate(tied):
        m[f] = [k + 1, 4 - k]                                 # four lists of total 5, every strand split different
    want = update_hap_map(m, 8, 1, 3)
    got = by_form(want)
    assert len(want) == 5 and [l[0] for l in want] == [top] + sorted(tied, reverse=True)
    detailed = [l[0] for l in want if l[2] != (-1, -1)]
    assert detailed == [top, tied[3], tied[2]] and got[tied[0]][2] == got[tied[1]][2] == (-1, -1)
    assert [got[f][1] for f in tied] == [(1, 4), (2, 3), (3, 2), (4, 1)]
    assert got[tied[2]][2] == (0, 0) and got[tied[3]][2] == (0, 0)          # the prefix sorts behind the longer list and does not contain it
    check(hap_host, tmp_path, [make(m, rng), make([m, m, {}], rng), make([{}, m, m], rng)])


def test_equal_totals_with_different_strand_splits(hap_host, tmp_path):
    rng = np.random.default_rng(2)
    forms = [((P(3), A_), (P(4 + k), C_)) for k in range(5)]
    m = {f: fr for f, fr in zip(forms, ([4, 0], [0, 4], [2, 2], [3, 1], [1, 3]))}
    want = update_hap_map(m, 8, 1, 2)
    assert [l[0] for l in want] == forms[::-1] and [l[1] for l in want] == [(1, 3), (3, 1), (2, 2), (0, 4), (4, 0)]
    assert [l[2] != (-1, -1) for l in want] == [True, True, False, False, False]
    check(hap_host, tmp_path, [make(m, rng, max_detail_cnt=2)])


def test_a_list_and_its_proper_prefix(hap_host, tmp_path):
    rng = np.random.default_rng(3)
    short = ((P(7), G_), (P(8), T_))
    long_ = short + ((P(50), A_),)
    cases = []
    for fr_short, fr_long, first, other_of_first in (([2, 2], [3, 1], long_, (0, 0)),      # equal totals: the longer list is the larger one
                                                      ([3, 2], [3, 1], short, (3, 1)),      # the prefix first: the longer list supports it
                                                      ([2, 1], [3, 1], long_, (0, 0))):
        m = {short: fr_short, long_: fr_long}
        want = update_hap_map(m, 8, 0, 1)
        assert want[0][0] == first and want[0][2] == other_of_first and want[1][2] == (-1, -1)
        cases.append(make(m, rng, min_ad=0, max_detail_cnt=1))
    check(hap_host, tmp_path, cases)


def test_link_before_base_at_one_position(hap_host, tmp_path):
    rng = np.random.default_rng(4)
    with_link = ((P(40), I1), (P(40), C_), (P(60), A_))       # the insertion in front of position 40, then the base at 40
    base_only = ((P(40), C_), (P(60), A_))
    del_first = ((P(40), D1), (P(60), A_))
    m = {with_link: [2, 2], base_only: [2, 2], del_first: [1, 3]}
    want = update_hap_map(m, 8, 0, 1)
    assert [l[0] for l in want] == [with_link, del_first, base_only]      # (p, LINK) > (p, BASE): the symbol decides at equal positions
    assert want[0][2] == (0, 0)                                            # neither of the others holds (40, I1)
    want2 = update_hap_map(m, 8, 0, 3)
    assert by_form(want2)[base_only][2] == (0, 0) and by_form(want2)[del_first][2] == (0, 0)
    s = phase_string(want2, P(40), I1)
    assert s == "((%d&<LI1>)(%d&C)(%d&A)&2&2&&2&2)" % (P(40), P(40) + 1, P(60) + 1)     # substitutions are printed one-based
    check(hap_host, tmp_path, [make(m, rng, min_ad=0, max_detail_cnt=1), make(m, rng, min_ad=0)])


def test_nested_lists_with_singletons_as_other_support(hap_host, tmp_path):
    rng = np.random.default_rng(5)
    a, b, c, d, e = (P(10), T_), (P(20), G_), (P(30), A_), (P(40), C_), (P(50), C_)
    m = {(a, b, c): [3, 3], (a, b): [4, 4], (b, c): [4, 3], (a, c): [2, 2],
         (a, b, d): [1, 0], (a, b, c, e): [0, 1], (b, c, d): [1, 0], (d, e): [0, 1]}      # four lists that occur once
    want = update_hap_map(m, 8, 1, 3)
    got = by_form(want)
    assert [l[0] for l in want] == [(a, b), (b, c), (a, b, c), (a, c)]                    # a list that occurs once is never written (1 < min_ad + size)
    assert got[(a, b)][2] == (3 + 1 + 0, 3 + 0 + 1)                                       # {a,b,c}, {a,b,d} and {a,b,c,e} stand behind it
    assert got[(b, c)][2] == (3 + 0 + 1, 3 + 1 + 0)                                       # {a,b,c}, {a,b,c,e}, {b,c,d}
    assert got[(a, b, c)][2] == (0, 1) and got[(a, c)][2] == (-1, -1)                     # only the singleton {a,b,c,e}
    check(hap_host, tmp_path, [make(m, rng), make([m, m, m], rng, max_detail_cnt=8), make(m, rng, max_detail_cnt=-1)])


def test_position_budget_carries_over_dropped_rows_but_not_min_ad_rows(hap_host, tmp_path):
    rng = np.random.default_rng(6)
    a, b, c, d, g, h, i, j, k = [(P(10 * q), q % 4) for q in range(1, 10)]
    r1, r2, r3 = (a, b), (a, c), (c, d)
    fail, r4 = (d, g, h, i, j), (g, k)
    m = {r1: [5, 5], r2: [5, 4], r3: [4, 4], fail: [3, 2], r4: [2, 2]}
    st = {}
    want = update_hap_map(m, 1, 1, 3, stats=st)
    # r1: 1 + 1 <= 2.  r2: a is at 2, 2 + 1 > 2, dropped, but c now stands at 1.  r3: c at 2, 2 + 1 > 2: dropped only because r2 counted.
    # fail: 5 reads < min_ad + 5 and raises nothing, so r4 sees g at 1: 1 + 1 <= 2, written.
    assert [l[0] for l in want] == [r1, r4] and st["budget_drops"] == 2 and st["min_ad_drops"] == 1
    assert [l[0] for l in update_hap_map({r1: m[r1], r3: m[r3]}, 1, 1, 3)] == [r1, r3]                # without r2 in front of it r3 is written
    assert [l[0] for l in update_hap_map(m, 1, 0, 3)] == [r1]              # once `fail` passes min_ad it is over its budget (d counted by r3) and costs r4 its place
    check(hap_host, tmp_path, [make(m, rng, max_count=1), make(m, rng, max_count=1, min_ad=0), make([m, {r1: m[r1], r3: m[r3]}, m], rng, max_count=1)])


NESTED = {((P(10), T_), (P(20), G_), (P(30), A_)): [3, 3], ((P(10), T_), (P(20), G_)): [4, 4], ((P(20), G_), (P(30), A_)): [4, 3],
          ((P(10), T_), (P(30), A_)): [2, 2], ((P(10), T_), (P(20), G_), (P(40), C_)): [1, 0], ((P(30), I1), (P(30), A_), (P(40), C_)): [6, 0]}


def test_max_count_and_min_ad_extremes(hap_host, tmp_path):
    rng = np.random.default_rng(7)
    assert update_hap_map(NESTED, 0, 1, 3) == []                                   # max_count 0: every row is over a budget of 0
    n0, nneg = len(update_hap_map(NESTED, 8, 0, 3)), len(update_hap_map(NESTED, 8, -3, 3))
    assert n0 == 5 and nneg == 6 and len(update_hap_map(NESTED, 8, 1, 3)) == 5     # the list that occurs once needs min_ad <= -2
    assert update_hap_map(NESTED, 8, 100, 3) == []
    assert len(update_hap_map(NESTED, 1, -3, 3)) < len(update_hap_map(NESTED, 2, -3, 3)) < nneg
    cases = [make(NESTED, rng, extra=singles(rng), max_count=v) for v in (0, 1, 2, 3)]
    cases += [make([NESTED, {}, NESTED], rng, extra=singles(rng), min_ad=v) for v in (0, -3, -100, 100, 2, 6)]
    check(hap_host, tmp_path, cases)


def test_max_detail_cnt_values_and_the_size_t_cast(hap_host, tmp_path):
    rng = np.random.default_rng(8)
    n_detailed = lambda v: sum(1 for l in update_hap_map(NESTED, 8, -3, v) if l[2] != (-1, -1))
    assert [n_detailed(v) for v in (0, 1, 3, 50)] == [0, 1, 3, 6]
    assert n_detailed(-1) == 6 and n_detailed(-2 ** 31) == 6                       # MIN((size_t)-1, size): every link is detailed
    check(hap_host, tmp_path, [make([NESTED, NESTED, {}], rng, min_ad=-3, max_detail_cnt=v) for v in (0, 1, 3, 50, -1, -7, -2 ** 31, 2 ** 31 - 1)])


def test_empty_buffers_and_buffers_of_singletons(hap_host, tmp_path):
    rng = np.random.default_rng(9)
    empty = dict(DEFAULTS, beg=BEG, npos=NPOS, maps=[{}, {}, {}], words=[])
    tail = dict(empty, words=[-1] * 9)
    one = dict(empty, words=[-1])
    lone = dict(empty, words=encode([{}, {}, {}], rng, extra=singles(rng, 9)))
    once = [{((P(q), A_), (P(q + 1 + k), C_)): [k % 2, 1 - k % 2] for q in range(0, 60, 7)} for k in range(3)]      # every list occurs once
    assert all(update_hap_map(m, 8, 1, 3) == [] for m in once) and all(len(update_hap_map(m, 8, -1, 3)) == 9 for m in once)
    check(hap_host, tmp_path, [empty, tail, one, lone, make(once, rng), make(once, rng, min_ad=-1)])


# ---- random cases ----
N_RANDOM = 2400


def random_case(rng):
    """2-6 positions and 2-4 symbols with one LINK / BASE pair at one position; up to 12 distinct lists per level with 1-6 reads per strand
    (some with one strand empty, some occurring once); the parameters drawn around the counts."""
    n_pos = int(rng.integers(2, 7))
    pos = sorted(int(v) for v in rng.choice(np.arange(0, NPOS), size=n_pos, replace=False))
    syms = [int(v) for v in rng.choice([A_, C_, G_, T_], size=int(rng.integers(1, 4)), replace=False)]
    link = int(rng.choice([D1, I1]))
    at_link = int(rng.integers(0, n_pos))
    alleles = []                                              # in the order a list holds them: ascending, LINK before BASE
    for q, p in enumerate(pos):
        if q == at_link:
            alleles.append((P(p), link))
        alleles.append((P(p), syms[int(rng.integers(0, len(syms)))]))
    if rng.random() < 0.3:                                    # a second base at one position: lists that differ in a symbol only
        q = int(rng.integers(0, len(alleles)))
        if alleles[q][1] < 4:
            alleles.insert(q + 1, (alleles[q][0], (alleles[q][1] + 1) % 4))
    maps = []
    for kind in range(3):
        m = {}
        for _ in range(int(rng.integers(0, 13))):
            keep = rng.random(len(alleles)) < rng.choice([0.4, 0.6, 0.8])
            form = tuple(a for a, k in zip(alleles, keep) if k)
            form = tuple(a for q, a in enumerate(form) if q == 0 or not (a[0] == form[q - 1][0] and a[1] < 4 and form[q - 1][1] < 4))   # one base per position
            if len(form) < 2:
                continue
            u = rng.random()
            fr = [int(rng.integers(1, 7)), int(rng.integers(1, 7))]
            if u < 0.15: fr[int(rng.integers(0, 2))] = 0
            elif u < 0.3: fr = [1, 0] if rng.random() < 0.5 else [0, 1]
            m[form] = fr
        maps.append(m)
    kw = dict(max_count=int(rng.choice([0, 1, 1, 2, 2, 3, 4, 8])), min_ad=int(rng.choice([-2, 0, 1, 1, 1, 2, 3, 6])),
              max_detail_cnt=int(rng.choice([-1, 0, 1, 2, 2, 3, 3, 5, 20])))
    return make(maps, rng, extra=singles(rng, int(rng.integers(0, 3))), **kw)


def test_random_buffers(hap_host, tmp_path):
    seed = 20240612
    rng = np.random.default_rng(seed)
    cases = [random_case(rng) for _ in range(N_RANDOM)]
    counts = dict(tie_at_boundary=0, subsets=0, budget_drops=0, min_ad_drops=0)
    for c in cases:
        st = [{}, {}, {}]
        expect(c, st)
        for k in ("tie_at_boundary", "subsets", "budget_drops", "min_ad_drops"):
            counts[k] += any(s[k] for s in st)
    print("seed", seed, "buffers", len(cases), counts)
    for k in ("tie_at_boundary", "subsets", "budget_drops", "min_ad_drops"):
        assert counts[k] >= 0.05 * len(cases), (seed, k, counts)
    check(hap_host, tmp_path, cases, what="seed %d" % seed)
