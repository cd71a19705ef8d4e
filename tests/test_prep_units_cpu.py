"""Preconditions of tests/test_gpu_prep_units.py, from the restatement alone: every case of tests/prep_unit_cases.py has what it claims (heads
on the listed read indices, more than 1 024 and more than 2 048 tiles, the three depths), every total equals the plain sum of its per-read
column, and every kind and stat_kind occurs.  The vectorised restatement is also walked read by read on the small case."""

import numpy as np
import pytest

from uvc_amd import region
import prep_unit_cases as pc
import prep_units_restatement as pr
from prep_units_restatement import D, EQ, H, I, M, N, PAD, S, X  # noqa: F401


def params_of(lib, case):
    P = region.default_params(lib, platform=case["platform"])
    for k, v in case["overrides"].items():
        setattr(P, k, v)
    return P


_cache = {}


def restated(oracle_lib, name, make):
    if name not in _cache:
        c = make()
        _cache[name] = (c, pr.prep_units(c["reads"], params_of(oracle_lib, c), c["rbeg"], c["rend"], c["npos"], c["zero_qual"]))
    return _cache[name]


def check_totals(o, n):
    assert o["n_frags"] == o["new_frag"].sum() and o["n_fs"] == o["new_fs"].sum() and o["n_complex"] == (o["kind"] != 0).sum() == len(o["complex_ids"])
    assert o["n_simple"] == n - o["n_complex"]
    assert o["n_p2"] == int(o["n_p2_of"].sum()) == int(np.diff(np.append(o["p2_first"], o["n_p2"])).sum()) == len(o["p2_aln"]) == o["p2_off[4]"]
    for total, col in (("table_rows", "trows"), ("item_slots", "items"), ("gap_slots", "gaps"), ("ins_total", "ins")):
        assert o[total] == int(o[col].sum()), total
    span = (o["fss.end"].astype(np.int64) - o["fss.beg"])
    assert o["work"] == int(span[o["fss.generic"] != 0].sum()) and o["n_generic"] == len(o["generic_fs"]) == len(o["generic_sorted"])
    assert o["n_sweep"] == len(o["sweep_frags"]) == (o["frags.stat_kind"] != 0).sum() and o["n_dup"] == len(o["dup_units"]) == len(o["dup_off"])
    assert [o["p2_off[%d]" % c] for c in range(5)] == [int((o["p2_cls"] < c).sum()) for c in range(5)]


@pytest.mark.parametrize("arm", list(pc.NESTING_ARMS))
def test_nesting_has_what_it_claims(arm, oracle_lib):
    c, o = restated(oracle_lib, "nesting_" + arm, lambda: pc.nesting(arm))
    r, n = c["reads"], c["reads"]["n_reads"]
    assert 3 * pc.TILE < n < 4 * pc.TILE and n % pc.TILE
    for e in pc.EDGES:
        for i in (e - 1, e, e + 1):
            assert o["new_frag"][i] and o["new_fs"][i], i
        assert o["kind"][e - 1] != 0 and o["kind"][e] != 0 and o["gaps"][e - 1] and o["gaps"][e] and o["ins"][e - 1] and o["trows"][e] and o["items"][e]
    shapes = {tuple(int(x) & 0xF for x in r["cigars"][a:a + k]) for a, k in zip(r["cigar_off"], r["n_cigar"])}
    assert shapes >= {(M,), (EQ, X, EQ), (S, M), (M, S), (S, M, S), (H, M), (H, S, M, S, H), (M, I, M), (M, D, M), (M, I, M, D, M, I, M), (M, I, D, M), (M, N, M), (M, PAD, M),
                      (S, I), (H,), (EQ,)}
    assert (r["l_qseq"] == 0).any()
    assert set(np.unique(o["frags.aln_end"] - o["frags.aln_beg"])) == {1, 2, 3}
    assert {1, 2, 5} <= set(np.unique(o["fss.frag_end"] - o["fss.frag_beg"]))
    partner = o["fss.other_fs"] >= 0
    duplex = (o["fss.dflag"] & 2) != 0
    assert partner.any() and (~partner).any() and (duplex & partner).any() and (duplex & ~partner).any() and ((o["fss.dflag"] & 4) != 0).any() and o["any_amplicon"] == 1
    assert o["n_dup"] > 0 and o["dup_work"] > 0
    # the last fragment: two alignments that end on the last position a read may cover; its span is clamped by the region end
    assert o["frags.aln_end"][-1] - o["frags.aln_beg"][-1] == 2 and (o["endpos"][-2:] == c["rend"] - 1).all() and o["frags.end"][-1] == c["rend"]
    assert 0 in r["mapq"] and 255 in r["mapq"] and 255 in o["frags.normMQ"]
    assert c["zero_qual"] is None and (r["quals"] == 0).sum() == 1
    assert (o["frags.stat_kind"] == pr.FRAG_STAT_ZERO_VALUE).sum() == 1 and o["frags.stat_kind"][o["frag_of"][c["zero_read"]]] == pr.FRAG_STAT_ZERO_VALUE
    assert set(np.unique(o["frags.stat_kind"])) == {0, 1, 2}
    if arm in ("default", "no_singleton"):
        assert set(np.unique(o["kind"])) == {0, 1, 2} and o["n_p2"] > n
        assert (o["n_p2_of"][o["kind"] == 2] == 0).any()              # a read of S and I ops only: no M run, yet not simple
    else:
        assert set(np.unique(o["kind"])) == {0, 1} and o["n_p2"] == o["n_simple"]
    assert bool(o["fss.generic"].all()) == (arm == "no_singleton") and set(np.unique(o["frags.singleton"])) == ({0} if arm == "no_singleton" else {0, 1})
    assert o["max_frag_depth"] == o["n_frags"] < 65536
    check_totals(o, n)


def test_restatement_walked_read_by_read(oracle_lib):
    """The closed forms of the restatement against a plain loop over the reads of the small case."""
    c, o = restated(oracle_lib, "nesting_default", lambda: pc.nesting("default"))
    r = c["reads"]
    t_off = i_off = g_off = p2 = 0
    ends = {}
    for i in range(r["n_reads"]):
        ops = [(int(x) & 0xF, int(x) >> 4) for x in r["cigars"][r["cigar_off"][i]:r["cigar_off"][i] + r["n_cigar"][i]]]
        pos = int(r["pos"][i])
        span = sum(l for op, l in ops if op in (M, EQ, X, D, N)) or 1
        runs = [op for op, l in ops if op in (M, EQ, X)]
        clips_only = all(op in (M, EQ, X, S, H) for op, l in ops)
        simple = len(runs) == 1 and clips_only and len(ops) <= 3 and not (len(ops) == 3 and ops[1][0] not in (M, EQ, X))
        offs, rp = [], 0
        for op, l in ops:
            if op in (M, EQ, X):
                offs.append((rp, span - rp - l))
            if op in (M, EQ, X, D, N):
                rp += l
        listed = simple or (not any(op in (N, PAD) for op, l in ops) and all(a <= 65535 and b <= 65535 for a, b in offs))
        kind = 0 if simple else (2 if listed else 1)
        assert (o["endpos"][i], o["kind"][i], o["p2_first"][i]) == (pos + span, kind, p2), i
        p2 += len(runs) if listed else 0
        if simple:
            assert o["table_off"][i] == o["item_off"][i] == o["gap_off"][i] == -1
        else:
            assert (o["table_off"][i], o["item_off"][i], o["gap_off"][i]) == (t_off, i_off, g_off), i
            t_off += span + 1
            i_off += 2 * int(r["l_qseq"][i]) + 2 * sum(l for op, l in ops if op == D) + len(ops) + 4
            g_off += sum(1 for op, l in ops if op in (I, D))
        for what, of in (("f", o["frag_of"][i]), ("u", o["fs_of"][i])):      # exc_end = MAX(exc_end, bam_endpos) + 1, inc_beg = MIN(inc_beg, pos)
            b, e = ends.get((what, of), (pr.INT32_MAX, 0))
            ends[what, of] = (min(b, pos), max(e, pos + span) + 1)
    for f in range(o["n_frags"]):
        assert (o["frags.beg"][f], o["frags.end"][f]) == (ends["f", f][0], min(ends["f", f][1], c["rend"])), f
    for u in range(o["n_fs"]):
        assert (o["fss.beg"][u], o["fss.end"][u]) == (ends["u", u][0], min(ends["u", u][1], c["rend"])), u


def test_carry_takes_three_rounds_in_every_column(oracle_lib):
    c, o = restated(oracle_lib, "carry", pc.carry)
    n = c["reads"]["n_reads"]
    assert n == 2 * 1024 * 2048 + 2048 + 1 == 4_196_353
    ntiles = -(-n // pc.TILE)
    assert ntiles == 2050 > 2 * 1024                          # rounds of 1 024 tiles: two full ones and a third
    cols = dict(new_frag=o["new_frag"], new_fs=o["new_fs"], complex=o["kind"] != 0, n_p2=o["n_p2_of"], trows=o["trows"], items=o["items"], ins=o["ins"], gaps=o["gaps"])
    for name, col in cols.items():
        tile_sums = np.add.reduceat(col.astype(np.int64), np.arange(0, n, pc.TILE))
        assert (tile_sums[:2049] > 0).all() and tile_sums[:1024].sum() > 0 and tile_sums[1024:2048].sum() > 0, name   # both carries are non-zero
    i = np.arange(n)
    assert np.array_equal(o["new_frag"], (i % 3 == 0) | (i % 7 == 0)) and np.array_equal(o["new_fs"], i % 7 == 0)
    assert c["npos"] == 4096 and c["reads"]["pos"].min() == c["rbeg"] and o["endpos"].max() <= c["rend"] - 1
    # the largest 64-bit offset of the case: far from 2^31, so no column passes it by accident
    assert o["item_off"].max() == 27_276_275 and o["table_off"].max() < o["item_off"].max() < 2 ** 31
    assert set(np.unique(o["kind"])) == {0, 2} and o["n_frags"] >= 65536 and o["max_frag_depth"] < o["n_frags"]
    check_totals(o, n)


@pytest.mark.parametrize("arm", list(pc.DEPTH_ARMS))
def test_depth_arms_give_the_three_depths(arm, oracle_lib):
    c, o = restated(oracle_lib, "depth_" + arm, lambda: pc.depth(arm))
    k, extra, want = pc.DEPTH_ARMS[arm]
    assert c["npos"] == 2_100_000 and -(-(c["npos"] + 1) // pc.TILE) > 1024 and pc.DEPTH_PILE > pc.ROUND      # the pile lies behind the first round of the depth scan
    assert o["n_frags"] == pc.DEPTH_THIN + k + extra == c["reads"]["n_reads"]
    beg, end = o["frags.beg"].astype(np.int64) - c["rbeg"], o["frags.end"].astype(np.int64) - c["rbeg"]
    assert (beg[:pc.DEPTH_THIN] < pc.ROUND).all()              # every thin fragment begins inside it: the pile's depth is carried
    over_pile = int(((beg <= pc.DEPTH_PILE) & (end > pc.DEPTH_PILE)).sum())
    assert over_pile == pc.DEPTH_THIN + k == want == o["max_frag_depth"]
    assert (o["n_frags"] < 65536) == (arm == "count_65535")
    assert o["table_rows"] > 2 ** 32                           # (64-bit offsets in earnest)


def test_depth_covers_both_sides_of_65536():
    assert sorted(v[2] for v in pc.DEPTH_ARMS.values()) == [65535, 65535, 65536, 65537]


def test_compact_lengths_are_odd_and_not_dense():
    l_qseq, n_cigar = pc.carry_lengths()
    assert len(l_qseq) == pc.CARRY_N and (l_qseq % 2 == 1).any() and (l_qseq % 2 == 0).any()
    off = pr.compact_offsets(l_qseq, n_cigar)
    n_b4 = int(off["b4_off"][-1] + (l_qseq[-1] + 1) // 2)
    assert 2 * n_b4 != int(l_qseq.sum())                      # not the dense form: uvc_prep_compact writes the 4-bit offsets
    for v in off.values():
        assert v[0] == 0 and (np.diff(v) > 0).all() and v[pc.ROUND] > 0 and v[2 * pc.ROUND] > v[pc.ROUND]


def test_sort_cases_tie_and_reach_both_ends():
    assert len(pc.SORT_BITS) == 11 and pc.SORT_BEG != 0
    for pb, cb in pc.SORT_BITS:
        assert 1 <= pb and pb + cb <= 32
        for n in pc.SORT_N:
            c = pc.sort_case(pb, cb, n)
            key = pr.sort_key(c["pos"], c["cls"], c["beg"], pb)
            assert len(key) == n and key.max() == (1 << (pb + cb)) - 1 and (n == 1 or key.min() == 0)
            assert len(np.unique(key)) <= 8 << cb and (n < 255 or len(np.unique(key)) < n // 4)           # most keys tie
            assert c["n_first"] == [0, n // 2, n]
            more, fewer = c["lists"]
            assert len(fewer["kind"]) > n and (len(more["kind"]) < n or n == 1)
            for l in c["lists"]:
                per = np.bincount(l["a"][0], minlength=len(l["kind"]))
                assert len(l["a"][0]) == n and (per[l["kind"] == 0] == 1).all() and (per[l["kind"] == 1] == 0).all()
            assert n < 255 or (per_kind2(more) > 1).any()


def per_kind2(l):
    return np.bincount(l["a"][0], minlength=len(l["kind"]))[l["kind"] == 2]
