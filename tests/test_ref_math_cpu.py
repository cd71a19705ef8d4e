"""The oracle's math primitives pinned on the reference's own functions, bit for bit.

oracle/_ref/libref_math.so is the reference's main_conversion.hpp, main_consensus.hpp and the macros of common.hpp, compiled from where they
lie by `make -C oracle ref_math` behind a C wrapper (oracle/ref_math_driver.cpp; oracle/ref_shim/ stands in for the two htslib headers they
include).  Every primitive the oracle has is compared with it over the grids of tests/math_grids.py: doubles by their bits, integers exactly.
The consensus blocks of the oracle and of the product (uvc_conblock.cpp is host code) are compared with the reference's ConsensusBlockSet on
the cases of tests/test_conblock.py; which events of a read reach the block set is main.hpp's business (not compilable) and stays with the
restatement of that file.  The symbol tables and predicates are compared over their whole domain, with the Python copies of the suite too.
The functions of main.hpp (indel_phred, hetLODQ, ...) have no compiled reference: tests/test_oracle_math.py keeps what pins them."""
import ctypes as C
import os

import numpy as np
import pytest

import math_grids as G
import score_restatement as SR
from msi_restatement import ref_codes
import test_conblock as TC
from uvc_amd import _ffi, consensus, region, synth

pytestmark = pytest.mark.skipif(not os.path.exists(G.REF_SO), reason="oracle/_ref/libref_math.so not built (needs /root/reference at build time)")


@pytest.fixture(scope="module")
def ref():
    return C.CDLL(G.REF_SO)


def both(ref, oracle_lib, name, rows):
    op = G.OPS[name]
    rows = G.host_rows(name, rows)
    return G.call_host(ref, op.ref, rows, op.n_out), G.call_host(oracle_lib.dll, op.oracle, rows, op.n_out)


def same_bits(a, b, rows, what):
    bad = np.flatnonzero((G.bits(a) != G.bits(b)).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d rows differ, first %r: reference %r, oracle %r" % (what, len(bad), len(rows), rows[bad[0]].tolist(), a[bad[0]].tolist(), b[bad[0]].tolist())


SCALAR = {
    "phred2nat": G.scalar_grid, "numstates2phred": G.scalar_grid, "numstates2deciphred": G.scalar_grid,
    # (numstates2deciphred of 0, -0, -1, +-inf and NaN converts a non-finite double to int32, undefined in C++: what is pinned there is the x86-64
    # build, cvttsd2si -> INT32_MIN, which the reference's binaries, the oracle and -- through i32_as_x86 -- the kernels all give)
    "prob2odds": G.probabilities, "odds2prob": G.scalar_grid, "logit": G.probabilities, "prob2realphred": G.scalar_grid,
    "prob2phred": lambda: np.vstack([G.log_spaced_doubles()[:2048], G.probabilities()[1:-1]]),
    "phred2prob": lambda: np.arange(-200.0, 4097.0).reshape(-1, 1), "proton_cigarlen2phred": G.integers_0_4096,
    "calc_non_negative_float": lambda: np.concatenate([np.linspace(-400.0, 400.0, 8001), np.arange(-50.0, 50.0, 1.0), [np.inf, -np.inf, 1e30, -1e30]]).reshape(-1, 1),
    "logit2": G.logit2_grid, "dp4": G.dp4_grid, "symbols_mutated": G.symbol_pairs,
    "symbol_kind": lambda: np.arange(0.0, 17.0).reshape(-1, 1), "len_to_symbol": lambda: np.arange(0.0, 41.0).reshape(-1, 1),
    "non_neg_minus": lambda: np.stack(np.meshgrid(G.scalar_grid()[::41, 0], G.scalar_grid()[::37, 0], indexing="ij"), -1).reshape(-1, 2),
    "non_neg_minus_i64": lambda: np.stack(np.meshgrid(np.arange(-64.0, 4097.0, 7), np.arange(-64.0, 4097.0, 11), indexing="ij"), -1).reshape(-1, 2),
}


@pytest.mark.parametrize("name", sorted(SCALAR))
def test_oracle_primitive_equals_the_reference(ref, oracle_lib, name):
    rows = SCALAR[name]()
    assert len(rows) > 10
    a, b = both(ref, oracle_lib, name, rows)
    same_bits(a, b, rows, name)


def test_binom_likeratio_all_four_forms(ref, oracle_lib):
    g = G.binom_grid(step=2)
    for bidir in (0, 1):
        for maxone in (0, 1):
            rows = np.hstack([g, np.full((len(g), 1), float(bidir)), np.full((len(g), 1), float(maxone))])
            if maxone:   # probabilities above one, which only this form brings back into range
                rows = np.vstack([rows, rows[::50] * np.array([3.0, 1, 1, 1, 1])])
            a = G.call_host(ref, "ref_binom_llr", rows, 1); b = G.call_host(oracle_lib.dll, "uvc_oracle_math_binom_llr", rows, 1)
            same_bits(a, b, rows, "calc_binom_10log10_likeratio<%d, %d>" % (bidir, maxone))


def test_infer_max_qual_on_the_adversarial_histograms_and_off_dec_qual_one(ref, oracle_lib):
    rows, names = G.adversarial_histograms(4000, seed=5)
    for dq in (1, 2, 3, 5):
        full = np.hstack([rows[:, :17], np.full((len(rows), 1), float(dq)), rows[:, 17:18]])
        a, b = both(ref, oracle_lib, "infer_max_qual", full)
        same_bits(a, b, full, "infer_max_qual dec_qual %d" % dq)
    assert (a[:, 0] > 0).sum() > 1000


def test_stored_adversarial_histograms_are_the_generators():
    """tests/golden/math_exact.npz keeps the 20 000 histograms the device test runs (their search takes seconds): still what the generator
    makes, class by class, and no class is empty"""
    z = np.load(G.EXACT_NPZ)
    rows, names = G.adversarial_histograms()
    classes = sorted(G.ADVERSARIAL_MIN)
    assert np.array_equal(z["adv_rows"], rows.astype(np.int32)) and [classes[k] for k in z["adv_class"]] == names.tolist()
    for name, least in G.ADVERSARIAL_MIN.items():
        assert (names == name).sum() >= least, name


@pytest.mark.parametrize("max_qual", G.MAX_QUALS)
def test_infer_max_qual_exhaustive_single_bucket(ref, oracle_lib, max_qual):
    """every 1 <= currAD <= totDP <= 2048: the domain with the 2 274 pairs whose value lies within 1e-11 of a whole number"""
    for dq in (1,) + G.DEC_QUALS_GENERIC:
        rows = G.one_bucket_rows(max_qual, dq)
        a, b = both(ref, oracle_lib, "infer_max_qual_one", rows)
        same_bits(a, b, rows, "infer_max_qual max_qual %d dec_qual %d" % (max_qual, dq))
    # the compact row is the 16-bucket row with one bucket filled
    few = rows[::997]
    full = np.zeros((len(few), 19)); full[:, 0] = few[:, 1]; full[:, 16:] = few[:, 2:]
    assert np.array_equal(G.call_host(ref, "ref_infer_max_qual", full, 3), G.call_host(ref, "ref_infer_max_qual_one", few, 3))


# ---- tables and predicates over their whole domain, and the Python copies of the suite ----
def test_char_to_symbol(ref, oracle_lib):
    r = np.zeros(128, np.int32); o = np.zeros(256, np.int32)
    ref.ref_char_to_symbol(C.c_void_p(r.ctypes.data)); oracle_lib.dll.uvc_oracle_math_char_to_symbol(C.c_void_p(o.ctypes.data))
    assert r.tolist() == o[:128].tolist()
    assert set(o[128:].tolist()) == {4}                                       # (the reference's table ends at 127)
    # the importable copy the suite holds, msi_restatement.ref_codes (base letters only; test_prep_cpu.py and others write the same table inline)
    py = ref_codes(bytes(range(128))).tolist()
    assert ref_codes(bytes(range(128, 256))).tolist() == o[128:].tolist()
    assert [(c, r[c], py[c]) for c in range(128) if r[c] != py[c] and chr(c) not in "Ii-_"] == []
    assert [int(r[ord(c)]) for c in "Ii-_"] == [SR.LINK_M, SR.LINK_M, SR.LINK_D1, SR.LINK_D1]


def test_symbol_predicates_and_python_copies(ref):
    k = G.call_host(ref, "ref_symbol_kind", np.arange(0.0, 14.0).reshape(-1, 1), 3)
    for s in range(14):
        assert (bool(k[s, 0]), bool(k[s, 1]), bool(k[s, 2])) == (SR.is_ins(s), SR.is_del(s), SR.is_subst(s)), s
    ls = G.call_host(ref, "ref_len_to_symbol", np.arange(0.0, 41.0).reshape(-1, 1), 2)
    for n in range(41):
        assert ls[n].tolist() == [SR.LINK_I1 if n == 1 else SR.LINK_I2 if n == 2 else SR.LINK_I3P, SR.LINK_D1 if n == 1 else SR.LINK_D2 if n == 2 else SR.LINK_D3P]
    m = G.call_host(ref, "ref_symbols_mutated", G.symbol_pairs(), 1).reshape(14, 14)
    for r_ in range(14):
        for a in range(14):
            want = (r_ != a and r_ < 4 and a < 4) if a <= SR.BASE_NN else (a not in (SR.LINK_M, SR.LINK_NN))
            assert bool(m[r_, a]) == want, (r_, a)
    plat = np.zeros(4, np.int32); ref.ref_sequencing_platforms(C.c_void_p(plat.ctypes.data))
    assert plat.tolist() == [0, 1, 2, 3] and plat[2] == SR.SEQUENCING_PLATFORM_IONTORRENT
    assert (SR.BASE_NN, SR.LINK_M, SR.LINK_D3P, SR.LINK_D2, SR.LINK_D1, SR.LINK_I3P, SR.LINK_I2, SR.LINK_I1, SR.LINK_NN) == tuple(range(5, 14))
    assert [_ffi.ENUMS[n] for n in ("UVC_BASE_A", "UVC_BASE_N", "UVC_BASE_NN", "UVC_LINK_M", "UVC_LINK_D3P", "UVC_LINK_I1", "UVC_LINK_NN")] == [0, 4, 5, 6, 7, 12, 13]


def test_process_cigar_every_op(ref):
    """ops 0..15: the four ops process_cigar handles itself move what the oracle's and the kernels' CIGAR walks move; BAM_CBACK throws -1 and
    everything else (the ops its callers handle before, and the unassigned codes) -2"""
    rows = np.array([(op, ln) for op in range(16) for ln in (0, 1, 7, 1000)], dtype=np.float64)
    out = G.call_host(ref, "ref_process_cigar", rows, 3)
    for (op, ln), (q, r, t) in zip(rows.tolist(), out.tolist()):
        want = {3: (0, ln, 0), 4: (ln, 0, 0), 5: (0, 0, 0), 6: (0, 0, 0), 9: (0, 0, -1)}.get(int(op), (0, 0, -2))
        assert (q, r, t) == want, (op, ln)


def test_small_helpers(ref):
    x = G.scalar_grid()[:6000]   # (squares and cubes that stay finite)
    assert np.array_equal(G.bits(G.call_host(ref, "ref_mathsquare", x, 1)), G.bits(x * x))
    assert np.array_equal(G.bits(G.call_host(ref, "ref_mathcube", x, 1)), G.bits(x * x * x))
    v = np.linspace(-100, 100, 2001)
    rows = np.stack([v, np.full_like(v, 0.25), np.full_like(v, 60.0)], -1)
    assert np.array_equal(G.call_host(ref, "ref_calc_score_with_penal_at_low_val", rows, 1)[:, 0], v * 0.25)
    dflt = G.call_host(ref, "ref_calc_non_negative", np.stack([v, np.full_like(v, np.nan), np.zeros_like(v)], -1), 1)[:, 0]
    assert (dflt[v >= 10] == v[v >= 10]).all() and (dflt > 0).all() and (np.diff(dflt[v < 10]) >= 0).all()   # (a soft floor below the threshold, the identity from it on)


# ---- consensus blocks on the reference's ConsensusBlockSet ----
def ref_unit_blocks(ref, events, fragment_level=False):
    """events: (fragment index, type, position, [(base code, quality)]) in read order -> {(type, position): rows}"""
    n = len(events)
    off = np.cumsum([0] + [len(e[3]) for e in events]).astype(np.int64)
    seq = "".join("ACGTN"[b] for e in events for b, _ in e[3]).encode() + b"\0"
    qual = np.array([q for e in events for _, q in e[3]] + [0], np.int8)
    arr = lambda k: np.array([e[k] for e in events] + [0], np.int32)
    ef, et, ep, el = arr(0), arr(1), arr(2), np.array([len(e[3]) for e in events] + [0], np.int32)
    blocks = np.zeros((n + 1, 4), np.int32); rows = np.zeros((int(off[-1]) + 1, 8), np.int32)
    fn = ref.ref_conblock_unit
    fn.restype = C.c_int64
    fn.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    nb = fn(n, ef.ctypes.data, et.ctypes.data, ep.ctypes.data, off.ctypes.data, el.ctypes.data, seq, qual.ctypes.data, int(fragment_level), blocks.ctypes.data, len(blocks), rows.ctypes.data, len(rows))
    assert nb >= 0
    return {(int(t), int(p)): rows[o:o + ln].tolist() for t, p, ln, o in blocks[:nb].tolist()}


def ref_family_blocks(ref, reads, P, min_fragments):
    """test_conblock.py_family_blocks with the reference's block sets in place of its dictionaries"""
    res = {}
    key = list(zip(reads["fam_id"].tolist(), reads["fam_strand"].tolist()))
    i, n = 0, reads["n_reads"]
    while i < n:
        j = i
        while j < n and key[j] == key[i]:
            j += 1
        frags = {}
        for k in range(i, j):
            frags.setdefault(int(reads["frag_id"][k]), []).append(k)
        if len(frags) >= min_fragments:
            events = [(g, t, r, seq) for g, (fid, members) in enumerate(frags.items()) for k in members for (t, r, seq) in TC.py_events(reads, k, P)]
            for (t, r), rows in ref_unit_blocks(ref, events).items():
                res[(key[i][0], key[i][1], t, r)] = (len(frags), rows)
        i = j
    return res


def ref_to_seq(ref, rows, r2l, trim):
    rows = np.ascontiguousarray(rows, np.int32).reshape(-1, 8)
    out = np.zeros((len(rows) + 1, 4), np.int32)
    p, k = trim if trim is not None else (-1, 0)
    fn = ref.ref_conblock_to_seq
    fn.restype, fn.argtypes = C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    n = fn(rows.ctypes.data, len(rows), int(r2l), p, k, out.ctypes.data)
    return [(chr(b), q, fs, fi) for b, q, fs, fi in out[:n].tolist()]


@pytest.mark.parametrize("case", [dict(seed=31, region_len=4000, depth=200, umi=True, indel_every=100, clip_frac=0.2),
                                  dict(seed=32, region_len=3000, depth=100, indel_every=100, clip_frac=0.3, min_fragments=1, set=dict(primerlen=20))])
def test_consensus_blocks_equal_the_references_block_set(case, ref, oracle_lib):
    product_lib = _ffi.Lib(_ffi.gpu_library_path(), "uvcgpu_")
    case = dict(case); overrides = case.pop("set", {}); mf = case.pop("min_fragments", 2)
    reads = synth.generate_region(**case)
    P = region.default_params(product_lib)
    for k, v in overrides.items():
        setattr(P, k, v)
    want = ref_family_blocks(ref, reads, P, mf)
    n_seq = 0
    for lib in (product_lib, oracle_lib):
        got = consensus.family_blocks(lib, P, reads, min_fragments=mf)
        assert len(got) == len(want) > 20
        for b in got:
            k = (b["fam_id"], b["strand"], b["type"], b["refpos"])
            assert b["n_fragments"] == want[k][0] and b["rows"].tolist() == want[k][1], k
            for trim in (None, (20, 3), (20, 5), (60, 1), (150, 2)):
                r2l = (b["type"] == 2)
                assert consensus.block_to_seq(lib, b["rows"], r2l, trim) == ref_to_seq(ref, b["rows"], r2l, trim), (k, trim)
                n_seq += 1
    assert n_seq > 200


def test_hand_written_family_on_the_references_block_set(ref, oracle_lib):
    """the family of test_conblock.test_a_family_written_down_by_hand, fragment level too: incByPosSeqQual's per-base maxima"""
    product_lib = _ffi.Lib(_ffi.gpu_library_path(), "uvcgpu_")
    P = region.default_params(product_lib)
    reads = TC.make_reads([
        (0, 0, 0, 100, "5M3I2M", "AAAAAACGTT", [30, 30, 30, 30, 30, 20, 25, 35, 30, 30], 0x0, 100, 0),
        (0, 0, 1, 100, "5M3I2M", "AAAAAACGTT", [30, 30, 30, 30, 30, 40, 10, 15, 30, 30], 0x0, 100, 0),
        (0, 0, 2, 100, "5M2I3M", "AAAAAATTTT", [30, 30, 30, 30, 30, 22, 33, 30, 30, 30], 0x0, 100, 0),
        (1, 1, 0, 200, "3S7M", "GCATTTTTTT", [11, 12, 13] + [30] * 7, 0x10, 200, 0),
        (1, 1, 0, 200, "2S5M3S", "TATTTTTACG", [21, 9] + [30] * 5 + [5, 6, 7], 0x10, 200, 0),
        (2, 0, 0, 300, "4S4M", "NACGACGT", [200, 128, 127, 0] + [30] * 4, 0x0, 300, 0),     # quality bytes above 127 are negative in the reference's int8 vector
    ])
    want = ref_family_blocks(ref, reads, P, 1)
    assert sorted(want) == [(0, 0, 1, 105), (1, 1, 0, 205), (1, 1, 2, 200), (2, 0, 2, 300)]
    for lib in (product_lib, oracle_lib):
        got = {(b["fam_id"], b["strand"], b["type"], b["refpos"]): b["rows"].tolist() for b in consensus.family_blocks(lib, P, reads, min_fragments=1)}
        assert got == {k: v[1] for k, v in want.items()}
        frag = consensus.fragment_blocks(lib, P, reads, 3, 2)
        events = [(0, t, r, seq) for k in (3, 4) for (t, r, seq) in TC.py_events(reads, k, P)]
        assert {(b["type"], b["refpos"]): b["rows"].tolist() for b in frag} == ref_unit_blocks(ref, events, fragment_level=True)
