"""The scalar math of the scoring and accumulate kernels on the device, function by function, against the reference's own functions.

uvc_launch_math_probe (uvc_kernels_score.hip; an internal launch entry like uvc_launch_block_scan) runs one DEV function per row of a grid.
The grids are those of tests/math_grids.py.  The comparator:

  libref_math.so (the reference's headers, compiled)      liboracle.so (main.hpp has no compiled form)
  ---------------------------------------------------     --------------------------------------------
  phred2nat numstates2phred numstates2deciphred           indel_phred_s          (indel_phred)
  prob2odds logit2 binom_llr (<false, false>)              indel_len_rusize_phred_s
  dp4 (the four template forms)                            more_STR_s             (is_indel_context_more_STR)
  symbols_mutated (areSymbolsMutated)                      norm_fa
  infer_max_qual, infer_max_qual_regs                      het_lodq               (hetLODQ)
  proton_cigarlen2phred                                    normv_quals, normv_quals2
  phred2prob, and through the table of k_fam_p5d           sscs_phred             (toPhredErrRate)
                                                           i32_as_x86             (cvttsd2si, by intrinsic)

Integer-valued results equal the comparator's at every grid point, +-inf, NaN and negative arguments included.  A row is knife-edge when the
exact value in front of the truncation (50-digit mpmath, tests/golden/math_exact.npz, made by tests/golden/make_math_exact.py) is closer to a
breakpoint than 4 x the largest error of the comparator's expression in double precision on that grid; such rows are counted and printed,
equality is asserted on them all the same, and they may be 0.2 % of a grid at most.  Double-valued results, two assertions:
  * against the exact value, over the stored rows of the grid (every row with a count of 1e3 or more, every row on the line a == prob * (a + b),
    the edges, and an even sample: math_grids.*_exact_rows): max |device - exact| / scale <= max(4 x max |comparator - exact| / scale, 2^-52),
    and the same row by row with 4 x 2^-52 added, so that one ill-conditioned row does not set the bound for the others;
  * against the comparator, over the WHOLE grid: |device - comparator| <= k x 2^-52 x scale, k counted from the operations (close_everywhere).
scale = |value| for products and quotients and the sum of the absolute terms for a sum (binom_llr: 10 / ln 10 (|a log(a / A)| +
|b log(b / B)|); dp4's first result is quotient x exp((n_nats - infogain) / pl_exponent), so an absolute error of the sum is a relative
error of the result: scale = |value| x max(1, (|n_nats| + the absolute terms of infogain) / pl_exponent)).  Plain arithmetic (phred2nat,
prob2odds, norm_fa, dp4's second result) is IEEE on both sides and is compared by its bits.

Buffers go through the HIP runtime the library links, as in test_gpu_block_scan.py.

Measured on the MI355X (|.| / scale; "whole grid" is device against comparator on every row, with its bound):
  primitive         device - exact   comparator - exact   stored rows   whole grid, device - comparator   bound
  binom_llr         0.536            0.536                11057         3.85e-16 of 1 110 802 rows         6 x 2^-52 = 1.33e-15
  dp4 (result 0)    3.91e-12         3.91e-12             5024          2.56e-16 of 165 888                8 x 2^-52 = 1.78e-15
  numstates2phred   3.78e-16         3.78e-16             4097          2.09e-16 of 8 203                  3 x 2^-52
  logit2            0.0175           0.0175               4424          2.22e-16 of 176 400                2 x 2^-52
  norm_fa           2.72e-16         2.72e-16             2136          0 of 2 144                         0
  phred2prob        1.78e-16         1.06e-16             301           2.22e-16 of 341                    4 ulp
  (binom_llr, dp4 and logit2: the largest error against the exact value is that of a few ill-conditioned rows -- 1 - prob at prob = 1 - 1e-9
  with a count of a million, a count of 1e-15 -- and is the arithmetic's, the same on both sides to the digits shown.)
  knife-edge rows: infer_max_qual 2 274 of 2 098 176 (0.108 %) at every max_qual; indel_phred 2 of 1 200 (0.167 %); binom_llr's branch 998
  of 1 110 802 (0.090 %); numstates2deciphred and het_lodq's binomial term 0.  The device equals the comparator on every one of them: no
  integer result differs anywhere, no branch of binom_llr, and no stored row of dp4 sits on another branch than its exact value.
  What the tests found: (int)round(x) in numstates2deciphred gave INT32_MAX / 0 for x = +inf / NaN where x86 gives INT32_MIN; the device
  function now converts through i32_as_x86, as het_lodq does.
"""
import ctypes as C
import os

import numpy as np
import pytest

import math_grids as G

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2
CAP = 0.002
FLOOR = 2.0 ** -52


class Probe:
    def __init__(self, gpu_lib):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; self.hip.hipFree.argtypes = [C.c_void_p]
        self.lib = gpu_lib.dll
        self.fn = gpu_lib.dll.uvc_launch_math_probe
        self.fn.restype, self.fn.argtypes = C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]

    def __call__(self, names, rows):
        """one upload of `rows`, one launch per name in `names` (ops that take the same row) -> list of results"""
        single = isinstance(names, str)
        names = [names] if single else list(names)
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        n, n_in = rows.shape
        res = []
        d_in, d_out = C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d_in), rows.nbytes) == 0
        try:
            assert self.hip.hipMemcpy(d_in, rows.ctypes.data, rows.nbytes, H2D) == 0
            for name in names:
                op = G.OPS[name]
                assert n_in == op.n_in, (name, n_in)
                out = np.full((n, op.n_out), np.nan)   # (a row the kernel does not write stays NaN)
                assert self.hip.hipMalloc(C.byref(d_out), out.nbytes) == 0
                try:
                    assert self.hip.hipMemcpy(d_out, out.ctypes.data, out.nbytes, H2D) == 0
                    assert self.fn(op.probe, n, d_in, n_in, d_out, op.n_out, None) == 0   # the null stream: the copy back waits for it
                    assert self.hip.hipMemcpy(out.ctypes.data, d_out, out.nbytes, D2H) == 0
                finally:
                    self.hip.hipFree(d_out)
                res.append(out)
        finally:
            self.hip.hipFree(d_in)
        return res[0] if single else res


@pytest.fixture(scope="module")
def probe(gpu_lib):
    return Probe(gpu_lib)


@pytest.fixture(scope="module")
def ref():
    return C.CDLL(G.REF_SO) if os.path.exists(G.REF_SO) else None   # (the tests whose comparator is liboracle.so run without it)


@pytest.fixture(scope="module")
def exact():
    return np.load(G.EXACT_NPZ)


def comparator(ref, oracle_lib, name, rows):
    op = G.OPS[name]
    rows = G.host_rows(name, rows)
    if op.ref and ref is None:
        pytest.skip("oracle/_ref/libref_math.so not built (needs /root/reference at build time)")
    return G.call_host(ref, op.ref, rows, op.n_out) if op.ref else G.call_host(oracle_lib.dll, op.oracle, rows, op.n_out)


def same(a, b):
    return (G.bits(a) == G.bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_equal(name, rows, dev, cmp_):
    bad = np.flatnonzero(~same(dev, cmp_).all(axis=1))
    print("%s: %d rows, %d differ" % (name, len(rows), len(bad)))
    for i in bad[:20]:
        print("   row %d %r: device %r comparator %r" % (i, rows[i].tolist(), dev[i].tolist(), cmp_[i].tolist()))
    assert len(bad) == 0, "%s: %d of %d rows differ from the comparator, first %r: device %r, comparator %r" % (name, len(bad), len(rows), rows[bad[0]].tolist(), dev[bad[0]].tolist(), cmp_[bad[0]].tolist())


def knife_rows(exact, key, n_rows):
    idx, dist, err = exact[key + "_idx"], exact[key + "_dist"], float(exact[key + "_cmp_err"])
    k = idx[np.abs(dist) < 4 * err]
    print("%s: %d knife-edge rows of %d (%.4f %%), comparator error %.3g" % (key, len(k), n_rows, 100.0 * len(k) / n_rows, err))
    assert len(k) <= CAP * n_rows, key
    return k


def error_bound(name, exact, key, dev, cmp_, scale, skip=None):
    """both sides of max |device - exact| / scale <= max(4 max |comparator - exact| / scale, 2^-52) over the stored rows"""
    rows = exact[key + "_rows"]
    ex = exact[key + "_hi"].astype(np.longdouble) + exact[key + "_lo"].astype(np.longdouble)
    d, c, s = dev[rows].astype(np.longdouble), cmp_[rows].astype(np.longdouble), np.asarray(scale, np.longdouble)[rows]
    use = np.isfinite(ex) & np.isfinite(c) & (s > 0)
    if skip is not None:
        use &= ~skip[rows]
    assert np.array_equal(np.isfinite(d[use]), np.isfinite(c[use])) and use.sum() > len(rows) // 2, name
    ed, ec = np.abs(d[use] - ex[use]) / s[use], np.abs(c[use] - ex[use]) / s[use]
    lhs, rhs = float(np.max(ed)), float(np.max(ec))
    print("%s: max |device - exact| / scale = %.3g, max |comparator - exact| / scale = %.3g, max |device - comparator| / scale = %.3g, over %d rows"
          % (name, lhs, rhs, float(np.max(np.abs(d[use] - c[use]) / s[use])), int(use.sum())))
    assert lhs <= max(4 * rhs, FLOOR), (name, lhs, rhs)
    # and row by row, so that one ill-conditioned row of the grid does not set the bound for all the others
    worse = np.flatnonzero(ed > 4 * ec + 4 * FLOOR)
    assert len(worse) == 0, (name, len(worse), rows[use][worse[:5]].tolist(), ed[worse[:5]].tolist(), ec[worse[:5]].tolist())
    # rows without a finite exact value or scale: the device says what the comparator says
    rest = ~use if skip is None else (~use & ~skip[rows])
    assert same(dev[rows][rest], cmp_[rows][rest]).all(), name


def close_everywhere(name, dev, cmp_, scale, k, skip=None):
    """over the WHOLE grid, no exact value needed: |device - comparator| <= k * 2^-52 * scale on every row where the comparator is finite, and
    what the comparator says on the others.  k counts the places where the two sides can part: each library's logarithm or exponential is
    good to 1 ulp, so a call differs by 2 at most, and every IEEE operation behind it rounds a slightly different input once more (1 each)."""
    d, c, s = dev.astype(np.longdouble), cmp_.astype(np.longdouble), np.asarray(scale, np.longdouble)
    fin = np.isfinite(c) & np.isfinite(s)
    if skip is not None:
        fin &= ~skip
    with np.errstate(all="ignore"):
        far = fin & ~(np.abs(d - c) <= k * FLOOR * s)
        ratio = np.where(fin & (s > 0), np.abs(d - c) / np.where(s > 0, s, 1), 0)
    print("%s: whole grid of %d rows, max |device - comparator| / scale = %.3g (bound %d x 2^-52 = %.3g), %d rows beyond it" % (name, len(c), float(ratio.max()), k, k * FLOOR, int(far.sum())))
    assert not far.any(), (name, int(far.sum()), np.flatnonzero(far)[:5].tolist(), dev[far][:5].tolist(), cmp_[far][:5].tolist())
    rest = ~fin if skip is None else (~fin & ~skip)
    assert same(dev[rest], cmp_[rest]).all(), name


# ---- the probe refuses what it cannot run ----
def test_probe_refuses_bad_calls(probe):
    one = C.c_void_p(8)   # never dereferenced: nothing is launched
    assert probe.fn(-1, 1, one, 1, one, 1, None) == -1 and probe.fn(len([o for o in G.OPS.values() if o.probe is not None]), 1, one, 1, one, 1, None) == -1
    assert probe.fn(G.OPS["dp4"].probe, 1, one, 12, one, 2, None) == -1 and probe.fn(G.OPS["dp4"].probe, 1, one, 13, one, 1, None) == -1
    assert probe.fn(0, 0, one, 1, one, 1, None) == -1 and probe.fn(0, 1, None, 1, one, 1, None) == -1
    # the second entry, which the first hands its three ops: the same refusals on its own
    fn2 = probe.lib.uvc_launch_math_probe_acc
    fn2.restype, fn2.argtypes = probe.fn.restype, probe.fn.argtypes
    first = G.OPS["proton_cigarlen2phred"].probe
    assert fn2(first - 1, 1, one, 1, one, 1, None) == -1 and fn2(first + 3, 1, one, 1, one, 1, None) == -1 and fn2(first, 0, one, 1, one, 1, None) == -1
    assert fn2(first, 1, one, 0, one, 1, None) == -1 and fn2(first, 1, one, 1, None, 1, None) == -1


# ---- infer_max_qual ----
@pytest.mark.parametrize("max_qual", G.MAX_QUALS)
def test_infer_max_qual_exhaustive_single_bucket(probe, ref, oracle_lib, exact, max_qual):
    """every 1 <= currAD <= totDP <= 2048, both forms at dec_qual 1, the generic form at dec_qual 2, 3, 5 too"""
    n = len(G.one_bucket_pairs()[0])
    knife_rows(exact, "infer_one_%d" % max_qual, n)
    for dq in (1,) + G.DEC_QUALS_GENERIC:
        rows = G.one_bucket_rows(max_qual, dq)
        want = comparator(ref, oracle_lib, "infer_max_qual_one", rows)
        names = ["infer_max_qual_one", "infer_max_qual_regs_one"] if dq == 1 else ["infer_max_qual_one"]
        for name, got in zip(names, probe(names, rows)):
            assert_equal("%s max_qual %d dec_qual %d" % (name, max_qual, dq), rows, got, want)


def test_infer_max_qual_regs_adversarial(probe, ref, oracle_lib, exact):
    rows = exact["adv_rows"].astype(np.float64)
    classes = sorted(G.ADVERSARIAL_MIN)
    cls = exact["adv_class"]
    assert len(rows) == 20000
    for k, name in enumerate(classes):
        n = int((cls == k).sum())
        print("class %s: %d cases" % (name, n))
        assert n >= G.ADVERSARIAL_MIN[name], name
    assert (rows[:, :16].sum(axis=1) <= rows[:, 17]).all() and (rows[:, :16].min() >= 0)
    assert set(rows[:, 17].astype(np.int64).tolist()) >= {65535, 65536, 65537, 10**6, 2**24 + 1}
    want = comparator(ref, oracle_lib, "infer_max_qual_regs", rows)
    assert (want[:, 0] > 0).sum() > 10000 and (want[:, 0] == 0).sum() >= 1000
    assert_equal("infer_max_qual_regs", rows, probe("infer_max_qual_regs", rows), want)
    full = G.host_rows("infer_max_qual_regs", rows)
    assert_equal("infer_max_qual", full, probe("infer_max_qual", full), want)


# ---- binom_llr and what is built on it ----
def test_binom_llr(probe, ref, oracle_lib, exact):
    rows = G.binom_grid()
    assert len(rows) <= 2**21 + 2**17
    dev, want = probe("binom_llr", rows), comparator(ref, oracle_lib, "binom_llr", rows)
    # the branch (0 or not): the comparator's, except where a - A itself is a rounding away from 0
    p, a, b = (rows[:, k].astype(np.longdouble) for k in range(3))
    pe, ae, be = (p + G.EPS) / (1 + 2 * G.EPS), a + G.EPS, b + G.EPS
    A = pe * (ae + be)
    knife = np.abs(ae - A) <= 4 * FLOOR * np.abs(A)
    flip = (dev[:, 0] == 0) != (want[:, 0] == 0)
    print("binom_llr: %d rows, %d knife-edge rows of a - A (%.4f %%), %d branch differences" % (len(rows), int(knife.sum()), 100.0 * knife.mean(), int(flip.sum())))
    for i in np.flatnonzero(flip)[:20]:
        print("   %r: device %r comparator %r" % (rows[i].tolist(), dev[i, 0], want[i, 0]))
    assert knife.mean() <= CAP and not (flip & ~knife).any()
    scale = G.binom_terms(rows)
    sel = exact["binom_llr_rows"]
    assert np.array_equal(sel, G.binom_exact_rows(rows)) and ((rows[sel, 1] >= 1e3) | (rows[sel, 2] >= 1e3)).sum() == ((rows[:, 1] >= 1e3) | (rows[:, 2] >= 1e3)).sum() > 800
    error_bound("binom_llr", exact, "binom_llr", dev[:, 0], want[:, 0], scale, skip=flip | knife)   # (on a knife-edge row the exact value may be 0 where the comparator's is not)
    # two logarithms (2 each, weighed by their own term: 2 of the scale together), the two products, the sum and the factor 10 / ln 10 (1 each)
    close_everywhere("binom_llr", dev[:, 0], want[:, 0], scale, 6, skip=flip)


def test_het_lodq(probe, ref, oracle_lib, exact):
    rows = G.het_lodq_grid()
    knife_rows(exact, "het_lodq_binom", len(rows))
    want = comparator(ref, oracle_lib, "het_lodq", rows)
    assert (want[:, 0] == -2147483648.0).sum() > 1000 and (want[:, 0] > 0).sum() > 1000   # the NaN -> INT32_MIN path, and the ordinary one
    assert_equal("het_lodq", rows, probe("het_lodq", rows), want)


def test_normv_quals(probe, ref, oracle_lib):
    g1, g2 = G.normv_grids()
    for name, rows in (("normv_quals", g1), ("normv_quals2", g2)):
        want = comparator(ref, oracle_lib, name, rows)
        assert len(np.unique(want[:, 3])) > 50
        assert_equal(name, rows, probe(name, rows), want)


def test_dp4(probe, ref, oracle_lib, exact):
    rows = G.dp4_grid()
    dev, want = probe("dp4", rows), comparator(ref, oracle_lib, "dp4", rows)
    assert same(dev[:, 1], want[:, 1]).all()   # nobiasFA: sums and one quotient
    r = rows.astype(np.longdouble)
    frac = np.where(r[:, 1] != 0, 1, r[:, 2])
    adp, adf, dpp, dpf = (r[:, k] * frac + (r[:, 11] if k < 5 else r[:, 12]) for k in (3, 4, 5, 6))
    swap = (r[:, 0] != 0) & (adp / dpp >= adf / dpf)
    adp, adf, dpp, dpf = np.where(swap, adf, adp), np.where(swap, adp, adf), np.where(swap, dpf, dpp), np.where(swap, dpp, dpf)
    bdf, bdp = dpf * 2 - adf, dpp * 2 - adp
    apf, bpf = adp / (adp + adf), bdp / (bdp + bdf)
    key = (r[:, 0] == 0) & (r[:, 9] >= 0) & (r[:, 10] >= 0)
    with np.errstate(all="ignore"):
        apf = np.where(key, r[:, 9] / (r[:, 9] + r[:, 10] * np.longdouble(0.9)), apf); bpf = np.where(key, 1 - apf, bpf)
        terms = np.abs(adf * np.log((1 - apf) / (1 - bpf))) + np.where(r[:, 0] != 0, np.abs(adp * np.log(apf / bpf)), 0)
        terms = np.where(np.isfinite(terms), terms, 0)
    scale = np.abs(want[:, 0]).astype(np.longdouble) * np.maximum(1, (np.abs(r[:, 8]) + terms) / r[:, 7])
    # a row whose exact value took another branch than the comparator (a tie of the two fractions, infogain at n_nats): knife-edge
    ex = exact["dp4_0_hi"]; sel = exact["dp4_0_rows"]
    other = np.zeros(len(rows), bool)
    with np.errstate(all="ignore"):
        other[sel] = np.isfinite(ex) & np.isfinite(want[sel, 0]) & (np.abs(want[sel, 0] - ex) > 1e-9 * np.abs(scale[sel].astype(np.float64)))
    print("dp4: %d rows, %d sampled, %d of them on another branch than the exact value (%.4f %%)" % (len(rows), len(sel), int(other.sum()), 100.0 * other.sum() / len(sel)))
    assert other.sum() <= CAP * len(sel)
    assert np.array_equal(sel, G.dp4_exact_rows(rows))
    error_bound("dp4", exact, "dp4_0", dev[:, 0], want[:, 0], scale, skip=other)
    # infogain: logarithms 2, products and sum 2; (n_nats - infogain) / pl_exponent 1; the exponential 2; the product with the quotient 1
    close_everywhere("dp4", dev[:, 0], want[:, 0], scale, 8)


# ---- integer-valued primitives ----
def test_indel_phred(probe, ref, oracle_lib, exact):
    rows = G.indel_phred_grid()
    assert {8, 63, 64, 65} <= set((rows[:, 1] * rows[:, 2]).astype(int).tolist())
    knife_rows(exact, "indel_phred", len(rows))   # (slips + 1 == 10 exactly at ampfact 3, unit 4 x 14, and at 6, 2 x 37)
    assert_equal("indel_phred", rows, probe("indel_phred", rows), comparator(ref, oracle_lib, "indel_phred", rows))


INT_GRIDS = {
    "indel_len_rusize_phred": G.indel_len_grid, "more_STR": G.more_str_grid, "symbols_mutated": G.symbol_pairs, "sscs_phred": G.sscs_grid,
    "proton_cigarlen2phred": G.integers_0_4096, "i32_as_x86": G.i32_values,
    "numstates2deciphred": G.scalar_grid,   # (+-inf, NaN and -1 with the rest: INT32_MIN on both sides, the device's through i32_as_x86)
    "phred2nat": G.scalar_grid, "prob2odds": G.probabilities,
}


@pytest.mark.parametrize("name", sorted(INT_GRIDS))
def test_integer_and_plain_arithmetic_primitives(probe, ref, oracle_lib, exact, name):
    rows = INT_GRIDS[name]()
    if name == "numstates2deciphred":
        knife_rows(exact, name, len(rows))
    want = comparator(ref, oracle_lib, name, rows)
    assert len(np.unique(want[~np.isnan(want)])) >= 2
    assert_equal(name, rows, probe(name, rows), want)


# ---- double-valued primitives ----
def test_numstates2phred_logit2_norm_fa(probe, ref, oracle_lib, exact):
    for name, rows in (("numstates2phred", G.scalar_grid()), ("logit2", G.logit2_grid()), ("norm_fa", G.norm_fa_grid())):
        dev, want = probe(name, rows), comparator(ref, oracle_lib, name, rows)
        assert np.array_equal(np.isnan(dev), np.isnan(want)) and np.array_equal(np.isinf(dev), np.isinf(want)), name
        scale = np.abs(want[:, 0])
        if name == "logit2":   # log(p / (1 - p)) = log p - log(1 - p): the sum of the absolute terms
            pr = (rows[:, 0].astype(np.longdouble) + G.EPS) / (rows[:, 0].astype(np.longdouble) + rows[:, 1] + 2 * G.EPS)
            with np.errstate(all="ignore"):
                scale = np.abs(np.log(pr)) + np.abs(np.log1p(-pr))
        error_bound(name, exact, name, dev[:, 0], want[:, 0], scale)
        # one logarithm (2); numstates2phred multiplies it once more (1); norm_fa is IEEE arithmetic alone, the same on both sides (0)
        close_everywhere(name, dev[:, 0], want[:, 0], np.abs(want[:, 0]), {"numstates2phred": 3, "logit2": 2, "norm_fa": 0}[name])
        if name == "logit2":
            assert np.array_equal(exact["logit2_rows"], G.logit2_exact_rows(rows))


def test_phred2prob_with_and_without_the_table(probe, ref, oracle_lib, exact):
    rows = np.arange(-40.0, 301.0).reshape(-1, 1)
    plain, tab = probe(["phred2prob", "phred2prob_tab"], rows)
    want = comparator(ref, oracle_lib, "phred2prob", rows)
    assert same(plain, tab).all()   # the table holds what the expression gives; outside 0..127 the expression itself
    stored = exact["phred2prob_rows"]
    off = int(-rows[0, 0])
    sub = lambda v: v[off:off + len(stored), 0]
    assert np.array_equal(rows[off:off + len(stored), 0], stored.astype(np.float64))
    ex = dict(phred2prob_rows=np.arange(len(stored)), phred2prob_hi=exact["phred2prob_hi"], phred2prob_lo=exact["phred2prob_lo"])
    error_bound("phred2prob", ex, "phred2prob", sub(plain), sub(want), np.abs(sub(want)))
    assert (np.abs(plain - want) <= 4 * np.spacing(np.abs(want))).all()   # the rows outside the stored range
