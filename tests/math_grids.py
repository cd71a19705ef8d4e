"""The grids of the scalar-math tests (tests/test_ref_math_cpu.py, tests/test_gpu_math_probe.py, tests/golden/make_math_exact.py) and the one
calling convention behind them: every primitive, in the reference checker (oracle/_ref/libref_math.so), in the oracle (liboracle.so,
uvc_oracle_math_*) and in the device probe (uvc_launch_math_probe), takes n rows of n_in doubles and fills n rows of n_out doubles.
Integer arguments and results travel as doubles (all below 2^31, so exactly)."""
import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_math.so")
EXACT_NPZ = os.path.join(ROOT, "tests", "golden", "math_exact.npz")
EPS = 2.220446049250313e-16
K10 = 10.0 / math.log(10.0)

# name -> probe op (UvcProbeOp of uvc_launch.h, None: host only), arguments, results, symbol in libref_math.so (None: a main.hpp function,
# which cannot be compiled), symbol in liboracle.so
Op = namedtuple("Op", "probe n_in n_out ref oracle")
OPS = {
    "phred2nat": Op(0, 1, 1, "ref_phred2nat", "uvc_oracle_math_phred2nat"),
    "numstates2phred": Op(1, 1, 1, "ref_numstates2phred", "uvc_oracle_math_numstates2phred"),
    "numstates2deciphred": Op(2, 1, 1, "ref_numstates2deciphred", "uvc_oracle_math_numstates2deciphred"),
    "prob2odds": Op(3, 1, 1, "ref_prob2odds", "uvc_oracle_math_prob2odds"),
    "logit2": Op(4, 2, 1, "ref_logit2", "uvc_oracle_math_logit2"),
    "binom_llr": Op(5, 3, 1, "ref_binom_llr", "uvc_oracle_math_binom_llr"),     # host side: 5 arguments (the two template flags behind)
    "dp4": Op(6, 13, 2, "ref_dp4", "uvc_oracle_math_dp4"),
    "indel_len_rusize_phred": Op(7, 2, 1, None, "uvc_oracle_math_indel_len_rusize_phred"),
    "indel_phred": Op(8, 3, 1, None, "uvc_oracle_math_indel_phred"),
    "more_STR": Op(9, 5, 1, None, "uvc_oracle_math_more_STR"),
    "norm_fa": Op(10, 2, 1, None, "uvc_oracle_math_norm_fa"),
    "i32_as_x86": Op(11, 1, 1, None, "uvc_oracle_math_i32_cast"),
    "het_lodq": Op(12, 4, 1, None, "uvc_oracle_math_het_lodq"),
    "normv_quals": Op(13, 11, 4, None, "uvc_oracle_math_normv_quals"),
    "normv_quals2": Op(14, 7, 4, None, "uvc_oracle_math_normv_quals2"),
    "symbols_mutated": Op(15, 2, 1, "ref_symbols_mutated", "uvc_oracle_math_symbols_mutated"),
    "sscs_phred": Op(16, 9, 1, None, "uvc_oracle_math_sscs_phred"),
    "infer_max_qual": Op(17, 19, 3, "ref_infer_max_qual", "uvc_oracle_math_infer_max_qual"),
    "infer_max_qual_regs": Op(18, 18, 3, "ref_infer_max_qual", None),             # host side: the 19-argument row with dec_qual = 1
    "infer_max_qual_one": Op(19, 5, 3, "ref_infer_max_qual_one", "uvc_oracle_math_infer_max_qual_one"),
    "infer_max_qual_regs_one": Op(20, 5, 3, "ref_infer_max_qual_one", None),     # host side: the same row with dec_qual = 1
    "proton_cigarlen2phred": Op(21, 1, 1, "ref_proton_cigarlen2phred", "uvc_oracle_math_proton_cigarlen2phred"),
    "phred2prob": Op(22, 1, 1, "ref_phred2prob", "uvc_oracle_math_phred2prob"),
    "phred2prob_tab": Op(23, 1, 1, "ref_phred2prob", "uvc_oracle_math_phred2prob"),
    # host only
    "odds2prob": Op(None, 1, 1, "ref_odds2prob", "uvc_oracle_math_odds2prob"),
    "logit": Op(None, 1, 1, "ref_logit", "uvc_oracle_math_logit"),
    "non_neg_minus": Op(None, 2, 1, "ref_non_neg_minus", "uvc_oracle_math_non_neg_minus"),
    "non_neg_minus_i64": Op(None, 2, 1, "ref_non_neg_minus_i64", "uvc_oracle_math_non_neg_minus_i64"),
    "calc_non_negative_float": Op(None, 1, 1, "ref_calc_non_negative_float", "uvc_oracle_math_calc_non_negative_float"),
    "prob2phred": Op(None, 1, 1, "ref_prob2phred", "uvc_oracle_math_prob2phred"),
    "prob2realphred": Op(None, 1, 1, "ref_prob2realphred", "uvc_oracle_math_prob2realphred"),
    "symbol_kind": Op(None, 1, 3, "ref_symbol_kind", "uvc_oracle_math_symbol_kind"),
    "len_to_symbol": Op(None, 1, 2, "ref_len_to_symbol", "uvc_oracle_math_len_to_symbol"),
}


def rows_of(a, n_in):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(-1, n_in)


def call_host(dll, symbol, rows, n_out):
    """One call of a grid-shaped host function: rows [n, n_in] -> [n, n_out]."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    out = np.full((rows.shape[0], n_out), np.nan)
    fn = getattr(dll, symbol)
    fn.restype, fn.argtypes = None, [C.c_int64, C.c_void_p, C.c_void_p]
    if rows.shape[0]:
        fn(rows.shape[0], rows.ctypes.data, out.ctypes.data)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_rows(name, rows):
    """The row a host function takes for the row the probe op `name` takes."""
    rows = np.asarray(rows, dtype=np.float64)
    if name == "binom_llr":
        return np.hstack([rows, np.zeros((len(rows), 2))])
    if name == "infer_max_qual_regs":
        return np.hstack([rows[:, :17], np.ones((len(rows), 1)), rows[:, 17:18]])
    return rows


# ---- scalar arguments ----
def integers_0_4096():
    return np.arange(0, 4097, dtype=np.float64).reshape(-1, 1)


def log_spaced_doubles():
    return np.power(10.0, np.linspace(-300.0, 300.0, 4096)).reshape(-1, 1)


def edge_doubles():
    return np.array([0.0, 5e-324, 2.2250738585072014e-308 / 4, 2.2250738585072014e-308, np.inf, -np.inf, np.nan, -0.0, -1.0, 1.0]).reshape(-1, 1)


def scalar_grid(positive_only=False):
    g = np.vstack([integers_0_4096(), log_spaced_doubles(), edge_doubles()])
    return g[~(g[:, 0] < 0)] if positive_only else g


def probabilities():
    """prob2odds / logit: inside (0, 1), its ends, and what lies around 1/2"""
    return np.concatenate([np.linspace(0.0, 1.0, 4097), 1.0 - np.power(10.0, -np.arange(1, 17.0)), np.power(10.0, -np.arange(1, 300.0, 7)), [0.5 - EPS, 0.5 + EPS, np.nan]]).reshape(-1, 1)


def i32_values():
    edge = [2147483647.0, 2147483647.5, 2147483648.0, 2147483649.0, -2147483648.0, -2147483648.5, -2147483648.9999995, -2147483649.0, -2147483650.0, 4294967296.0, 1e19, -1e19, 0.5, -0.5, 0.99999, -0.99999]
    r = np.random.default_rng(11)
    return np.concatenate([scalar_grid()[:, 0], -scalar_grid()[:, 0], edge, r.uniform(-3e9, 3e9, 4096)]).reshape(-1, 1)


# ---- binom_llr and what is built on it ----
GERMLINE_FRACTIONS = (0.47, 1.0 - 0.47, 0.02, 0.05)   # germ_hetero_FA and its complement, contam_any_mul_frac, contam_t2n_mul_frac of the default parameters
PROBS = (1e-9, 1e-3, 0.02, 0.1, 0.5, 0.9, 1.0 - 1e-9) + GERMLINE_FRACTIONS
BIG = (1e3, 1e4, 1e5, 1e6, 3e6)


def ab_pairs(step=1):
    """(a, b): the integer counts 0..300 crossed, the large values crossed with each other and with a few counts, the centi-read values"""
    c = np.arange(0, 301, step, dtype=np.float64)
    big = np.array(BIG)
    few = np.array([0.0, 1.0, 2.0, 10.0, 300.0])
    cen = np.arange(0, 301, max(3, step), dtype=np.float64) / 100.0
    parts = [np.stack(np.meshgrid(x, y, indexing="ij"), -1).reshape(-1, 2) for x, y in ((c, c), (big, big), (big, few), (few, big), (cen, cen))]
    return np.vstack(parts)


def binom_grid(step=1):
    """prob, a, b: every probability with every pair, and per probability the line a == prob * (a + b), where the branch flips"""
    ab = ab_pairs(step)
    out = []
    for p in PROBS:
        out.append(np.hstack([np.full((len(ab), 1), p), ab]))
        tot = np.concatenate([np.arange(1, 301, 3, dtype=np.float64), BIG])   # (every third total: these rows are knife-edge by construction, and a grid may hold 0.2 % of them)
        a = p * tot
        out.append(np.stack([np.full(len(tot), p), a, tot - a], -1))
    return np.vstack(out)


def even_sample(n, k):
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(np.int64))


def binom_exact_rows(rows):
    """the rows of binom_grid() whose exact value is stored: every row with a large count, every row on the line a == prob * (a + b), the
    edges a == 0 and b == 0 and the centi-read values thinned, and an even sample of everything"""
    p, a, b = rows[:, 0], rows[:, 1], rows[:, 2]
    big = np.flatnonzero((a >= 1e3) | (b >= 1e3))
    with np.errstate(all="ignore"):
        line = np.flatnonzero(np.abs(a - p * (a + b)) <= 4 * 2.0 ** -52 * np.abs(p * (a + b)))
    edge = np.flatnonzero((a == 0) | (b == 0))[::5]
    centi = np.flatnonzero((a != np.floor(a)) | (b != np.floor(b)))[::40]
    return np.unique(np.concatenate([big, line, edge, centi, even_sample(len(rows), 5000)]))


def logit2_exact_rows(rows):
    """logit2_grid(): every row with a large or a tiny argument thinned to a third, and an even sample"""
    a, b = rows[:, 0], rows[:, 1]
    ends = np.flatnonzero((a >= 1e3) | (b >= 1e3) | ((a < 0.5) & (b < 0.5)))[::3]
    return np.unique(np.concatenate([ends, even_sample(len(rows), 3000)]))


def dp4_exact_rows(rows):
    """dp4_grid(): every 48th row with a depth of 1e4 or 1e6 or a half read, and an even sample (which meets every form, every prior and
    both exponents: they change in blocks of the grid)"""
    v = rows[:, 3:7]
    special = np.flatnonzero((v >= 1e4).any(axis=1) | (v == 0.5).any(axis=1))[::48]
    return np.unique(np.concatenate([special, even_sample(len(rows), 3000)]))


def binom_terms(rows):
    """scale of the final sum of binom_llr: 10 / ln 10 * (|a log(a / A)| + |b log(b / B)|), in extended precision"""
    p, a, b = (rows[:, k].astype(np.longdouble) for k in range(3))
    p = (p + EPS) / (1 + 2 * EPS); a = a + EPS; b = b + EPS
    A, B = p * (a + b), (1 - p) * (a + b)
    return np.longdouble(K10) * (np.abs(a * np.log(a / A)) + np.abs(b * np.log(b / B)))


def het_lodq_grid():
    """a1, a2, expfrac, powlaw_exponent: expfrac outside (0, 1) makes the logarithms NaN -> INT32_MIN"""
    ab = ab_pairs(step=4)
    out = []
    for e in (0.47, 0.53, 0.5, 0.0, 1.0, 1.5, -0.1):
        for pl in (3.0, 5.4):
            out.append(np.hstack([ab, np.full((len(ab), 1), e), np.full((len(ab), 1), pl)]))
    return np.vstack(out)


def normv_grids():
    """(normv_quals rows, normv_quals2 rows): depths as the callers pass them, (count + 0.5) / 100 over (count + 1) / 100"""
    r = np.random.default_rng(23)
    cnt = np.concatenate([np.arange(0, 301), [1000, 10000, 100000, 1000000, 3000000]])
    n = 60000
    tAD = r.choice(cnt, n); tDP = tAD + r.choice(cnt, n); nAD = r.choice(cnt, n); nDP = nAD + r.choice(cnt, n)
    tVQ = r.integers(0, 200, n); cap = r.integers(0, 200, n); nVQ = r.integers(0, 200, n)
    add = r.choice([0.0, 0.02, 1.0], n)
    base = [(tAD + 0.5) / 100.0, (tDP + 1.0) / 100.0, tVQ, cap, (nAD + 0.5) / 100.0 + add, (nDP + 1.0) / 100.0 + add, nVQ]
    coef = r.choice([8.0, 4.0, 16.0], n); prior = r.choice([31, 20, 0], n); xm = r.choice([0, 5, 30], n); pl = r.choice([3.0, 5.4], n)
    g2 = np.stack(base, -1).astype(np.float64)
    g1 = np.hstack([g2, np.stack([coef, prior, xm, pl], -1)])
    # whole counts too (the first pair of calls in the tumor / normal step rounds nothing)
    g2w = g2.copy(); g2w[:, 0] = tAD; g2w[:, 1] = np.maximum(tDP, 1); g2w[:, 4] = nAD; g2w[:, 5] = np.maximum(nDP, 1)
    g1w = np.hstack([g2w, g1[:, 7:]])
    return np.vstack([g1, g1w]), np.vstack([g2, g2w])


def dp4_grid():
    """bidir, overseq_disabled, overseq_frac, ADpass, ADfail, DPpass, DPfail, pl_exponent, n_nats, ADkey, DPkey, priorAD, priorDP"""
    v = (0.0, 0.5, 1.0, 2.0, 10.0, 100.0, 1e4, 1e6)
    cells = [(ap, af, dp, df) for ap in v for af in v for dp in v for df in v if ap <= dp and af <= df]
    out = []
    for bidir in (0, 1):
        for dis in (0, 1):
            for frac in ((0.01, 0.5, 1.0) if not dis else (-1.0,)):
                for pl, nn in ((3.0, math.log(501.0)), (5.4, math.log(501.0)), (3.0, math.log(10.0) / 10.0 * 31), (5.4, math.log(10.0) / 10.0 * 20)):
                    for key in ((-1.0, -1.0, 0.5, 1.0), (30.0, 70.0, 0.5, 1.0), (0.0, 12.5, 0.25, 0.5), (150.0, 0.0, 0.25, 0.5)):
                        c = np.array(cells)
                        out.append(np.hstack([np.tile([bidir, dis, frac], (len(c), 1)), c, np.tile([pl, nn] + list(key), (len(c), 1))]))
    return np.vstack(out)


# indel_polymerase_slip_rate alone and times indel_del_to_ins_err_ratio: the defaults (8, 8 x 5), test_gpu_rtr.test_other_parameters (3, 3 x 2),
# tests/param_moves.py (13.9 x 5)
INDEL_AMPFACTS = (8.0, 40.0, 3.0, 6.0, 69.5)


def indel_phred_grid():
    return np.array([(amp, rs, rn) for amp in INDEL_AMPFACTS for rs in range(1, 7) for rn in range(1, 41)], dtype=np.float64)


def indel_len_grid():
    return np.array([(ln, rs) for ln in range(0, 101) for rs in range(1, 21)], dtype=np.float64)


def more_str_grid():
    return np.array([(l1, c1, l2, c2, mx) for l1 in range(0, 9) for c1 in range(0, 6) for l2 in range(0, 9) for c2 in range(0, 6) for mx in (6, 4, 2)], dtype=np.float64)


def norm_fa_grid():
    fa = np.concatenate([np.linspace(0, 1, 257), np.power(10.0, -np.arange(1, 12.0))])
    rb = np.array([0.0, 0.01, 0.1, 0.25, 0.5, 1.0, 2.0, 10.0])
    return np.stack(np.meshgrid(fa, rb, indexing="ij"), -1).reshape(-1, 2)


def logit2_grid():
    c = np.concatenate([np.arange(0, 200.0), np.arange(0, 200.0) + 0.5, BIG, np.power(10.0, -np.arange(1, 16.0))])
    return np.stack(np.meshgrid(c, c, indexing="ij"), -1).reshape(-1, 2)


def symbol_pairs():
    return np.array([(r, a) for r in range(14) for a in range(14)], dtype=np.float64)


def sscs_grid():
    dflt = (60, 5, 44, 48, 52, 56)
    other = (11, 3, 21, 25, 33, 37)
    return np.array([(c, a) + p + (t,) for c in range(14) for a in range(14) for p in (dflt, other) for t in (0, 1)], dtype=np.float64)


# ---- infer_max_qual ----
MAX_QUALS = (1, 2, 15, 16, 17, 37, 45, 93)
DEC_QUALS_GENERIC = (2, 3, 5)
ONE_N = 2048


def one_bucket_pairs():
    """(currAD, totDP) for every 1 <= currAD <= totDP <= 2048: 2 098 176 pairs"""
    dp = np.repeat(np.arange(1, ONE_N + 1), np.arange(1, ONE_N + 1))
    ad = np.arange(len(dp)) - (dp * (dp - 1)) // 2 + 1
    return ad.astype(np.float64), dp.astype(np.float64)


def one_bucket_rows(max_qual, dec_qual, idx=0):
    ad, dp = one_bucket_pairs()
    n = len(ad)
    return np.stack([np.full(n, float(idx)), ad, np.full(n, float(max_qual)), np.full(n, float(dec_qual)), dp], -1)


def infer_pre(ad, dp, bq):
    """the value infer_max_qual truncates, currAD * (currBQ - 10 / ln 10 * log(totDP / currAD + eps)), in extended precision"""
    ad, dp = np.asarray(ad, np.longdouble), np.asarray(dp, np.longdouble)
    return ad * (np.longdouble(bq) - np.longdouble(10) / np.log(np.longdouble(10)) * np.log(dp / ad + np.longdouble(EPS)))


def _val(ad, dp, bq):
    return float(ad) * (bq - K10 * math.log(dp / float(ad) + EPS))


# (totDP, max_qual, first bucket, second bucket, count of the first, count of the second): two buckets whose exact values truncate to the same
# number, the first the smaller -- so the first wins -- at the largest magnitudes the single-precision pass of infer_max_qual_regs sees
# (values of 3 to 4 million, where a float resolves 0.25): the single-precision value of the second comes out 1.25 to 1.5 above that of the
# first.  Found by an exhaustive search over the second bucket's cumulative depth with the pass restated in numpy float32; they are what
# separates the window of that pass from a window of 1.
WINDOW_CASES = (
    (45289, 93, 1, 4, 43576, 1402), (47515, 93, 0, 9, 40557, 4154), (48893, 93, 2, 6, 45039, 1978), (49158, 93, 5, 9, 43192, 1966),
    (50000, 93, 0, 2, 42860, 905), (50000, 93, 0, 10, 39853, 4602), (50000, 93, 0, 12, 42784, 6043), (50000, 93, 2, 14, 34719, 5077),
    (50000, 93, 5, 9, 39283, 1798), (50000, 93, 6, 15, 39976, 4409), (50589, 93, 0, 5, 45039, 2449), (53080, 93, 2, 7, 46111, 2566),
    (53239, 93, 4, 15, 41364, 5581), (54246, 93, 0, 6, 41708, 2770), (55359, 93, 4, 15, 39027, 5293), (56154, 93, 1, 11, 45465, 5307),
    (56419, 93, 0, 12, 43226, 6140), (56631, 93, 4, 11, 46037, 3764), (57426, 93, 4, 13, 47531, 5108), (57479, 93, 5, 13, 47454, 4535),
    (58645, 93, 5, 12, 45068, 3739), (59652, 93, 2, 6, 41163, 1833), (60000, 45, 1, 12, 42826, 12915), (60000, 93, 0, 4, 42040, 1830),
    (60000, 93, 1, 14, 37765, 6012), (60000, 93, 1, 15, 34754, 6057), (60000, 93, 2, 10, 42833, 3981), (60000, 93, 4, 5, 39098, 432),
    (60000, 93, 4, 8, 46972, 2126), (60000, 93, 6, 7, 45941, 515), (60000, 93, 6, 10, 48356, 2236), (60288, 93, 1, 14, 42931, 6790),
    (60288, 93, 3, 14, 46179, 6160), (61401, 93, 0, 9, 39906, 4143), (61560, 93, 3, 9, 45552, 3135), (62461, 93, 4, 5, 44730, 492),
    (63945, 93, 1, 4, 44897, 1466), (63945, 93, 3, 12, 47020, 5024), (64263, 93, 5, 7, 43086, 972), (65000, 93, 0, 2, 44529, 950),
    (65000, 93, 2, 8, 43922, 3002), (65000, 93, 2, 10, 46190, 4294), (65000, 93, 2, 11, 44637, 4730), (65000, 93, 5, 9, 47616, 2187),
    (65000, 93, 5, 10, 46190, 2686), (65000, 93, 6, 15, 39709, 4443), (65000, 93, 7, 8, 42629, 487), (65000, 93, 7, 14, 45483, 3884),
    (65376, 93, 5, 9, 48014, 2205), (65535, 93, 1, 13, 36105, 5280), (65535, 93, 2, 9, 42239, 3414), (65535, 93, 2, 11, 39177, 4181),
    (65535, 93, 3, 4, 41966, 459), (65535, 93, 6, 11, 37554, 2234),
)


def adversarial_histograms(n_total=20000, seed=77):
    """Seeded histograms for infer_max_qual_regs in named classes -> (rows [n, 18]: 16 counts, max_qual, totDP; class name per row).
    The classes are made by search over cumulative depths, with the double-precision value of a bucket as the guide."""
    r = np.random.default_rng(seed)
    rows, names = [], []
    TOT = (65535, 65536, 65537, 10**6, 2**24 + 1)

    def emit(name, h, mq, dp):
        rows.append(list(h) + [mq, dp]); names.append(name)

    def rand_hist(mq, dp, nb, lead=0):
        """nb filled buckets from index `lead` on, cumulative depth <= dp"""
        h = [0] * 16
        idxs = sorted(r.choice(np.arange(lead, 16), size=min(nb, 16 - lead), replace=False).tolist())
        left = dp
        for k, i in enumerate(idxs):
            c = int(r.integers(1, max(2, left // (len(idxs) - k) + 1)))
            c = min(c, left)
            if c <= 0:
                break
            h[i] = c; left -= c
        return h

    def vals(ad, dp, bq):
        ad = np.asarray(ad, dtype=np.float64)
        return ad * (bq - K10 * np.log(dp / ad + EPS))

    per = n_total // 10
    # 1. two and three buckets whose exact values differ by less than 1: the second bucket's count by search
    # 2. ties after truncation: the same search, kept where (int) of both values agree
    for name in ("near", "tie"):
        cnt = 0
        while cnt < per:
            mq = int(r.choice([17, 20, 37, 45, 60, 93])); dp = int(r.choice([50, 200, 1000, 5000, 40000, 65535]))
            i0 = int(r.integers(0, 8)); i1 = int(r.integers(i0 + 1, 16))
            a0 = int(r.integers(1, max(2, dp // 3)))
            v0 = _val(a0, dp, mq - i0)
            if i1 >= mq or v0 < 1:
                continue
            a1 = np.arange(1, dp - a0 + 1) if dp <= 5000 else r.integers(1, dp - a0 + 1, 4096)
            v1 = vals(a0 + a1, dp, mq - i1)
            ok = np.flatnonzero((np.abs(v1 - v0) < 1.0) if name == "near" else (np.trunc(v1) == math.trunc(v0)))
            if not len(ok):
                continue
            k = int(ok[r.integers(0, len(ok))])
            h = [0] * 16; h[i0] = a0; h[i1] = int(a1[k])
            used = a0 + int(a1[k])
            if name == "near" and cnt % 3 == 0 and i1 + 1 < min(16, mq) and used < dp:   # a third bucket close to both
                i2 = int(r.integers(i1 + 1, min(16, mq)))
                a2 = np.arange(1, dp - used + 1) if dp <= 5000 else r.integers(1, dp - used + 1, 4096)
                ok2 = np.flatnonzero(np.abs(vals(used + a2, dp, mq - i2) - v0) < 1.0)
                if len(ok2):
                    h[i2] = int(a2[ok2[0]])
            emit(name, h, mq, dp); cnt += 1
    # 3. a candidate 16, 17 and 18 (to within 3/4) above or below another: the distances around the window of the single-precision pass
    for gap in (16, 17, 18):
        cnt = 0
        while cnt < per // 2:
            mq = int(r.choice([20, 37, 45, 93])); dp = int(r.choice([1000, 3000, 5000]))
            i0 = int(r.integers(0, 6)); i1 = int(r.integers(i0 + 1, 16))
            a0 = int(r.integers(5, max(6, dp // 4)))
            v0 = _val(a0, dp, mq - i0)
            if i1 >= mq or v0 < gap + 2:
                continue
            a1 = np.arange(1, dp - a0 + 1)
            d = vals(a0 + a1, dp, mq - i1) - v0
            ok = np.flatnonzero(np.abs(np.abs(d) - gap) < 0.75)
            if not len(ok):
                continue
            h = [0] * 16; h[i0] = a0; h[i1] = int(a1[ok[r.integers(0, len(ok))]])
            emit("gap%d" % gap, h, mq, dp); cnt += 1
    # 4. all values <= 0: qualities below the expected one
    cnt = 0
    while cnt < per // 2:
        mq = int(r.choice([1, 2, 5, 10, 16])); dp = int(r.choice([1000, 65535, 10**6]))
        h = rand_hist(mq, dp // 1000 + 1, int(r.integers(1, 5)))
        if all(_val(sum(h[:i + 1]), dp, mq - i) <= 0 for i in range(min(16, mq)) if h[i]):
            emit("nonpositive", h, mq, dp); cnt += 1
    # 5. leading and trailing empty buckets
    for cnt in range(per):
        mq = int(r.choice([17, 37, 45, 93])); dp = int(r.choice([30, 3000, 65535]))
        lead = int(r.integers(1, 12))
        h = rand_hist(mq, dp, int(r.integers(1, 4)), lead=lead)
        last = max(i for i in range(16) if h[i]) if any(h) else 15
        if cnt % 2:
            for i in range(min(last + 1, 13), 16):
                h[i] = 0
        emit("empty_ends", h, mq, dp)
    # 6. max_qual below, at and above 16 (buckets at and past max_qual are not read)
    for cnt in range(per):
        mq = int(r.choice([1, 3, 8, 14, 15, 16, 17, 18, 30]))
        dp = int(r.choice([20, 500, 65535]))
        emit("max_qual", rand_hist(mq, dp, int(r.integers(1, 17))), mq, dp)
    # 7. the depths around the switch of the single-precision pass and far above it
    for cnt in range(per):
        dp = TOT[cnt % len(TOT)]; mq = int(r.choice([16, 17, 37, 45, 93]))
        emit("totDP", rand_hist(mq, dp if cnt % 3 else min(dp, int(r.integers(1, 70000))), int(r.integers(1, 17))), mq, dp)
    # 8. currAD up to totDP
    for cnt in range(per):
        dp = int(r.choice([1, 2, 17, 4096, 65535, 65536, 10**6])); mq = int(r.choice([16, 37, 93]))
        h = rand_hist(mq, dp, int(r.integers(1, 6)))
        i = max([k for k in range(16) if h[k]] + [0])
        h[i] += dp - sum(h)
        emit("full_depth", h, mq, dp)
    # 9. the ties at the largest magnitudes
    for (dp, mq, i0, i1, a0, a1) in WINDOW_CASES:
        h = [0] * 16; h[i0] = a0; h[i1] = a1
        emit("window", h, mq, dp)
    # 10. plain random histograms for the rest
    while len(rows) < n_total:
        mq = int(r.integers(1, 94)); dp = int(r.integers(1, 70000))
        emit("random", rand_hist(mq, dp, int(r.integers(1, 17))), mq, dp)
    return np.array(rows[:n_total], dtype=np.float64), np.array(names[:n_total])


ADVERSARIAL_MIN = {"near": 2000, "tie": 2000, "gap16": 1000, "gap17": 1000, "gap18": 1000, "nonpositive": 1000, "empty_ends": 2000, "max_qual": 2000,
                   "totDP": 2000, "full_depth": 2000, "window": 54, "random": 1}
