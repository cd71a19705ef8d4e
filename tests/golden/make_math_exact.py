"""Writes tests/golden/math_exact.npz: what tests/test_gpu_math_probe.py needs to know exactly, computed with 50-digit mpmath.

  python tests/golden/make_math_exact.py        (some minutes; needs mpmath, no library of the project and no GPU)

Two kinds of entries, keyed by the grid's name (the grids themselves are made by tests/math_grids.py, never stored):
  * integer-valued primitives -- <key>_idx, <key>_dist, <key>_cmp_err: the rows whose value in front of the truncation (or rounding) lies
    within NEAR of a breakpoint (found in 80-bit arithmetic, which errs by 1e-14 at most on these magnitudes), the exact signed distance
    to that breakpoint, and the largest error of the same expression evaluated in double precision -- written out here in Python, operation
    for operation what the comparator evaluates, with math.log / math.exp / math.log1p, which are the C library's own functions -- over those
    rows and an even sample of the grid (not over the whole grid: mpmath on two million rows is out of reach, and the rows near a breakpoint
    are all in).  The comparator itself returns only the truncated value, so its error in front of the truncation cannot be read from it.
    The test calls a row knife-edge when |dist| < 4 * cmp_err.
  * double-valued primitives -- <key>_rows, <key>_hi, <key>_lo: the rows math_grids.<key>_exact_rows picks (every large count, every row on a
    branch line, the edges, and an even sample; all of a small grid) and the exact result as an unevaluated sum of two doubles.
The stored adversarial histograms of infer_max_qual_regs (adv_rows, adv_class) are math_grids.adversarial_histograms() as it stands: the
search that makes them takes seconds, a test should not; tests/test_ref_math_cpu.py checks on every run that the generator still makes them."""
import math
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import math_grids as G   # noqa: E402

mp.mp.dps = 50
NEAR = 1e-6
EPS = mp.mpf(G.EPS)
LN10 = mp.log(10)
out = {}


def split(x):
    hi = float(x)
    if not math.isfinite(hi):
        return hi, 0.0
    return hi, float(x - mp.mpf(hi))


def sample(n, k):
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(np.int64))


def store_int(key, idx, exact_pre, double_pre, breakpoint_of, trunc_to_zero=False):
    """idx: candidate rows (near rows and the sample); exact_pre / double_pre: per candidate"""
    dist = np.array([float(e - breakpoint_of(e)) for e in exact_pre])
    err = max([abs(float(e - mp.mpf(d))) for e, d in zip(exact_pre, double_pre) if math.isfinite(d)] + [0.0])
    near = (np.abs(dist) < NEAR) & np.array([not (trunc_to_zero and abs(e) < 0.5) for e in exact_pre])   # ((int)v has no breakpoint at 0)
    out[key + "_idx"] = np.asarray(idx, np.int64)[near].astype(np.int32); out[key + "_dist"] = dist[near]; out[key + "_cmp_err"] = np.float64(err)
    print(key, "near", int(near.sum()), "cmp_err", err, "knife", int((np.abs(dist[near]) < 4 * err).sum()))


def nearest_int(e):
    return mp.nint(e)


def nearest_half(e):
    return mp.floor(e) + mp.mpf(0.5)


# ---- infer_max_qual, one bucket: v = currAD * (currBQ - 10 / ln 10 * log(totDP / currAD + eps)), truncated ----
ad, dp = G.one_bucket_pairs()
for bq in G.MAX_QUALS:
    v = G.infer_pre(ad, dp, bq)
    cand = np.union1d(np.flatnonzero(np.abs(v - np.rint(v)) < NEAR), sample(len(ad), 2000))
    ex = [mp.mpf(int(ad[i])) * (bq - 10 / LN10 * mp.log(mp.mpf(int(dp[i])) / mp.mpf(int(ad[i])) + EPS)) for i in cand]
    db = [ad[i] * (bq - 10.0 / math.log(10.0) * math.log(dp[i] / ad[i] + G.EPS)) for i in cand]
    store_int("infer_one_%d" % bq, cand, ex, db, nearest_int, trunc_to_zero=True)

# ---- numstates2deciphred: round(100 / ln 10 * log(x)) ----
g = G.scalar_grid()[:, 0]
ok = np.flatnonzero(np.isfinite(g) & (g > 0))
ex = [100 / LN10 * mp.log(mp.mpf(float(g[i]))) for i in ok]
db = [(100.0 / math.log(10.0)) * math.log(g[i]) for i in ok]
store_int("numstates2deciphred", ok, ex, db, nearest_half)

# ---- indel_phred: floor(-10 log((1 - eps) / (slips + 1)) / log 10) ----
g = G.indel_phred_grid()
ex, db = [], []
for amp, rs, rn in g.tolist():
    size = int(rs * rn)
    slips = (mp.mpf(size - 8) if size > 64 else mp.log1p(mp.exp(mp.mpf(size - 8)))) * mp.mpf(amp) / (rs * rs)
    ex.append(-10 * mp.log((1 - EPS) / (slips + 1)) / LN10)
    s = ((size - 8.0) if size > 64 else math.log1p(math.exp(size - 8.0))) * amp / (rs * rs)
    db.append(-10 * math.log((1.0 - G.EPS) / (s + 1.0)) / math.log(10.0))
store_int("indel_phred", np.arange(len(g)), ex, db, nearest_int)


# ---- binom_llr: the value (double-valued) and, for het_lodq, its distance to a whole number ----
def binom_exact(p, a, b):
    p = (mp.mpf(p) + EPS) / (1 + 2 * EPS); a = mp.mpf(a) + EPS; b = mp.mpf(b) + EPS
    A, B = p * (a + b), (1 - p) * (a + b)
    return (10 / LN10 * (a * mp.log(a / A) + b * mp.log(b / B))) if a > A else mp.mpf(0)


def store_double(key, rows_idx, exact):
    hl = np.array([split(e) for e in exact])
    out[key + "_rows"] = np.asarray(rows_idx, np.int32); out[key + "_hi"] = hl[:, 0]; out[key + "_lo"] = hl[:, 1]
    print(key, len(rows_idx), "rows")


g = G.binom_grid()
idx = G.binom_exact_rows(g)
store_double("binom_llr", idx, [binom_exact(*g[i]) for i in idx])

g = G.logit2_grid()
idx = G.logit2_exact_rows(g)
store_double("logit2", idx, [mp.log(((mp.mpf(a) + EPS) / (mp.mpf(a) + mp.mpf(b) + 2 * EPS)) / (1 - (mp.mpf(a) + EPS) / (mp.mpf(a) + mp.mpf(b) + 2 * EPS))) for a, b in g[idx].tolist()])

g = G.scalar_grid()[:, 0]
idx = np.flatnonzero(np.isfinite(g) & (g > 0))[::2]
store_double("numstates2phred", idx, [10 / LN10 * mp.log(mp.mpf(float(g[i]))) for i in idx])

g = G.norm_fa_grid()
store_double("norm_fa", np.arange(len(g)), [(mp.mpf(f) + mp.mpf(f) * mp.mpf(r)) / (mp.mpf(f) + (1 - mp.mpf(f)) / (1 + mp.mpf(r)) + mp.mpf(f) * mp.mpf(r)) for f, r in g.tolist()])

q = np.arange(0, 301)
store_double("phred2prob", q, [mp.power(10, mp.mpf(float(-np.float32(v) / np.float32(10)))) for v in q])   # (the exponent is the float quotient the function forms)


def dp4_exact(r):
    bidir, dis, frac, ap, af, dpp, dpf, pl, nn, ak, dk, pa, pd = [mp.mpf(float(x)) for x in r]
    if not dis:
        dpf *= frac; dpp *= frac; af *= frac; ap *= frac
    dpf += pd; dpp += pd; af += pa; ap += pa
    nobias = (af + ap) / (dpf + dpp)
    if ap / dpp >= af / dpf:
        if bidir:
            dpf, dpp = dpp, dpf; af, ap = ap, af
        else:
            return ap / dpp, nobias
    bf, bp = dpf * 2 - af, dpp * 2 - ap
    apf, bpf = ap / (ap + af), bp / (bp + bf)
    if (not bidir) and ak >= 0 and dk >= 0:
        apf = ak / (ak + dk * mp.mpf(0.9)); bpf = 1 - apf
    if (1 - apf) <= 0 or (1 - bpf) <= 0 or (bidir and (apf <= 0 or bpf <= 0)):
        return mp.nan, nobias
    gain = af * mp.log((1 - apf) / (1 - bpf))
    if bidir:
        gain += ap * mp.log(apf / bpf)
    if gain <= nn:
        return af / dpf, nobias
    return max(ap / dpp, (af / dpf) * mp.exp((nn - gain) / pl)), nobias


g = G.dp4_grid()
idx = G.dp4_exact_rows(g)
ex = [dp4_exact(g[i]) for i in idx]
store_double("dp4_0", idx, [e[0] for e in ex])
store_double("dp4_1", idx, [e[1] for e in ex])

# ---- het_lodq: (int)binom_llr and round(10 / ln 10 * powlaw_exponent * max(logit2(..), 0)) ----
g = G.het_lodq_grid()
valid = np.flatnonzero((g[:, 2] > 0) & (g[:, 2] < 1))
a1, a2, e, pl = (g[valid, k].astype(np.longdouble) for k in range(4))
pe, a_, b_ = (e + G.EPS) / (1 + 2 * G.EPS), a1 + G.EPS, a2 + G.EPS
vb = np.where(a_ > pe * (a_ + b_), np.longdouble(G.K10) * (a_ * np.log(a_ / (pe * (a_ + b_))) + b_ * np.log(b_ / ((1 - pe) * (a_ + b_)))), 0)
cand = np.union1d(np.flatnonzero((np.abs(vb - np.rint(vb)) < NEAR) & (vb != 0)), sample(len(valid), 1000))
ex = [binom_exact(g[valid[i], 2], g[valid[i], 0], g[valid[i], 1]) for i in cand]
db = [float(G.K10 * (float(a_[i]) * math.log(float(a_[i]) / (float(pe[i]) * float(a_[i] + b_[i]))) + float(b_[i]) * math.log(float(b_[i]) / ((1.0 - float(pe[i])) * float(a_[i] + b_[i]))))) if x != 0 else 0.0
      for i, x in zip(cand, ex)]
store_int("het_lodq_binom", valid[cand], ex, db, nearest_int, trunc_to_zero=True)

# ---- the adversarial histograms as generated ----
rows, names = G.adversarial_histograms()
out["adv_rows"] = rows.astype(np.int32); out["adv_class"] = np.array([sorted(G.ADVERSARIAL_MIN).index(n) for n in names], np.int8)   # index into sorted(ADVERSARIAL_MIN)

np.savez_compressed(G.EXACT_NPZ, **out)
print(G.EXACT_NPZ, os.path.getsize(G.EXACT_NPZ), "bytes")
