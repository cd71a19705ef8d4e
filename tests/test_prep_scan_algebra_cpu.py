"""The arithmetic of k_prep_scan (uvc_amd/csrc/uvc_kernels_acc.hip) without a GPU: the five P1 counters behind the base quality, once
straight from their definition (what k_prep_fast adds per covering read and position) and once as the kernel forms them -- interval sums
over the covering reads minus a point correction per low-quality base, per tile, in wrapping 32-bit words for the distance sums and with the
LOW words of the 64-bit BAQ prefix sums taken relative to the tile's first position.  Both must be equal, also where the prefix sums cross
2^31 or 2^32 inside a read."""
import numpy as np
import pytest

THR = 20


def make_reads(rng, n_pos, n_reads):
    apos = np.sort(rng.integers(0, n_pos - 2, n_reads))
    length = np.where(rng.random(n_reads) < 0.2, rng.integers(1, 18, n_reads), rng.integers(40, 160, n_reads))
    rend = np.minimum(apos + length, n_pos - 1)
    quals = [np.where(rng.random(e - a) < 0.25, rng.integers(0, THR, e - a), rng.integers(THR, 42, e - a)) for a, e in zip(apos, rend)]
    for k in range(0, n_reads, 11):   # low throughout, low at both ends
        quals[k][:] = 3
    for k in range(5, n_reads, 7):
        quals[k][0] = 0
        quals[k][-1] = 19
    return apos, rend, quals


def i32(v):
    """The low word of v as a signed 32-bit number."""
    return ((np.asarray(v, np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int64)


def by_definition(n_pos, apos, rend, quals, baq_lo):
    hbq = np.zeros(n_pos, np.int64)
    ld, rd = np.zeros(n_pos, np.uint32), np.zeros(n_pos, np.uint32)
    lb, rb = np.zeros(n_pos, np.int64), np.zeros(n_pos, np.int64)
    for a, e, q in zip(apos, rend, quals):
        p = np.arange(a, e)[q >= THR]
        hbq[p] += 1
        ld[p] += (p - a + 1).astype(np.uint32)
        rd[p] += (e - p).astype(np.uint32)
        lb[p] += i32(baq_lo[p] - baq_lo[a] + 1)        # (int)(my_baq - baq_pos + 1) on 32-bit words
        rb[p] += i32(baq_lo[e - 1] - baq_lo[p] + 1)
    return hbq, ld, rd, lb, rb


def by_tiles(n_pos, apos, rend, quals, baq_lo, tile, origin):
    """origin: the reference position of index 0 (the kernel adds up reference positions, which wrap 32 bits at any depth above two)."""
    out = [np.zeros(n_pos, np.int64), np.zeros(n_pos, np.uint32), np.zeros(n_pos, np.uint32), np.zeros(n_pos, np.int64), np.zeros(n_pos, np.int64)]
    for t0 in range(0, n_pos, tile):
        t1 = min(t0 + tile, n_pos)
        d32 = np.zeros((3, tile + 1), np.uint32)     # A, sum of apos, sum of rend
        d64 = np.zeros((2, tile + 1), np.uint64)     # sum of cL, sum of cR
        c32 = np.zeros((3, tile), np.uint32)
        c64 = np.zeros((2, tile), np.uint64)
        b0 = baq_lo[t0]
        for a, e, q in zip(apos, rend, quals):
            if e <= t0 or a >= t1:
                continue
            s, en = max(a, t0), min(e, t1)
            cl, cr = i32(b0 - baq_lo[a] + 1), i32(baq_lo[e - 1] - b0 + 1)
            v32 = np.array([1, origin + a, origin + e]).astype(np.uint32)
            v64 = np.array([cl, cr]).astype(np.int64).astype(np.uint64)
            d32[:, s - t0] += v32
            d32[:, en - t0] -= v32
            d64[:, s - t0] += v64
            d64[:, en - t0] -= v64
            low = np.arange(a, e)[q < THR]
            low = low[(low >= s) & (low < en)] - t0
            c32[:, low] += v32[:, None]
            c64[:, low] += v64[:, None]
        s32 = np.cumsum(d32[:, :tile], axis=1, dtype=np.uint32) - c32
        s64 = (np.cumsum(d64[:, :tile], axis=1, dtype=np.uint64) - c64).astype(np.int64)
        n = t1 - t0
        p = (origin + np.arange(t0, t1)).astype(np.uint32)
        hb = s32[0, :n]
        d = i32(baq_lo[t0:t1] - b0)
        out[0][t0:t1] = hb
        out[1][t0:t1] = (p + np.uint32(1)) * hb - s32[1, :n]
        out[2][t0:t1] = s32[2, :n] - p * hb
        out[3][t0:t1] = hb.astype(np.int64) * d + s64[0, :n]
        out[4][t0:t1] = s64[1, :n] - hb.astype(np.int64) * d
    return out


@pytest.mark.parametrize("tile", [256, 512, 1024])
@pytest.mark.parametrize("baq_start", [0, (1 << 31) - 20000, (1 << 32) - 20000, (1 << 33) + (1 << 31) - 9000])
def test_interval_sums_minus_point_corrections_equal_the_definition(baq_start, tile):
    rng = np.random.default_rng(17)
    n_pos, n_reads = 2600, 400
    apos, rend, quals = make_reads(rng, n_pos, n_reads)
    baq64 = baq_start + np.cumsum(rng.integers(0, 31, n_pos)).astype(np.int64)
    if baq_start:   # the prefix sums cross a 32-bit boundary inside the region, and inside reads
        edge = (baq_start | ((1 << 31) - 1)) + 1
        x = int(np.searchsorted(baq64, edge))
        assert 0 < x < n_pos and ((apos < x) & (rend > x)).any()
    baq_lo = i32(baq64)
    want = by_definition(n_pos, apos, rend, quals, baq_lo)
    got = by_tiles(n_pos, apos, rend, quals, baq_lo, tile, origin=1_500_000_000)
    for name, w, g in zip(("highBQ_dp", "l_dist_sum", "r_dist_sum", "l_BAQ_sum", "r_BAQ_sum"), want, got):
        assert np.array_equal(w.astype(np.int64), g.astype(np.int64)), name
    assert want[0].max() > 5 and (want[0] == 0).any()
