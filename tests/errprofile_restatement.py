"""The definitions of uvcgpu_region_error_profile (include/uvcgpu.h) restated in numpy over fetched plane groups: the checker
of tests/test_gpu_errprofile.py, and the layout helpers of the reader library's text."""
import numpy as np

from uvc_amd import _ffi

E = _ffi.ENUMS
NLEVEL, ROW = E["UVC_NERRLEVEL"], E["UVC_ERR_ROW"]
NCTX, NBASE, NLINK = E["UVC_ERR_NCTX"], E["UVC_ERR_NBASE"], E["UVC_ERR_NLINK"]
BASE_BINS, LINK_BINS, COUNTERS = E["UVC_ERR_BASE_BINS"], E["UVC_ERR_LINK_BINS"], E["UVC_ERR_COUNTERS"]
COUNTER_NAMES = ["BASE_counted", "BASE_low_depth", "BASE_high_alt", "LINK_counted", "LINK_low_depth", "LINK_high_alt", "no_context"]
C = {n: COUNTERS + E["UVC_ERRC_" + n] for n in COUNTER_NAMES}
BASE_SYMBOLS = ["A", "C", "G", "T"]
LINK_SYMBOLS = ["M", "D3P", "D2", "D1", "I3P", "I2", "I1"]
LEVEL_PLANES = [("FRAG", "UVC_FRAG_bDP"), ("FAM", "UVC_FAM_cDP1"), ("FAM", "UVC_FAM_cDP12"), ("FAM", "UVC_FAM_cDP2"), ("DUPLEX", "UVC_DUPLEX_dDP1")]   # the table of the issue


def level_cells(fetch):
    """c_L(s, p) of the five levels, int64 [NLEVEL][14][npos], from a `fetch(group)` of plane groups: both strands summed where there are two."""
    groups = {g: fetch(g) for g in ("FRAG", "FAM", "DUPLEX")}
    out = []
    for g, plane in LEVEL_PLANES:
        a = groups[g]
        out.append(a[:, E[plane]].sum(0, dtype=np.int64) if g != "DUPLEX" else a[E[plane]].astype(np.int64))
    return np.stack(out)


def contexts(refseq, npos):
    """(ctx, m) per position of a region of npos positions whose reference string holds npos - 1 characters: ctx = 16 l + 4 m + r, or -1 where
    one of the three symbols is not A/C/G/T; positions without a reference base (outside the string) are N."""
    assert len(refseq) == npos - 1
    code = np.full(256, 4, np.int64)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = k
    sym = np.concatenate([code[np.frombuffer(refseq.encode(), np.uint8)], [4]])
    l, r = np.concatenate([[4], sym[:-1]]), np.concatenate([sym[1:], [4]])
    ok = (l < 4) & (sym < 4) & (r < 4)
    return np.where(ok, 16 * l + 4 * sym + r, -1), sym


class Restatement:
    """Per-position classification of one (planes, reference, gate); profile(ranges) sums the positions of a range list."""

    def __init__(self, cells, refseq, beg, min_depth, max_alt_permille):
        self.cells, self.beg, self.npos = cells, beg, cells.shape[2]
        self.ctx, self.m = contexts(refseq, self.npos)
        self.kinds = []   # per level and kind: (level, first bin, n symbols, v [n][npos], class per position: 0 counted, 1 low depth, 2 high alt)
        at = np.arange(self.npos)
        for L in range(NLEVEL):
            for first, v, ref in ((BASE_BINS, cells[L, E["UVC_BASE_A"]:E["UVC_BASE_T"] + 1], np.minimum(self.m, 3)),
                                  (LINK_BINS, cells[L, E["UVC_LINK_M"]:E["UVC_LINK_I1"] + 1], np.zeros(self.npos, np.int64))):
                d = v.sum(0)
                alt = v.copy()
                alt[ref, at] = 0
                a = alt.max(0)
                cls = np.where(d < min_depth, 1, np.where(a * 1000 > max_alt_permille * d, 2, 0))
                self.kinds.append((L, first, v.shape[0], v, cls))

    def profile(self, ranges):
        sel = np.zeros(self.npos, bool)
        for a, b in ranges:
            assert not sel[a - self.beg:b - self.beg].any()
            sel[a - self.beg:b - self.beg] = True
        out = np.zeros((NLEVEL, ROW), np.int64)
        out[:, C["no_context"]] = int((sel & (self.ctx < 0)).sum())
        has = sel & (self.ctx >= 0)
        for k, (L, first, n, v, cls) in enumerate(self.kinds):
            c0 = COUNTERS + (E["UVC_ERRC_BASE_counted"] if first == BASE_BINS else E["UVC_ERRC_LINK_counted"])
            for which in range(3):
                out[L, c0 + which] = int((has & (cls == which)).sum())
            idx = np.nonzero(has & (cls == 0))[0]
            for s in range(n):
                np.add.at(out[L], first + self.ctx[idx] * n + s, v[s, idx])
        return out


def report_text(levels, profile, min_depth, max_alt_permille):
    """The text uvcio_errprofile_write writes for `profile` [n_levels][ROW]."""
    t = ["##error_profile_min_depth=%d" % min_depth, "##error_profile_max_alt_permille=%d" % max_alt_permille, "#level\tcounter\tcount"]
    for L, name in enumerate(levels):
        t += ["%s\t%s\t%d" % (name, c, profile[L][C[c]]) for c in COUNTER_NAMES]
    t.append("#level\tkind\tcontext\tsymbol\tcount\tref_count")
    for L, name in enumerate(levels):
        for kind, first, syms in (("BASE", BASE_BINS, BASE_SYMBOLS), ("LINK", LINK_BINS, LINK_SYMBOLS)):
            for ctx in range(NCTX):
                b = profile[L][first + ctx * len(syms):first + (ctx + 1) * len(syms)]
                if not np.any(b):
                    continue
                ref = (ctx >> 2) & 3 if kind == "BASE" else 0
                tri = "ACGT"[ctx >> 4] + "ACGT"[(ctx >> 2) & 3] + "ACGT"[ctx & 3]
                t += ["%s\t%s\t%s\t%s\t%d\t%d" % (name, kind, tri, s, b[j], b[ref]) for j, s in enumerate(syms)]
    return "\n".join(t) + "\n"
