"""A numpy restatement of the callable-region intervals (uvcgpu_region_callable, uvcio_callable_*, uvc1-mi355x --callable-out), written from
the definitions alone; it loads no library.

Position p has six depths m_k(p), k in the order of MEASURES.  A request is min_depth[6] and max_aDP; 0 = not tested.  The mask of p:
bit k (LOW_<measure k>) when min_depth[k] > 0 and m_k(p) < min_depth[k]; bit 6 (EXCESS_aDP) when max_aDP > 0 and m_0(p) > max_aDP; bit 7
(NO_COVERAGE) when m_0(p) == 0.  p is callable iff its mask is 0.  A run is a maximal stretch of consecutive positions of one range with
equal masks; runs never cross a range border.  The report fills what no piece of a target reported with the mask of depth 0, joins
neighbouring runs of equal mask inside a target (never across targets) and writes one BED line per run."""
import numpy as np

MEASURES = ["aDP", "bDP", "cDP1", "cDP12", "cDP2", "dDP1"]
BITS = ["LOW_" + m for m in MEASURES] + ["EXCESS_aDP", "NO_COVERAGE"]
EXCESS, NOCOV = 6, 7
RUN = np.dtype([("range", np.int32), ("pos_beg", np.int32), ("pos_end", np.int32), ("mask", np.int32)])


def request(min_depth=None, max_aDP=0):
    """(min_depth as a list of six, max_aDP) from a dict name -> depth"""
    return [int((min_depth or {}).get(m, 0)) for m in MEASURES], int(max_aDP)


def masks_of(m, min_depth, max_aDP):
    """m: int [6][npos] -> the mask of every position, int32 [npos]"""
    m = np.asarray(m, dtype=np.int64)
    mask = np.zeros(m.shape[1], np.int32)
    for k, t in enumerate(min_depth):
        if t > 0:
            mask |= (m[k] < t).astype(np.int32) << k
    if max_aDP > 0:
        mask |= (m[0] > max_aDP).astype(np.int32) << EXCESS
    mask |= (m[0] == 0).astype(np.int32) << NOCOV
    return mask


def runs_of(m, beg, ranges, min_depth, max_aDP):
    """The runs of `ranges` ((pos_beg, pos_end) pairs, sorted, disjoint) over measures m [6][npos] whose column 0 is position `beg`."""
    mask = masks_of(m, min_depth, max_aDP)
    out = []
    for i, (a, b) in enumerate(ranges):
        v = mask[a - beg:b - beg]
        heads = np.concatenate([[0], np.flatnonzero(v[1:] != v[:-1]) + 1])
        ends = np.concatenate([heads[1:], [len(v)]])
        r = np.zeros(len(heads), RUN)
        r["range"], r["pos_beg"], r["pos_end"], r["mask"] = i, a + heads, a + ends, v[heads]
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, RUN)


def class_of(mask):
    return "CALLABLE" if mask == 0 else ",".join(n for k, n in enumerate(BITS) if mask >> k & 1)


def depth0_mask(min_depth):
    return (1 << NOCOV) | sum(1 << k for k, t in enumerate(min_depth) if t > 0)


def fill_join(beg, end, runs, min_depth):
    """runs: (pos_beg, pos_end, mask) of the pieces of the target [beg, end), in any order -> sorted, gaps filled with the mask of depth 0,
    neighbours of equal mask joined"""
    out, at, fill = [], beg, depth0_mask(min_depth)

    def put(a, b, k):
        if b <= a:
            return
        if out and out[-1][2] == k and out[-1][1] == a:
            out[-1][1] = b
        else:
            out.append([a, b, k])
    for a, b, k in sorted((int(a), int(b), int(k)) for a, b, k in runs):
        assert beg <= a and b <= end and a >= at, "the pieces of a target are disjoint and inside it"
        put(at, a, fill)
        put(a, b, k)
        at = b
    put(at, end, fill)
    return [tuple(r) for r in out]


def report_text(targets, runs_per_target, min_depth, max_aDP):
    """targets: (chrom, beg, end, name or None); runs_per_target: per target the (pos_beg, pos_end, mask) of its pieces"""
    text = "##callable_regions=1\n#min_depth\t" + ",".join("%s=%d" % (n, t) for n, t in zip(MEASURES, min_depth)) + "\n#max_aDP\t%d\n" % max_aDP
    text += "#chrom\tbeg\tend\tclass\ttarget\n"
    total, callable_, per_bit = 0, 0, [0] * len(BITS)
    for (chrom, beg, end, name), runs in zip(targets, runs_per_target):
        for a, b, k in fill_join(beg, end, runs, min_depth):
            text += "%s\t%d\t%d\t%s\t%s\n" % (chrom, a, b, class_of(k), name or ".")
            total += b - a
            callable_ += (b - a) if k == 0 else 0
            for j in range(len(BITS)):
                per_bit[j] += (b - a) if k >> j & 1 else 0
    text += "#summary\tpositions\t%d\n#summary\tCALLABLE\t%d\n" % (total, callable_)
    return text + "".join("#summary\t%s\t%d\n" % (n, v) for n, v in zip(BITS, per_bit))
