"""A plain numpy restatement of the device read preparation (uvc_prep_reads, uvc_prep_compact and the order helpers of uvc_gap.hip), written
from the definitions and not from the kernels:

  * the comments of uvc_prep.h and uvc_device.h (FragRec, FsRec, FRAG_STAT_*, AlnRec: "simple = [one clip op] one M/=/X op [one clip op]")
  * fillTidBegEndFromAlns1 / 2 of the reference (main.hpp:658-697): exc_end = MAX(exc_end, bam_endpos(aln)) + 1 for every alignment in turn,
    inc_beg = MIN(inc_beg, pos); the handle clamps the end to the region end
  * bam_endpos: pos + the reference-consuming lengths (M = X D N), pos + 1 for a read without any
  * bam_get_strand (common.hpp:90): flag & 0x81 == 0x81 ? flag & 0x20 : flag & 0x10 -- the work-list class is is_reverse | strand << 1

Everything is a per-read map, a segment sum (np.add.reduceat) or a prefix sum (np.cumsum), so 4 M reads take seconds.  The recurrence
end = max(end, e_k) + 1 over the alignments k = 0 .. m-1 of a fragment or unit (from 0) has the closed form max_k(e_k - k) + m.

tests/test_prep_units_cpu.py checks it against itself (totals = sums of the per-read columns, and a slow per-read loop on the small
case); tests/test_gpu_prep_units.py compares the HIP path with it bit for bit."""
import numpy as np

M, I, D, N, S, H, PAD, EQ, X = range(9)
FRAG_STAT_EVENTS, FRAG_STAT_SWEEP, FRAG_STAT_ZERO_VALUE = 0, 1, 2
IONTORRENT = 2
INT32_MAX = 2 ** 31 - 1

SCALARS = ("n_frags n_fs n_complex n_simple n_generic n_dup n_sweep n_frag_strand0 max_frag_span max_unit_span max_unit_frags max_p2_span "
           "max_frag_depth any_amplicon p2_off[0] p2_off[1] p2_off[2] p2_off[3] p2_off[4] n_p2 table_rows item_slots gap_slots ins_total work dup_work").split()
PER_READ = {"endpos": np.int32, "kind": np.int32, "dflag_of": np.int32, "frag_of": np.int32, "fs_of": np.int32, "p2_first": np.int32,
            "table_off": np.int64, "item_off": np.int64, "gap_off": np.int64}
FRAG_FIELDS = "aln_beg aln_end beg end fs strand dflag normMQ n_cov n_near singleton stat_kind".split()      # n_cov / n_near: zero until k_fragstat
FS_FIELDS = {"frag_beg": np.int32, "frag_end": np.int32, "beg": np.int32, "end": np.int32, "strand": np.int32, "dflag": np.int32, "fam": np.int32,
             "generic": np.int32, "work_off": np.int64, "other_fs": np.int32}
# every output array of UvcPrepOut -> its element type (the order is the order the comparison reports in)
ARRAYS = dict(PER_READ)
ARRAYS.update({"complex_ids": np.int32, "frag_beg": np.int32, "frag_strand": np.int32})
ARRAYS.update({"frags." + f: np.int32 for f in FRAG_FIELDS})
ARRAYS.update({"fss." + f: t for f, t in FS_FIELDS.items()})
ARRAYS.update({"generic_fs": np.int32, "generic_sorted": np.int32, "sweep_frags": np.int32, "dup_units": np.int32, "dup_off": np.int64,
               "p2_aln": np.int32, "p2_beg": np.int32, "p2_end": np.int32, "p2_qb": np.int32, "p2_cls": np.int32})


def excl(v):
    """exclusive prefix sum, int64"""
    c = np.cumsum(v, dtype=np.int64)
    return c - v


def seg_sum(v, starts):
    return np.add.reduceat(np.asarray(v, np.int64), starts) if len(v) else np.zeros(len(starts), np.int64)


def zero_value_qual(P):
    """the quality at or below which a base adds nothing (uvc_rules.h): minus the addend of a mismatch; on IonTorrent minus the smaller addend"""
    a = min(P.bq_phred_added_misma, P.bq_phred_added_indel) if P.inferred_sequencing_platform == IONTORRENT else P.bq_phred_added_misma
    return -int(a)


def amplicon_gated(dflag, P):
    is_amplicon = ((dflag & 4) != 0) | bool(P.primerlen > 0 and not (2 & P.primer_flag))
    return is_amplicon & (not (P.tn_is_paired and (1 & P.primer_flag)))


def spans(pos, endpos, starts, counts, rend):
    """(beg, end) of each segment of consecutive alignments by fillTidBegEndFromAlns1 / 2, end clamped to the region end"""
    rel = np.arange(len(pos), dtype=np.int64) - np.repeat(starts, counts)
    beg = np.minimum.reduceat(pos, starts)
    end = np.maximum.reduceat(endpos.astype(np.int64) - rel, starts) + counts
    return beg.astype(np.int32), np.minimum(end, rend).astype(np.int32)


def prep_units(reads, P, rbeg, rend, npos, zero_qual=None):
    """reads: the UvcReadSoA columns as numpy arrays (tests' convention); P: a UvcParams; [rbeg, rend): the region, npos = rend - rbeg;
    zero_qual: UvcPrepIn::zero_qual (None: not known).  -> {name: array or int} of every name of ARRAYS and SCALARS."""
    n = int(reads["n_reads"])
    pos = reads["pos"].astype(np.int64); nc = reads["n_cigar"].astype(np.int64); lq = reads["l_qseq"].astype(np.int64)
    seq_off = reads["seq_off"].astype(np.int64); flag = reads["flag"].astype(np.int64)
    # ---- one row per CIGAR op
    first_op = excl(nc)
    rd = np.repeat(np.arange(n), nc)
    at = np.repeat(reads["cigar_off"].astype(np.int64), nc) + (np.arange(int(nc.sum())) - np.repeat(first_op, nc))
    op = (reads["cigars"][at] & 0xF).astype(np.int64); ln = (reads["cigars"][at] >> 4).astype(np.int64)
    is_m = (op == M) | (op == EQ) | (op == X)
    on_ref = is_m | (op == D) | (op == N)
    on_query = is_m | (op == I) | (op == S)
    ref_len = seg_sum(ln * on_ref, first_op)
    endpos = pos + np.where(ref_len > 0, ref_len, 1)
    n_m = seg_sum(is_m, first_op)
    n_other = seg_sum(~is_m & (op != S) & (op != H), first_op)            # ops that are neither an M-like run nor a clip
    first_is_m = is_m[first_op]; last_is_m = is_m[first_op + nc - 1]
    simple = (n_m == 1) & (n_other == 0) & (nc <= 3) & ~((nc == 3) & (first_is_m | last_is_m))
    n_gap = seg_sum((op == I) | (op == D), first_op); ins_len = seg_sum(ln * (op == I), first_op); del_len = seg_sum(ln * (op == D), first_op)
    has_np = seg_sum((op == N) | (op == PAD), first_op) > 0
    ref_at = excl(ln * on_ref) - np.repeat(excl(ln * on_ref)[first_op], nc)          # reference offset of the op from the alignment's begin
    q_at = excl(ln * on_query) - np.repeat(excl(ln * on_query)[first_op], nc)        # query offset of the op
    far = is_m & ((ref_at > 65535) | (np.repeat(endpos - pos, nc) - (ref_at + ln) > 65535))
    runs_near = seg_sum(far, first_op) == 0
    seg_eligible = (P.inferred_sequencing_platform != IONTORRENT) and rbeg >= 65536 and P.bias_thres_interfering_indel <= 10000
    kind = np.where(simple, 0, np.where(runs_near & ~has_np & bool(seg_eligible), 2, 1))
    n_p2 = np.where(kind != 1, n_m, 0)
    cplx = kind != 0
    out = {}
    out["endpos"] = endpos; out["kind"] = kind; out["n_p2_of"] = n_p2; out["p2_first"] = excl(n_p2)
    trows = np.where(cplx, endpos - pos + 1, 0); items = np.where(cplx, 2 * lq + 2 * del_len + nc + 4, 0)
    gaps = np.where(cplx, n_gap, 0); ins = np.where(cplx, ins_len, 0)
    out["trows"], out["items"], out["gaps"], out["ins"] = trows, items, gaps, ins
    for name, col in (("table_off", trows), ("item_off", items), ("gap_off", gaps)):
        out[name] = np.where(cplx, excl(col), -1)
    out["complex_ids"] = np.flatnonzero(cplx)
    fam = reads["fam_id"].astype(np.int64); strand = reads["fam_strand"].astype(np.int64); frag_id = reads["frag_id"].astype(np.int64)
    dflag_of = reads["fam_dflag"].astype(np.int64)[fam]
    out["dflag_of"] = dflag_of
    # ---- the nesting: a new unit where (fam_id, fam_strand) changes, a new fragment there or where frag_id changes
    new_fs = np.ones(n, bool); new_fs[1:] = (fam[1:] != fam[:-1]) | (strand[1:] != strand[:-1])
    new_frag = new_fs.copy(); new_frag[1:] |= frag_id[1:] != frag_id[:-1]
    out["new_frag"], out["new_fs"] = new_frag, new_fs
    out["frag_of"] = np.cumsum(new_frag) - 1; out["fs_of"] = np.cumsum(new_fs) - 1
    f0 = np.flatnonzero(new_frag); nf = len(f0); f1 = np.append(f0[1:], n); fcnt = f1 - f0
    u0 = np.flatnonzero(new_fs); nu = len(u0); u1 = np.append(u0[1:], n); ucnt = u1 - u0
    # ---- fragments
    fbeg, fend = spans(pos, endpos, f0, fcnt, rend)
    all_simple = seg_sum(cplx, f0) == 0
    f_dflag = dflag_of[f0]
    stat = np.where(all_simple & (fcnt <= 2) & ~amplicon_gated(f_dflag, P), FRAG_STAT_EVENTS, FRAG_STAT_SWEEP)
    zthr = zero_value_qual(P)
    if zthr > 0 or (zthr == 0 and (zero_qual is None or zero_qual != 0)):
        low = np.concatenate([[0], np.cumsum(reads["quals"].astype(np.int64) <= zthr)])
        stat = np.where(seg_sum(low[seq_off + lq] - low[seq_off], f0) > 0, FRAG_STAT_ZERO_VALUE, stat)
    # ---- units
    ubeg, uend = spans(pos, endpos, u0, ucnt, rend)
    u_fam, u_strand, u_dflag = fam[u0], strand[u0], dflag_of[u0]
    u_frag_beg = out["frag_of"][u0]; u_frag_end = np.append(u_frag_beg[1:], nf)
    unit_of = np.full((int(reads["n_fams"]), 2), -1, np.int64)
    assert len(np.unique(u_fam * 2 + u_strand)) == nu, "reads of one (fam_id, fam_strand) are not contiguous"
    unit_of[u_fam, u_strand] = np.arange(nu)
    other = unit_of[u_fam, 1 - u_strand]
    singleton_ok = min(P.fam_thres_dup1add, P.fam_thres_dup2add, P.fam_thres_emperr_all_flat_snv, P.fam_thres_emperr_all_flat_indel) >= 2
    duplex = ((u_dflag & 2) != 0) & (other >= 0)
    generic = ((u_frag_end - u_frag_beg) >= 2) | duplex | (not singleton_ok)
    uspan = (uend.astype(np.int64) - ubeg) * generic
    generic_fs = np.flatnonzero(generic)
    is_dup = duplex & (u_strand == 0)
    o_safe = np.where(other >= 0, other, 0)
    dspan = np.where(is_dup, np.maximum(uend, np.minimum(uend[o_safe], rend)).astype(np.int64) - np.minimum(ubeg, ubeg[o_safe]), 0)
    out.update({"frag_beg": fbeg, "frag_strand": strand[f0], "frags.aln_beg": f0, "frags.aln_end": f1, "frags.beg": fbeg, "frags.end": fend, "frags.fs": out["fs_of"][f0],
                "frags.strand": strand[f0], "frags.dflag": f_dflag, "frags.normMQ": np.maximum.reduceat(reads["mapq"].astype(np.int64), f0), "frags.n_cov": np.zeros(nf, np.int64),
                "frags.n_near": np.zeros(nf, np.int64), "frags.singleton": 1 - generic[out["fs_of"][f0]].astype(np.int64), "frags.stat_kind": stat,
                "sweep_frags": np.flatnonzero(stat != FRAG_STAT_EVENTS)})
    out.update({"fss.frag_beg": u_frag_beg, "fss.frag_end": u_frag_end, "fss.beg": ubeg, "fss.end": uend, "fss.strand": u_strand, "fss.dflag": u_dflag, "fss.fam": u_fam,
                "fss.generic": generic.astype(np.int64), "fss.work_off": np.where(generic, excl(uspan), 0), "fss.other_fs": other,
                "generic_fs": generic_fs, "generic_sorted": generic_fs[np.argsort(ubeg[generic_fs], kind="stable")],
                "dup_units": np.flatnonzero(is_dup), "dup_off": excl(dspan)[is_dup]})
    # ---- the work-list entries: every M-like run of the reads with n_p2 > 0, in read order
    listed = is_m & np.repeat(n_p2 > 0, nc)
    e_rd = rd[listed]
    cls_of = ((flag & 0x10) != 0) * 1 + np.where((flag & 0x81) == 0x81, (flag & 0x20) != 0, (flag & 0x10) != 0) * 2
    e_beg = pos[e_rd] + ref_at[listed]
    qb = (seq_off[e_rd] + q_at[listed] - e_beg) & 0xFFFFFFFF
    out.update({"p2_aln": e_rd, "p2_beg": e_beg, "p2_end": e_beg + ln[listed], "p2_qb": qb.astype(np.uint32).view(np.int32), "p2_cls": cls_of[e_rd]})
    # ---- totals and bounds
    cls_n = np.bincount(cls_of[e_rd], minlength=4)
    depth = nf
    if nf >= 65536:   # the exact largest number of fragment spans [beg, end) over one position
        d = np.zeros(npos + 2, np.int64)
        np.add.at(d, fbeg.astype(np.int64) - rbeg, 1); np.add.at(d, fend.astype(np.int64) - rbeg, -1)
        depth = int(np.cumsum(d).max())
    gen_frags = (u_frag_end - u_frag_beg)[generic]
    sc = {"n_frags": nf, "n_fs": nu, "n_complex": int(cplx.sum()), "n_simple": n - int(cplx.sum()), "n_generic": len(generic_fs), "n_dup": int(is_dup.sum()),
          "n_sweep": int((stat != FRAG_STAT_EVENTS).sum()), "n_frag_strand0": int((strand[f0] == 0).sum()),
          "max_frag_span": max(1, int((fend.astype(np.int64) - fbeg).max())), "max_unit_span": max(1, int(uspan.max())),
          "max_unit_frags": int(gen_frags.max()) if len(gen_frags) else 0, "max_p2_span": max(1, int(ln[listed].max()) if listed.any() else 1),
          "max_frag_depth": depth, "any_amplicon": int(((dflag_of & 4) != 0).any()),
          "n_p2": int(n_p2.sum()), "table_rows": int(trows.sum()), "item_slots": int(items.sum()), "gap_slots": int(gaps.sum()), "ins_total": int(ins.sum()),
          "work": int(uspan.sum()), "dup_work": int(dspan.sum())}
    for c in range(5):
        sc["p2_off[%d]" % c] = int(cls_n[:c].sum())
    out.update(sc)
    return out


def compact_offsets(l_qseq, n_cigar):
    """the three offset columns of the compact input form: seq_off, cigar_off and the byte offset of each read in the 4-bit base column"""
    lq = l_qseq.astype(np.int64)
    return {"seq_off": excl(lq), "cigar_off": excl(n_cigar.astype(np.int64)), "b4_off": excl((lq + 1) // 2)}


def sort_key(pos, cls, beg, pos_bits):
    """the key of uvc_sort_by_pos_cls: (pos - beg) | cls << pos_bits, as an unsigned 32-bit number"""
    return ((pos.astype(np.int64) - beg) & 0xFFFFFFFF) | (cls.astype(np.int64) << pos_bits)


def sorted_ids(pos, cls, beg, pos_bits):
    return np.argsort(sort_key(pos, cls, beg, pos_bits), kind="stable")


def rank_from_sorted(perm, n_first, sentinel):
    """-> (out_ids, rank): out_ids[k] = the k-th id for k < n_first, the rest keeps the sentinel; rank[id] = k for those, -1 for the others"""
    n = len(perm)
    ids = np.full(n, sentinel, np.int64); ids[:n_first] = perm[:n_first]
    rank = np.full(n, -1, np.int64); rank[perm[:n_first]] = np.arange(n_first)
    return ids, rank


def gather4(perm, cols, kind, sentinel):
    """-> ([four columns in sorted order], slot): the slot of a kind-0 alignment is the index of its single entry (cols[0] names the
    entry's alignment); every other alignment gets -1"""
    o = [c[perm] for c in cols]
    slot = np.where(kind == 0, sentinel, -1).astype(np.int64)
    k0 = kind[o[0]] == 0
    slot[o[0][k0]] = np.flatnonzero(k0)
    return o, slot
