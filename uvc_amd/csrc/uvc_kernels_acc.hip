// uvc_kernels_acc.hip -- hand-written gfx950 kernels for the accumulate half of the UVC hot path.
//
// Decomposition.  The reference walks every read 5 times and scatters `+=`
// into ~5.5 KB of per-position state (main.hpp:2543-3594).  Here the loops are turned inside out:
// a wavefront owns 64 consecutive reference positions (one lane = one position), loops over the
// alignments / fragments that overlap its window (wave-uniform control flow; the per-read scalars of
// 64 records are loaded one per lane and broadcast with v_readlane; base/qual bytes come through a
// bounds-checked buffer descriptor, coalesced across lanes) and keeps the accumulators of the two
// symbols that matter at a position -- the reference base and LINK_M -- in registers.  Everything
// rare takes a sparse path: mismatching bases through per-wave LDS queues and a lane-per-item
// kernel, InDel symbols through wave-per-read kernels, rare symbols of the fragment pass through
// fire-and-forget atomics.  All updates are integer adds or maxima, so any order gives
// bit-identical results.  The kernels are issue-bound:
// the code below is written to minimise VALU + SALU instructions per (read, 64 positions).
//
//   k_pack_bq        per read base  base | qual << 8
//   k_aln_prelude    per read       nge/ngo/clips, xm1500, bm1500s, penalties, eligibility; the work-list record of a simple read   main.hpp:1795-1885
//   k_build_p2list   per entry      the work-list records of the M runs of InDel reads (one list for P1 and P2, 4 orientation classes)
//   k_correct_bq     per read       apply_bq_err_correction3 (on request)                     grouping.cpp:459-543
//   k_prep_fast      per position   P1 for simple reads (the work list without the M runs)    main.hpp:924-1204
//   k_prep_scan      read / tile    the same by a byte-parallel scan of each read + interval sums (the default where the split form does not run)
//   k_prep_slow      wave per read  P1 for reads with InDels (atomics)
//   k_thres          per position   P1b, also edits rtr.indelphred                            main.hpp:1206-1299
//   k_p2_fast<L,B>   per position   P2 + dealwith_segbias, LINK_M / read base instantiations   main.hpp:1360-1595, 1762-2296
//   k_p2_mism        per queued base  the same for bases that differ from the reference
//   k_p2_slow<BIAS>  wave per read  CIGAR walk of InDel reads: P2 items (BIAS) or the BASE_QUALITY_MAX contribution table
//   k_p2_items       wave per read  applies the items
//   k_fragstat_*     per fragment   covered / near-mutation position counts, M runs of InDel fragments   main.hpp:2738-2756
//   k_frag_generic   wave per fragment chunk  P3 at the positions next to InDels / of fragments with > 2 alignments
//   k_frag           per position   P3 + P3b, and P4/P5 of singleton families                 main.hpp:2620-2830, 2832-3594
//   k_fam_stat       per generic family-strand unit  medians of read ends, no-strict-bias window main.hpp:2916-2998
//   k_fam_p4/p5      per (unit, position)  P4 / P5 of multi-fragment families, generic form    main.hpp:2883-3522
//   k_fam_p4d(_rest)/p5d  per 64-position window  the same on deep data, through a per-cell digest
//   k_duplex(_d)     per (duplex family, position)  generic form / from the digest             main.hpp:3523-3550
//   k_p5b            per (position, strand)  bucket -> quality for family consensus           main.hpp:3552-3591
//   k_gap_keys/alleles/rows  per (family, InDel position)  the allele-keyed counters of the InDel symbols   main.hpp:2710-2717, 3196-3546
// uvc_launch_accumulate at the end of the file orders them on three streams (the dependency table in front of it).
// The reference rules that several of them share (pair consensus, assay predicates, ...) stand once in uvc_rules.h; record words and flag bits go by the names of uvc_device.h.
#include "uvc_launch.h"
#include "uvc_collectives.h"
#include "uvc_report_dev.h"   // the family-concordance kernels at the end tally like the report kernels
#include <algorithm>
#include <stdlib.h>
#include <string.h>

// ------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------
DEV int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Workgroups are dealt to the 8 XCDs round-robin (block b -> XCD b % 8) and each XCD has its own L2.  Position-window kernels
// therefore give XCD k one contiguous eighth of the region, so that neighbouring windows, which read the same alignments,
// share an L2.  Placement only affects speed, never results.
DEV int xcd_block() {
    const int nb = gridDim.x, b = blockIdx.x, q = nb >> 3, r = nb & 7, k = b & 7, i = b >> 3;
    return k * q + (k < r ? k : r) + i;
}

DEV int bcast(int v, int j) { return __builtin_amdgcn_readlane(v, j); }   // j must be wave-uniform
#ifdef UVC_FRAG_COARSE   // debug build (make XFLAGS=-DUVC_FRAG_COARSE): s_memtime at the three stages of k_frag, printed for a few waves
#define COARSE_T(v) unsigned long long v; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) :: "memory");
#else
#define COARSE_T(v)
#endif
// base | qual << 8 of read byte `idx` through a raw buffer descriptor: out-of-range indices (lanes outside the read) return 0
DEV __amdgpu_buffer_rsrc_t bq_rsrc(const RegionDev &R) { return __builtin_amdgcn_make_buffer_rsrc((void *)R.bq, 0, (int)R.bq_bytes, 0x00020000); }
DEV int bq_load(__amdgpu_buffer_rsrc_t rs, int idx) { return (int)__builtin_amdgcn_raw_buffer_load_b16(rs, idx << 1, 0, 0); }
// Window index: for every 64-position window w and every begin-sorted work list, the records a wave of window w walks:
// [first record with begin >= window begin - longest span + 1, first record with begin >= window end).  A binary search per wave and list is
// ~20 dependent memory round trips (8 lists' bounds in k_p2_fast: an eighth of a wave's life); the table costs one load each.
// Lists: 1..4 = the four sub-lists of frec2 (k_p2_fast; k_prep_sums and k_prep_fast walk the same four and skip what is not a whole simple
// alignment), 5..6 = the two strands of ffast (k_frag), 7 = the generic family-strand units by begin (the window kernels of the family
// passes: two loads per search step there).  Slot 0 of the table is not used.
#define WIN_LISTS 8
DEV int win_lo(const RegionDev &R, int list, int w) { return R.win[((size_t)list * 2) * R.nwin + w]; }
DEV int win_hi(const RegionDev &R, int list, int w) { return R.win[((size_t)list * 2 + 1) * R.nwin + w]; }
__global__ void __launch_bounds__(256) k_win_index(RegionDev R, int list_beg, int list_end) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_list = 2 * (int64_t)R.nwin;
    if (t >= per_list * (list_end - list_beg)) return;
    const int list = list_beg + (int)(t / per_list), which = (int)((t % per_list) / R.nwin), w = (int)(t % R.nwin);
    const char *base; int stride, lo, hi, span;
    if (list <= 4) { base = (const char *)&R.frec2[0].pos; stride = sizeof(FastRec); lo = R.p2_off[list - 1]; hi = R.p2_off[list]; span = R.max_p2_span; }
    else if (list <= 6) { base = (const char *)&R.ffast[0].beg; stride = sizeof(FragFast); lo = R.frag_off[list - 5]; hi = R.frag_off[list - 4]; span = R.max_frag_span; }
    else { base = nullptr; stride = 0; lo = 0; hi = R.n_generic_fs; span = R.max_unit_span; }
    const int w0 = R.beg + 64 * w, key = (which == 0 ? w0 - span + 1 : w0 + 64);
    if (list <= 6) { while (lo < hi) { const int mid = (lo + hi) >> 1; if (*(const int32_t *)(base + (size_t)mid * stride) < key) lo = mid + 1; else hi = mid; } }
    else { while (lo < hi) { const int mid = (lo + hi) >> 1; if (R.fss[R.generic_sorted[mid]].beg < key) lo = mid + 1; else hi = mid; } }
    R.win[((size_t)list * 2 + which) * R.nwin + w] = lo;
}

struct SegAcc {   // SegFormatInfoSet (main_conversion.hpp:645-691) + the VQ a1/a2 sums + bqsum of ONE symbol at ONE position
    int s[UVC_NSEG32];
    long long l[UVC_NSEG64];
    int lp[UVC_NSEG64];   // k_p2_fast: 32-bit partial sums of the 64-bit counters over one chunk of 64 reads (each term < 2^25), folded into l[] per chunk
    int a1BQf, a1BQr, a2BQf, a2BQr, bq;
    DEV void zero() { for (int i = 0; i < UVC_NSEG32; i++) s[i] = 0; for (int i = 0; i < UVC_NSEG64; i++) { l[i] = 0; lp[i] = 0; } a1BQf = a1BQr = a2BQf = a2BQr = bq = 0; }
    DEV void fold() { for (int i = 0; i < UVC_NSEG64; i++) { l[i] += (long long)lp[i]; lp[i] = 0; } }
};

DEV void seg_flush(const RegionDev &R, const SegAcc &A, int sym, int64_t x) {
    mark_sym(R, sym, x);   // (with RegionDev::occ: scoring looks at the marked symbols of a position only)
#pragma unroll
    for (int f = 0; f < UVC_NSEG32; f++) if (A.s[f]) atomicAdd(&S32(R, f, sym, x), A.s[f]);
#pragma unroll
    for (int f = 0; f < UVC_NSEG64; f++) if (A.l[f]) add64(&S64(R, f, sym, x), A.l[f]);
    if (A.a1BQf) atomicAdd(&VQP(R, UVC_VQ_a1BQf, sym, x), A.a1BQf);
    if (A.a1BQr) atomicAdd(&VQP(R, UVC_VQ_a1BQr, sym, x), A.a1BQr);
    if (A.a2BQf) atomicAdd(&VQP(R, UVC_VQ_a2BQf, sym, x), A.a2BQf);
    if (A.a2BQr) atomicAdd(&VQP(R, UVC_VQ_a2BQr, sym, x), A.a2BQr);
    if (A.bq) atomicAdd(&BQS(R, sym, x), A.bq);
}

// first writer of (sym, x) after the planes were zeroed: plain stores, no read-modify-write
DEV void seg_store(const RegionDev &R, const SegAcc &A, int sym, int64_t x) {
#pragma unroll
    for (int f = 0; f < UVC_NSEG32; f++) if (A.s[f]) S32(R, f, sym, x) = A.s[f];
#pragma unroll
    for (int f = 0; f < UVC_NSEG64; f++) if (A.l[f]) S64(R, f, sym, x) = A.l[f];
    if (A.a1BQf) VQP(R, UVC_VQ_a1BQf, sym, x) = A.a1BQf;
    if (A.a1BQr) VQP(R, UVC_VQ_a1BQr, sym, x) = A.a1BQr;
    if (A.a2BQf) VQP(R, UVC_VQ_a2BQf, sym, x) = A.a2BQf;
    if (A.a2BQr) VQP(R, UVC_VQ_a2BQr, sym, x) = A.a2BQr;
    if (A.bq) BQS(R, sym, x) = A.bq;
}

// The completion pass of LINK_M (k_p2_fast<true, false>): everything of A but the five cells the base pass has stored (aDP**, BQSUM), added
// to what k_p2_items put there since.  The lane owns its cells while the pass runs and no other writer does: load, add, store.
DEV constexpr bool seg_is_adp(int f) { return f == UVC_S_aDPff || f == UVC_S_aDPfr || f == UVC_S_aDPrf || f == UVC_S_aDPrr; }
template <bool WITH5>   // WITH5 (the generic forms): the five cells too, nobody has stored them
DEV void seg_add_link(const RegionDev &R, const SegAcc &A, int64_t x) {
    if (WITH5 && A.bq) BQS(R, UVC_LINK_M, x) += A.bq;
#pragma unroll
    for (int f = 0; f < UVC_NSEG32; f++) if (A.s[f] && (WITH5 || !seg_is_adp(f))) S32(R, f, UVC_LINK_M, x) += A.s[f];
#pragma unroll
    for (int f = 0; f < UVC_NSEG64; f++) if (A.l[f]) S64(R, f, UVC_LINK_M, x) += A.l[f];
    if (A.a1BQf) VQP(R, UVC_VQ_a1BQf, UVC_LINK_M, x) += A.a1BQf;
    if (A.a1BQr) VQP(R, UVC_VQ_a1BQr, UVC_LINK_M, x) += A.a1BQr;
    if (A.a2BQf) VQP(R, UVC_VQ_a2BQf, UVC_LINK_M, x) += A.a2BQf;
    if (A.a2BQr) VQP(R, UVC_VQ_a2BQr, UVC_LINK_M, x) += A.a2BQr;
}

struct PosThres { int t[UVC_NTHRES]; };

// per-read quantities that dealwith_segbias needs; all wave-uniform in the fast kernels
struct SegRead {
    int pos, rend, flag, mapq, isize, frag_pos_L, frag_pos_R, xm1500, clip_cnt, dflag;
    long long baq_pos, baq_last, baq2_last;
};

DEV SegRead make_segread(const RegionDev &R, const AlnRec &a) {
    SegRead r;
    r.pos = a.pos; r.rend = a.rend; r.flag = a.flag; r.mapq = a.mapq; r.isize = a.isize;
    r.frag_pos_L = imin(a.pos, a.mpos); r.frag_pos_R = r.frag_pos_L + abs(a.isize);
    r.xm1500 = a.xm1500; r.clip_cnt = a.clip_cnt; r.dflag = a.dflag;
    r.baq_pos = a.baq_pos; r.baq_last = a.baq_last; r.baq2_last = a.baq2_last;
    return r;
}

// update_bidirectional_bias, main.hpp:1318-1358
DEV void bidir(int &LP1, int &LP2, int &RP1, int &RP2, long long &LPL, long long &RPL, int L1, int L2, int R1, int R2, long long nl, long long nr, bool tier2, int n_indel) {
    if (nl + n_indel >= L1) LP1 += 1;
    if ((nl + n_indel >= L2) && tier2) LP2 += 1;
    if (nr >= R1) RP1 += 1;
    if ((nr >= R2) && tier2) RP2 += 1;
    LPL += nl; RPL += nr;
}

// dealwith_segbias<isGap>, main.hpp:1360-1595 (COMPILATION_ENABLE_XMGOT == 0)
template <bool isGap>
DEV void segbias(SegAcc &A, const UvcParams &P, const SegRead &r, const PosThres &T, int rpos, long long baq_p, long long baq2_p,
                 int bq, int bm1500, int cigar_op, int indel_len, int dist_to_interfering_indel) {
    const bool amplicon = is_assay_amplicon(r.dflag, P);
    const bool normal_filter_primers = normal_filters_primers(P);
    const bool is_assay_UMI = (r.dflag & UVC_DFLAG_UMI);
    const int seg_l_baq1 = (int)(baq_p - r.baq_pos + 1);
    const int _seg_r_baq = (int)(r.baq_last - baq_p + 1);
    const int seg_r_baq1 = (isGap ? (int)lmin((long long)_seg_r_baq, r.baq2_last - baq2_p + 7) : _seg_r_baq);
    const int seg_l_nbases = rpos - r.pos + 1;
    const int seg_r_nbases = r.rend - rpos;
    const bool is_high_readlen = (P.central_readlen >= P.microadjust_median_readlen_thres);
    const int seg_l_baq = (is_high_readlen ? seg_l_baq1 : imax(seg_l_baq1, seg_l_nbases * P.microadjust_BAQ_per_base_x1024 / 1024));
    const int seg_r_baq = (is_high_readlen ? seg_r_baq1 : imax(seg_r_baq1, seg_r_nbases * P.microadjust_BAQ_per_base_x1024 / 1024));
    const int frag_l_nbases2 = ((r.isize != 0) ? imin(rpos - r.frag_pos_L + 1, MAX_INSERT_SIZE) : MAX_INSERT_SIZE);
    const int frag_r_nbases2 = ((r.isize != 0) ? imin(r.frag_pos_R - rpos, MAX_INSERT_SIZE) : MAX_INSERT_SIZE);
    const bool is_normal = ((r.isize != 0) || (0 == (r.flag & 0x1)));
    const bool isrc = (r.flag & 0x10) != 0;
    const bool strand = ((r.flag & 0x81) == 0x81) ? ((r.flag & 0x20) != 0) : ((r.flag & 0x10) != 0);   // bam_get_strand, common.hpp:89

    if (isrc) { A.a1BQr += bq; A.a2BQr += bq * bq / SQR_QUAL_DIV; } else { A.a1BQf += bq; A.a2BQf += bq * bq / SQR_QUAL_DIV; }
    A.s[UVC_S_aMQs] += r.mapq;
    A.s[UVC_S_aDPff] += (!strand && !isrc); A.s[UVC_S_aDPfr] += (!strand && isrc);
    A.s[UVC_S_aDPrf] += (strand && !isrc);  A.s[UVC_S_aDPrr] += (strand && isrc);
    if (imin(dist_to_interfering_indel, imin(seg_l_nbases, seg_r_nbases)) >= P.bias_thres_interfering_indel) A.s[UVC_S_aP3] += 1;
    if (0 == r.clip_cnt) A.s[UVC_S_aNC] += 1;
    if (isrc) A.l[UVC_S64_aLIT] += ((r.isize != 0) ? frag_l_nbases2 : 0);
    else      A.l[UVC_S64_aRIT] += ((r.isize != 0) ? frag_r_nbases2 : 0);

    const int _LPxT = T.t[UVC_T_aLPxT], RPxT = T.t[UVC_T_aRPxT];
    const int LPxT = (isGap ? _LPxT : imin(_LPxT, RPxT));
    const bool is_far_from_edge = (seg_l_nbases + ((C_INS == cigar_op) ? (int)nnminus(indel_len, P.microadjust_nobias_pos_indel_maxlen) : 0) >= LPxT) && (seg_r_nbases >= RPxT);
    const int thres_highBAQ = P.bias_thres_highBAQ + (isGap ? 0 : 3);
    const bool is_unaffected_by_edge = (seg_l_baq >= thres_highBAQ && seg_r_baq >= thres_highBAQ);
    const int min_dist2iend = ((r.flag & 0x1) ? imin(frag_l_nbases2, frag_r_nbases2) : (isrc ? seg_r_nbases : seg_l_nbases));
    if (is_far_from_edge && is_unaffected_by_edge && (min_dist2iend > P.primerlen2 || !amplicon)) A.s[UVC_S_aP1] += 1;
    if (is_assay_UMI || !amplicon) A.s[UVC_S_aP2] += 1;

    int ampfact2 = 100;
    if (bq < P.bias_thres_PFBQ1) ampfact2 = 100 * (bq * bq) / (P.bias_thres_PFBQ1 * P.bias_thres_PFBQ1);
    A.s[UVC_S_aPF1] += (isGap ? imin(100, ampfact2) : (100 * ampfact2 / 100));
    ampfact2 = 100;
    if (bq < P.bias_thres_PFBQ2) ampfact2 = 100 * (bq * bq) / (P.bias_thres_PFBQ2 * P.bias_thres_PFBQ2);
    A.s[UVC_S_aPF2] += (isGap ? imin(100, ampfact2) : (100 * ampfact2 / 100));
    if (!isGap) {
        A.s[UVC_S_a2XM2] += (r.xm1500 > 20 ? (100 * (20 * 20) / (r.xm1500 * r.xm1500)) : 100);
        A.s[UVC_S_a2BM2] += (bm1500 > 20 ? (100 * (20 * 20) / (bm1500 * bm1500)) : 100);
    }
    if (((!isGap) && bq >= P.bias_thres_highBQ) || (isGap && dist_to_interfering_indel >= P.bias_thres_interfering_indel)) {
        const bool tier2 = (isGap || bq >= P.bias_thres_highBQ);
        if (is_far_from_edge) {
            long long LPL = 0, RPL = 0;
            bidir(A.s[UVC_S_aLP1], A.s[UVC_S_aLP2], A.s[UVC_S_aRP1], A.s[UVC_S_aRP2], LPL, RPL,
                  T.t[UVC_T_aLP1t], T.t[UVC_T_aLP2t], T.t[UVC_T_aRP1t], T.t[UVC_T_aRP2t], seg_l_nbases, seg_r_nbases, tier2, indel_len);
            A.s[UVC_S_aLPL] += (int)LPL; A.s[UVC_S_aRPL] += (int)RPL;
        }
        if (is_unaffected_by_edge) {
            bidir(A.s[UVC_S_aLB1], A.s[UVC_S_aLB2], A.s[UVC_S_aRB1], A.s[UVC_S_aRB2], A.l[UVC_S64_aLBL], A.l[UVC_S64_aRBL],
                  P.bias_thres_BAQ1, P.bias_thres_BAQ2, P.bias_thres_BAQ1, P.bias_thres_BAQ2, seg_l_baq, seg_r_baq, tier2, 0);
        }
        A.s[UVC_S_aBQ2] += 1;
    }
    const bool mate_ok = ((0 == (r.flag & 0x8)) || (0 == (r.flag & 0x1)));
    const bool is_l_nonbiased = (mate_ok && seg_l_nbases > seg_r_nbases);
    const bool is_r_nonbiased = (mate_ok && seg_l_nbases < seg_r_nbases);
    const bool pos_good = ((!amplicon) || (!normal_filter_primers) || (is_far_from_edge && is_unaffected_by_edge));
    if (isrc) {
        const int d = frag_l_nbases2;
        if ((d >= T.t[UVC_T_aLI1t]) && (d <= T.t[UVC_T_aLI1T] || isGap) && (is_normal || (isGap && is_l_nonbiased))) A.s[UVC_S_aLI1] += 1;
        if ((d >= T.t[UVC_T_aLI2t]) && (d <= T.t[UVC_T_aLI2T] || isGap) && (is_normal || (isGap && is_l_nonbiased))) { if (pos_good) A.s[UVC_S_aLI2] += 1; }
        if (pos_good) A.s[UVC_S_aLIr] += 1;
    } else {
        const int d = frag_r_nbases2;
        if ((d >= T.t[UVC_T_aRI1t]) && (d <= T.t[UVC_T_aRI1T] || isGap) && (is_normal || (isGap && is_r_nonbiased))) A.s[UVC_S_aRI1] += 1;
        if ((d >= T.t[UVC_T_aRI2t]) && (d <= T.t[UVC_T_aRI2T] || isGap) && (is_normal || (isGap && is_r_nonbiased))) { if (pos_good) A.s[UVC_S_aRI2] += 1; }
        if (pos_good) A.s[UVC_S_aRIf] += 1;
    }
}

// Lane masks.  A per-lane condition is kept as the 64-bit ballot of its compare (an SGPR pair), conditions are combined
// on the scalar unit, and a counter takes the mask as the carry-in of one v_addc: one vector instruction per counter.
typedef unsigned long long wmask;
#define BAL(c) __builtin_amdgcn_ballot_w64(c)
DEV wmask umask(bool b) { return b ? ~0ull : 0ull; }   // wave-uniform condition
DEV void addm(int &acc, wmask m) { asm("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(acc) : "s"(m) : "vcc"); }
DEV int selm(wmask m, int v) { int r; asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(v), "s"(m)); return r; }

// dealwith_segbias<true> for LINK_M (lanes with hasL) and dealwith_segbias<false> for the read base (lanes with hasB) at one
// position of a simple alignment: cigar_op = M, indel_len = 0, dist_to_interfering_indel = 10000 (main.hpp:1360-1595).
// Everything that does not depend on the symbol is computed once for both.
// ISRC / STRAND (bam_get_strand, common.hpp:89) are compile-time: the P2 work list is split by them, so the direction-specific
// counters are fixed registers in each instantiation and the loop has no branch on the read's orientation.
// PLAIN: the region holds no amplicon-flagged family, no primer length is set and the reads are long (is_high_readlen), so the amplicon arms
// and the microadjust arm are compiled out.
// The tables of the PFBQ factor hold the values -256 .. 255 (a value is below 0 with a negative bq_phred_added_misma, never below the addend, which
// uvcgpu_params_check keeps at -256 or above; above 255 the factor is 100 as at 255 while the thresholds stay below 256): one v_med3 and a constant offset.
#define AMP_LO 256
#define AMP_AT(bq) (imax(imin((bq), 255), -AMP_LO) + AMP_LO)
template <bool ISRC, bool STRAND, bool PLAIN>
DEV void segbias_simple(SegAcc &AL, SegAcc &AB, const UvcParams &P, const SegRead &r, const PosThres &T, int rpos, long long baq_p, long long baq2_p,
                        bool hasL, bool hasB, int bqL, int bqB, int xm_inc, int bm_inc, const int *amp1, const int *amp2) {
    const bool amplicon = (PLAIN ? false : is_assay_amplicon(r.dflag, P));
    const bool normal_filter_primers = normal_filters_primers(P);
    const bool is_assay_UMI = (r.dflag & UVC_DFLAG_UMI);
    constexpr bool isrc = ISRC, strand = STRAND;
    const bool is_normal = ((r.isize != 0) || (0 == (r.flag & 0x1)));
    const bool mate_ok = ((0 == (r.flag & 0x8)) || (0 == (r.flag & 0x1)));
    // PLAIN also means is_high_readlen (main.hpp:1404): the microadjust arm (two full-width integer multiplies per read and wave, quarter rate) is compiled out
    const bool hrl = (PLAIN ? true : (P.central_readlen >= P.microadjust_median_readlen_thres));
    const int l_nb = rpos - r.pos + 1, r_nb = r.rend - rpos;
    // differences of BAQ prefix sums: truncation to 32 bits commutes with the subtraction
    const int l_baq1 = (int)((unsigned)baq_p - (unsigned)r.baq_pos + 1u);
    const int r_baq1B = (int)((unsigned)r.baq_last - (unsigned)baq_p + 1u);
    const int r_baq1L = imin(r_baq1B, (int)((unsigned)r.baq2_last - (unsigned)baq2_p + 7u));
    const int kb = P.microadjust_BAQ_per_base_x1024;
    const int l_baq = (hrl ? l_baq1 : imax(l_baq1, l_nb * kb / 1024));
    const int r_baqB = (hrl ? r_baq1B : imax(r_baq1B, r_nb * kb / 1024));
    const int r_baqL = (hrl ? r_baq1L : imax(r_baq1L, r_nb * kb / 1024));
    const bool has_isize = (r.isize != 0);
    const int fl2 = (has_isize ? imin(rpos - r.frag_pos_L + 1, MAX_INSERT_SIZE) : MAX_INSERT_SIZE);
    const int fr2 = (has_isize ? imin(r.frag_pos_R - rpos, MAX_INSERT_SIZE) : MAX_INSERT_SIZE);
    // masks
    const wmask m_p3 = BAL(imin(10000, imin(l_nb, r_nb)) >= P.bias_thres_interfering_indel);
    const int LPxT_L = T.t[UVC_T_aLPxT], RPxT = T.t[UVC_T_aRPxT], LPxT_B = imin(LPxT_L, RPxT);
    const wmask m_rfar = BAL(r_nb >= RPxT);
    const wmask m_farL = BAL(l_nb >= LPxT_L) & m_rfar, m_farB = BAL(l_nb >= LPxT_B) & m_rfar;
    const int hb = P.bias_thres_highBAQ;
    const wmask m_unaffL = BAL(l_baq >= hb) & BAL(r_baqL >= hb), m_unaffB = BAL(l_baq >= hb + 3) & BAL(r_baqB >= hb + 3);
    const int min_dist2iend = ((r.flag & 0x1) ? imin(fl2, fr2) : (isrc ? r_nb : l_nb));
    const wmask m_iend = umask(!amplicon) | BAL(min_dist2iend > P.primerlen2);
    const wmask m_lp1 = BAL(l_nb >= T.t[UVC_T_aLP1t]), m_lp2 = BAL(l_nb >= T.t[UVC_T_aLP2t]);
    const wmask m_rp1 = BAL(r_nb >= T.t[UVC_T_aRP1t]), m_rp2 = BAL(r_nb >= T.t[UVC_T_aRP2t]);
    const wmask m_lb1 = BAL(l_baq >= P.bias_thres_BAQ1), m_lb2 = BAL(l_baq >= P.bias_thres_BAQ2);
    const wmask m_goodU = umask((!amplicon) || (!normal_filter_primers));
    const wmask m_goodL = m_goodU | (m_farL & m_unaffL), m_goodB = m_goodU | (m_farB & m_unaffB);
    // insert-end thresholds of this read's direction
    const int d = (isrc ? fl2 : fr2);
    wmask m_i1lo, m_i1hi, m_i2lo, m_i2hi, m_nonb;
    if (isrc) {
        m_i1lo = BAL(d >= T.t[UVC_T_aLI1t]); m_i1hi = BAL(d <= T.t[UVC_T_aLI1T]); m_i2lo = BAL(d >= T.t[UVC_T_aLI2t]); m_i2hi = BAL(d <= T.t[UVC_T_aLI2T]);
        m_nonb = BAL(l_nb > r_nb);
    } else {
        m_i1lo = BAL(d >= T.t[UVC_T_aRI1t]); m_i1hi = BAL(d <= T.t[UVC_T_aRI1T]); m_i2lo = BAL(d >= T.t[UVC_T_aRI2t]); m_i2hi = BAL(d <= T.t[UVC_T_aRI2T]);
        m_nonb = BAL(l_nb < r_nb);
    }
    const wmask m_okB = umask(is_normal), m_okL = m_okB | (umask(mate_ok) & m_nonb);
    const int p2 = (is_assay_UMI || !amplicon), nc = (0 == r.clip_cnt);
    auto common = [&](SegAcc &A, int bq) {
        const int bq2 = (int)((unsigned)__mul24(bq, bq) / SQR_QUAL_DIV);   // |bq| < 2^12 (below 0 with a negative bq_phred_added_misma; uvcgpu_params_check keeps the addends within -256 .. 3840): the signed 24-bit multiply is exact and full rate
        if (isrc) { A.a1BQr += bq; A.a2BQr += bq2; } else { A.a1BQf += bq; A.a2BQf += bq2; }
        A.bq += bq;
        A.s[UVC_S_aMQs] += r.mapq;
        if (strand) { if (isrc) A.s[UVC_S_aDPrr] += 1; else A.s[UVC_S_aDPrf] += 1; }
        else        { if (isrc) A.s[UVC_S_aDPfr] += 1; else A.s[UVC_S_aDPff] += 1; }
        addm(A.s[UVC_S_aP3], m_p3);
        A.s[UVC_S_aNC] += nc; A.s[UVC_S_aP2] += p2;
        if (has_isize) { if (isrc) A.lp[UVC_S64_aLIT] += fl2; else A.lp[UVC_S64_aRIT] += fr2; }
    };
    // (in_all: `in` is one wave-uniform mask, all lanes or none -- a mask, not a branch around the block: the loop has no branch per read for it)
    auto bias = [&](SegAcc &A, bool in_all, wmask in, wmask far, wmask unaff, wmask m_rb1, wmask m_rb2, int r_baq) {
        const wmask a = (in & far), b = (in & unaff);
        addm(A.s[UVC_S_aLP1], a & m_lp1); addm(A.s[UVC_S_aLP2], a & m_lp2); addm(A.s[UVC_S_aRP1], a & m_rp1); addm(A.s[UVC_S_aRP2], a & m_rp2);
        A.s[UVC_S_aLPL] += selm(a, l_nb); A.s[UVC_S_aRPL] += selm(a, r_nb);
        addm(A.s[UVC_S_aLB1], b & m_lb1); addm(A.s[UVC_S_aLB2], b & m_lb2); addm(A.s[UVC_S_aRB1], b & m_rb1); addm(A.s[UVC_S_aRB2], b & m_rb2);
        A.lp[UVC_S64_aLBL] += selm(b, l_baq); A.lp[UVC_S64_aRBL] += selm(b, r_baq);
        if (in_all) A.s[UVC_S_aBQ2] += (in ? 1 : 0); else addm(A.s[UVC_S_aBQ2], in);
        addm(A.s[UVC_S_aP1], far & unaff & m_iend);
    };
    if (hasB) {
        common(AB, bqB);
        AB.s[UVC_S_aPF1] += amp1[AMP_AT(bqB)]; AB.s[UVC_S_aPF2] += amp2[AMP_AT(bqB)];   // "100 * amp / 100" == amp (main.hpp:1472-1519)
        AB.s[UVC_S_a2XM2] += xm_inc; AB.s[UVC_S_a2BM2] += bm_inc;
        // the base side enters the bias blocks when bq >= highBQ (tier2 then holds)
        bias(AB, false, BAL(bqB >= P.bias_thres_highBQ), m_farB, m_unaffB, BAL(r_baqB >= P.bias_thres_BAQ1), BAL(r_baqB >= P.bias_thres_BAQ2), r_baqB);
        if (isrc) { addm(AB.s[UVC_S_aLI1], m_i1lo & m_i1hi & m_okB); addm(AB.s[UVC_S_aLI2], m_i2lo & m_i2hi & m_okB & m_goodB); addm(AB.s[UVC_S_aLIr], m_goodB); }
        else      { addm(AB.s[UVC_S_aRI1], m_i1lo & m_i1hi & m_okB); addm(AB.s[UVC_S_aRI2], m_i2lo & m_i2hi & m_okB & m_goodB); addm(AB.s[UVC_S_aRIf], m_goodB); }
    }
    if (hasL) {
        common(AL, bqL);
        AL.s[UVC_S_aPF1] += imin(100, amp1[AMP_AT(bqL)]); AL.s[UVC_S_aPF2] += imin(100, amp2[AMP_AT(bqL)]);
        // the gap side enters when dist_to_interfering_indel (10000) >= bias_thres_interfering_indel
        bias(AL, true, umask(10000 >= P.bias_thres_interfering_indel), m_farL, m_unaffL, BAL(r_baqL >= P.bias_thres_BAQ1), BAL(r_baqL >= P.bias_thres_BAQ2), r_baqL);   // (aP1 inside does not look at `in`)
        if (isrc) { addm(AL.s[UVC_S_aLI1], m_i1lo & m_okL); addm(AL.s[UVC_S_aLI2], m_i2lo & m_okL & m_goodL); addm(AL.s[UVC_S_aLIr], m_goodL); }
        else      { addm(AL.s[UVC_S_aRI1], m_i1lo & m_okL); addm(AL.s[UVC_S_aRI2], m_i2lo & m_okL & m_goodL); addm(AL.s[UVC_S_aRIf], m_goodL); }
    }
}

DEV void load_thres(const RegionDev &R, PosThres &T, int64_t x) {
#pragma unroll
    for (int f = 0; f < UVC_NTHRES; f++) T.t[f] = TH(R, f, x);
}

// primer gating of updateByAln, main.hpp:1872-1875, 1895
DEV void primer_window(const UvcParams &P, const AlnRec &a, int &ibeg, int &iend) {
    const bool isrc = (a.flag & 0x10) != 0;
    ibeg = ((a.isize != 0) ? (imin(a.pos, a.mpos) + P.primerlen) : ((isrc && (0x0 == (0x1 & a.flag))) ? 0 : (a.pos + P.primerlen)));
    iend = ((a.isize != 0) ? (int)nnminus(imin(a.pos, a.mpos) + abs(a.isize), P.primerlen) : ((isrc && (0x0 == (0x1 & a.flag))) ? (int)nnminus(a.rend, P.primerlen) : INT32_MAX));
}

// ------------------------------------------------------------------------------------------------
// k_aln_prelude: one thread per alignment (main.hpp:1795-1885 prelude of updateByAln)
// ------------------------------------------------------------------------------------------------

// does the read have an InDel next to low base qualities (main.hpp:1817-1859)?  Then dist_to_interfering_indel varies along the
// read and its M runs cannot take the simple path of k_p2_fast.
DEV bool has_lowbq_indel(const UvcParams &P, const AlnRec &a, const uint32_t *cigar, const uint8_t *quals) {
    auto Q = [&](int q) -> int { return (int)quals[imin(imax(q, 0), a.l_qseq - 1)]; };
    int qpos = 0;
    for (int i = 0; i < a.n_cigar; i++) {
        const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
        if (op == C_MATCH || op == C_EQUAL || op == C_DIFF || op == C_SOFT_CLIP) qpos += len;
        else if (op == C_INS) {
            for (int q2 = qpos - imin(qpos, 1); q2 < imin(qpos + len + 1, a.rend); q2++) if (Q(q2) < P.bias_thres_interfering_indel_BQ) return true;
            qpos += len;
        } else if (op == C_DEL) {
            if (imin(Q(imax(1, qpos) - 1), Q(qpos)) <= P.bias_thres_interfering_indel_BQ) return true;
        }
    }
    return false;
}

// digest of alignment `a` (index `id`) for the position-centric kernels, covering [cbeg, cend) with query offset qb_lo; m_run: the entry is
// an M run of an InDel read (FREC_M_RUN: P1 leaves the read to k_prep_slow), not a whole simple alignment
DEV void fill_fastrec(FastRec &f, const AlnRec &a, int id, int cbeg, int cend, int32_t qb_lo, bool m_run) {
    f.pos = cbeg; f.rend = cend; f.qb_lo = qb_lo; f.aln = id;
    f.fmd = (a.flag & 0xFFFF) | ((a.mapq & 0xFF) << 16) | ((a.dflag & 0xFF) << 24); f.isize = a.isize; f.mpos = a.mpos; f.xm1500 = a.xm1500;
    // per-read constants of dealwith_segbias<false>: the a2XM2 / a2BM2 increments (main.hpp:1521-1522), each <= 100
    int bv[5];
    for (int s2 = 0; s2 < 5; s2++) bv[s2] = (a.bm1500[s2] > 20 ? (100 * (20 * 20) / (a.bm1500[s2] * a.bm1500[s2])) : 100);
    const int xv = (a.xm1500 > 20 ? (100 * (20 * 20) / (a.xm1500 * a.xm1500)) : 100);
    f.bmv = bv[0] | (bv[1] << 8) | (bv[2] << 16) | (bv[3] << 24); f.xbv = bv[4] | (xv << 8) | (m_run ? FREC_M_RUN : 0);
    f.bm4c = ((a.clip_cnt & 0xF) << 16) | (a.nogap_penal & 0xFFFF);   // nogap_penal is negative when NM < the InDel lengths
    f.clips = imin(a.lclip_oplen, FREC_CLIP_MAX) | (imin(a.rclip_oplen, FREC_CLIP_MAX) << 16);   // saturated: frec_clip_len reads a full half from alns[]
    f.baq_pos = (int32_t)a.baq_pos; f.baq_last = (int32_t)a.baq_last; f.baq2_last = (int32_t)a.baq2_last;
    f.ext = ((cbeg - a.pos) & 0xFFFF) | ((a.rend - cend) << 16);
}

// Work list of P1 and P2: entry j covers [cbeg[j], cend[j]) of alignment aln[j] (sorted by (class, cbeg)).  The entry of a simple alignment
// is the record k_aln_prelude wrote straight into its slot (RawReads::fast_rank); only the M runs of InDel reads are built here, from the
// alignment records the prelude made.
__global__ void __launch_bounds__(256) k_build_p2list(RegionDev R, const int32_t *fast_rank, const int32_t *aln, const int32_t *cbeg, const int32_t *cend, const int32_t *qb) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= R.n_fast2) return;
    const int id = aln[j];
    if (fast_rank[id] >= 0) return;
    FastRec f;
    const AlnRec &a = R.alns[id];
    // an InDel read that k_aln_prelude found ineligible keeps its slot (the list stays sorted) but covers nothing
    fill_fastrec(f, a, id, cbeg[j], (a.kind == 1 ? cbeg[j] : cend[j]), qb[j], true);
    R.frec2[j] = f;
}

// Mismatching bases per base symbol (bm1500s, main.hpp:1860-1863) of the simple alignments.  Eight lanes per alignment, eight bases per lane
// and step: read bases and reference codes are bytes below 0x80, so "differs" and "is symbol s" are byte-parallel tests on two 8-byte words
// (unaligned loads: the hardware takes them) and a count is a popcount.  The eight lanes of an alignment read 64 consecutive bytes, so a
// load of the wave touches eight cache lines; with a lane per alignment it touched 64 (8 bytes of each, 150 bytes apart) and the kernel was
// bound by the L2 -> L1 traffic of lines read sixteen times over (0.39 ms per 2 M reads; a wave per alignment was 0.59 ms, a thread per
// alignment walking byte by byte 2.0 ms).  The five counts wait in the alignment's own FastRec slot of the work list.
DEV unsigned long long load8u(const uint8_t *p) { unsigned long long v; __builtin_memcpy(&v, p, 8); return v; }
__global__ void __launch_bounds__(256) k_aln_bm(RegionDev R, RawReads W) {
    const unsigned long long K7F = 0x7F7F7F7F7F7F7F7FULL, K80 = 0x8080808080808080ULL, K01 = 0x0101010101010101ULL;
    const int sub = threadIdx.x & 7;
    for (int id = (blockIdx.x * blockDim.x + threadIdx.x) >> 3; id < R.n_alns; id += (gridDim.x * blockDim.x) >> 3) {
        const int rk = W.fast_rank[id];
        if (rk < 0) continue;   // (the eight lanes of the alignment leave together)
        const int pos = W.pos[id], len = W.endpos[id] - pos;
        const uint32_t c0 = R.cigars[W.cigar_off[id]];
        const uint8_t *b = R.bases + W.seq_off[id] + (cig_op(c0) == C_SOFT_CLIP ? cig_len(c0) : 0);
        const uint8_t *rf = R.refsym + (pos - R.beg);
        int cnt[5] = { 0, 0, 0, 0, 0 };
        for (int k = 8 * sub; k + 8 <= len; k += 64) {
            const unsigned long long bb = load8u(b + k), rr = load8u(rf + k);
            const unsigned long long mism = ((bb ^ rr) + K7F) & K80;          // 0x80 in every byte that differs (all bytes are < 0x80)
#pragma unroll
            for (int s2 = 0; s2 < 5; s2++) cnt[s2] += __popcll(mism & ~((bb ^ (K01 * (unsigned)s2)) + K7F) & K80);
        }
        { const int k = (len & ~7) + sub;   // the last len % 8 bases, one per lane
          if (k < len) { const int bs = b[k]; const bool mm = (bs != rf[k]);
#pragma unroll
                         for (int s2 = 0; s2 < 5; s2++) cnt[s2] += (mm && bs == s2); } }
#pragma unroll
        for (int s2 = 0; s2 < 5; s2++) cnt[s2] = wave_sum<8>(cnt[s2]);   // over the read's eight lanes
        if (sub == 0) {
            int32_t *dst = (int32_t *)&R.frec2[rk];
#pragma unroll
            for (int s2 = 0; s2 < 5; s2++) dst[s2] = cnt[s2];
        }
    }
}

// the prelude of one alignment; returns the number of its bases that go through the mismatch queue of k_p2_fast
DEV int aln_prelude_one(const RegionDev &R, const RawReads &W, const UvcParams &P, const int id, AlnRec &out) {
    AlnRec a;
    a.pos = W.pos[id]; a.rend = W.endpos[id]; a.mpos = W.mpos[id]; a.isize = W.isize[id]; a.flag = W.flag[id]; a.mapq = W.mapq[id];
    a.dflag = W.dflag[id]; a.l_qseq = W.l_qseq[id]; a.seq_off = W.seq_off[id]; a.cigar_off = W.cigar_off[id]; a.table_off = W.table_off[id]; a.item_off = W.item_off[id]; a.gap_off = W.gap_off[id];
    a.n_cigar = W.n_cigar[id]; a.kind = W.kind[id]; a.frag = W.frag[id]; a.fs = W.fs[id]; a.id = id;
    const uint32_t *cigar = R.cigars + a.cigar_off;
    const uint8_t *bases = R.bases + a.seq_off;
    int nge = 0, ngo = 0, clip_cnt = 0;
    for (int i = 0; i < a.n_cigar; i++) {
        const int op = cig_op(cigar[i]);
        if (C_INS == op || C_DEL == op) { nge += cig_len(cigar[i]); ngo++; }
        if (C_SOFT_CLIP == op || C_HARD_CLIP == op) clip_cnt++;
        if (op > C_DIFF) atomicExch(R.err, UVCGPU_EUNSUPPORTED);   // BAM_CBACK etc.: process_cigar throws, main_conversion.hpp:911-915
    }
    const int nm_cnt = (W.nm[id] >= 0 ? W.nm[id] : nge);
    const int qlen = a.rend - a.pos;
    a.xm1500 = (nm_cnt - nge) * 1500 / qlen;
    a.go1500 = ngo * 1500 / qlen;
    a.clip_cnt = clip_cnt;
    int bm[5] = { 0, 0, 0, 0, 0 };
    int qpos = 0, rpos = a.pos, lclip_q = 0, m_index = -1;
    const int rk0 = W.fast_rank[id];
    if (rk0 >= 0) {   // simple alignment: k_aln_bm counted its mismatching bases with a whole wave and left them in this read's own FastRec slot
        const int32_t *pre = (const int32_t *)&R.frec2[rk0];
        for (int s2 = 0; s2 < 5; s2++) bm[s2] = pre[s2];
        for (int i = 0; i < a.n_cigar && m_index < 0; i++) {
            const int op = cig_op(cigar[i]);
            if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) { m_index = i; lclip_q = qpos; }
            else if (op == C_SOFT_CLIP) qpos += cig_len(cigar[i]);
        }
    } else
    for (int i = 0; i < a.n_cigar; i++) {
        const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
        if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) {
            if (m_index < 0) { m_index = i; lclip_q = qpos; }
            for (int k = 0; k < len; k++) { const int b = bases[qpos]; if (R.refsym[rpos - R.beg] != b) bm[b] += 1; qpos++; rpos++; }
        } else if (op == C_INS || op == C_SOFT_CLIP) qpos += len;
        else if (op == C_DEL || op == C_REF_SKIP) rpos += len;
    }
    for (int s = 0; s < 5; s++) a.bm1500[s] = bm[s] * 1500 / qlen;
    a.lclip_len = ((a.n_cigar > 0 && cig_op(cigar[0]) == C_SOFT_CLIP) ? cig_len(cigar[0]) : 0);
    a.rclip_len = ((a.n_cigar > 0 && cig_op(cigar[a.n_cigar - 1]) == C_SOFT_CLIP) ? cig_len(cigar[a.n_cigar - 1]) : 0);
    const int by_clip = imax(a.lclip_len, a.rclip_len) / 6;
    const int by_nm = (a.xm1500 + a.go1500) / 30;
    a.indel_penal = imin(1, by_nm + by_clip);
    a.nogap_penal = imin(4, by_nm + by_clip) + 1;
    // NM below the InDel lengths (malformed, but the reference computes with it) makes the penalties negative; the 16-bit value
    // fields of Item / Contrib hold the results down to here
    if (by_nm + by_clip < -30000) atomicExch(R.err, UVCGPU_EUNSUPPORTED);   // (an NM tag tens of thousands below the InDel lengths of the read)
    a.lclip_q = lclip_q; a.m_index = m_index;
    a.lclip_oplen = 0; a.rclip_oplen = 0;
    if (a.kind == 0) {
        if (m_index > 0) a.lclip_oplen = cig_len(cigar[m_index - 1]);
        if (m_index + 1 < a.n_cigar) a.rclip_oplen = cig_len(cigar[m_index + 1]);
    }
    a.qbase = a.seq_off + lclip_q - a.pos;
    a.baq_pos = BAQ1(R, a.pos); a.baq_last = BAQ1(R, a.rend - 1); a.baq2_last = BAQ2(R, a.rend - 1);
    if (a.kind == 2 && has_lowbq_indel(P, a, cigar, R.quals + a.seq_off)) a.kind = 1;
    const int rk = W.fast_rank[id];
    int n_mis = 0;
    a.n_mutc = bm[0] + bm[1] + bm[2] + bm[3] + bm[4] + ngo;
    out = a;
    if (rk >= 0 || W.kind[id] == 2) n_mis = bm[0] + bm[1] + bm[2] + bm[3] + bm[4];   // every alignment that can be on the P2 work list: its mismatching bases go through the mismatch queue
    if (rk >= 0) {
        FastRec f;
        fill_fastrec(f, a, id, a.pos, a.rend, (int32_t)(a.qbase & 0xFFFFFFFFLL), false);
        R.frec2[rk] = f;
    }
    return n_mis;
}
// One thread per alignment.  The 200-byte records leave through LDS: written from registers, a lane's record is 25 stores that each touch 64
// cache lines of the wave; the block's 256 records are one contiguous 51 200-byte span of alns[] and are copied out with coalesced 16-byte stores.
__global__ void __launch_bounds__(256) k_aln_prelude(RegionDev R, RawReads W, UvcParams P) {
    static_assert(sizeof(AlnRec) % 8 == 0 && (256 * sizeof(AlnRec)) % 16 == 0, "the staged copy moves the block's records as 16-byte words");
    __shared__ __attribute__((aligned(16))) AlnRec stage[256];
    const int id0 = blockIdx.x * blockDim.x, id = id0 + threadIdx.x;
    __shared__ int mis_s[4];
    const int n_mis = (id < R.n_alns) ? aln_prelude_one(R, W, P, id, stage[threadIdx.x]) : 0;
    // one atomic per block: same-address atomics serialise.  (The barrier inside also orders the records in `stage` before the copy below.)
    const int t = waves_sum<4>(wave_sum(n_mis), mis_s);
    if (threadIdx.x == 0 && t) atomicAdd(R.mis_total, (unsigned long long)t);
    const int nrec = imin(256, R.n_alns - id0);
    if (nrec == 256) {
        const uint4 *src = (const uint4 *)&stage[0]; uint4 *dst = (uint4 *)(R.alns + id0);
        for (int i = threadIdx.x; i < (int)(256 * sizeof(AlnRec) / 16); i += 256) dst[i] = src[i];
    } else {
        const unsigned long long *src = (const unsigned long long *)&stage[0]; unsigned long long *dst = (unsigned long long *)(R.alns + id0);
        for (int i = threadIdx.x; i < nrec * (int)(sizeof(AlnRec) / 8); i += 256) dst[i] = src[i];
    }
}

// ------------------------------------------------------------------------------------------------
// P1 (update_seg_format_prep_sets_by_aln, main.hpp:924-1204)
// ------------------------------------------------------------------------------------------------
// SNV / DNV run detection started at ref position s of alignment a (main.hpp:1025-1046).
// `q_of_r` maps the walk to the query: the reference advances query and reference together
// regardless of the CIGAR, so q = q_s + (r - s).
DEV void snv_dnv_scatter(const RegionDev &R, const uint8_t *qbases, int q_s, int l_qseq, int apos, int rend, int s) {
    int nq = q_s, nr = s;
    int refsymbol = UVC_BASE_NN, readsymbol = UVC_NUM_SYMBOLS;
    while (refsymbol != readsymbol && nq < l_qseq && nr < rend) {
        refsymbol = R.refsym[nr - R.beg];
        readsymbol = qbases[nq];
        nq++; nr++;
    }
    if (nr == s + 2) for (int r = imax(apos, s - 1); r < imin(nr, rend); r++) atomicAdd(&P32(R, UVC_P_a_snv_dp, r - R.beg), 1);
    if (nr > s + 2)  for (int r = imax(apos, s - 1); r < imin(nr, rend); r++) atomicAdd(&P32(R, UVC_P_a_dnv_dp, r - R.beg), 1);
}

DEV void clip_event(const RegionDev &R, const UvcParams &P, int rpos, int i, int len, int pcr_dp_inc) {   // main.hpp:1183-1199
    const int delta = ((0 == i) ? 0 : -1);
    if (pcr_dp_inc) {
        for (int r2 = rpos + delta - P.microadjust_near_clip_dist; r2 <= rpos + delta + P.microadjust_near_clip_dist; r2++)
            if (R.beg <= r2 && r2 < R.end) atomicAdd(&P32(R, UVC_P_a_near_pcr_clip_dp, r2 - R.beg), pcr_dp_inc);
    }
    if ((0 == pcr_dp_inc) && (len >= P.microadjust_alignment_clip_min_len)) {
        const int r2 = rpos + delta;
        if (R.beg <= r2 && r2 < R.end) atomicAdd(&P32(R, UVC_P_a_near_long_clip_dp, r2 - R.beg), 1);
    }
}

// The clip op length of a simple alignment from one 16-bit half of FastRec::clips.  A half below FREC_CLIP_MAX is the length itself; a full
// half stands for "65 535 or more" (a BAM op length has 28 bits: the hard clip of a supplementary alignment of an ultra-long read) and the
// length comes from the alignment's own record, so that every microadjust_alignment_clip_min_len compares with the CIGAR's value.
DEV int frec_clip_len(const RegionDev &R, int half, int aln, bool right) {
    if (half < FREC_CLIP_MAX) return half;
    return right ? R.alns[aln].rclip_oplen : R.alns[aln].lclip_oplen;
}

DEV int simple_base_value(const UvcParams &P, const AlnRec &a, int p, const uint8_t *quals_qbase, bool proton);

// A mismatching base of a simple alignment: decide with the reference's fragment consensus (main.hpp:2658-2726) whether
// position p is a high-quality mutation of the fragment and, if so, record it once (by the first mismatching alignment).
DEV void mut_event(const RegionDev &R, const UvcParams &P, const AlnRec &a, int p, int my_ref) {
    const FragRec &f = R.frags[a.frag];
    if (f.stat_kind != FRAG_STAT_EVENTS) return;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    int m[6] = { 0, 0, 0, 0, 0, 0 };
    int first_mis = -1;
    for (int k = f.aln_beg; k < f.aln_end; k++) {
        const AlnRec &al = R.alns[k];
        if (p < al.pos || p >= al.rend) continue;
        const int sym = R.bases[al.qbase + p];
        if (sym != my_ref && first_mis < 0) first_mis = k;
        const int v = simple_base_value(P, al, p, R.quals + al.qbase, proton);
        m[sym] = imax(m[sym], v);
    }
    if (first_mis != a.id) return;
    int cs = UVC_BASE_NN, cc = 0, ct = 0;
    for (int s2 = 0; s2 < 6; s2++) { if (cc < m[s2]) { cs = s2; cc = m[s2]; } ct += m[s2]; }
    const int con_qual = cc * 2 - ct;
    const bool highBQ = (proton ? true : (con_qual >= P.bias_thres_highBQ));
    if (symbols_mutated(my_ref, cs) && highBQ) {
        const int idx = atomicAdd(&R.frag_nmut[a.frag], 1);
        if (idx < UVC_MAXEV) R.frag_mut[(size_t)a.frag * UVC_MAXEV + idx] = p;
    }
}

#define PREPQ_CAP 192   // per-wave LDS queue of the bases that differ from the reference, see prepq_entry
// An entry of the LDS queues of P1: x = FastRec::aln, with PREPQ_MRUN when the base belongs to an M run of an InDel read (k_prep_slow has that
// read: only the base's item is made); y = position - `origin` (the window's or the tile's first position) | symbol << 16 | quality << 24.
#define PREPQ_MRUN ((int)0x80000000u)
DEV int2 prepq_entry(int aln, bool mrun, int p, int origin, int sym, int q) { return make_int2(aln | (mrun ? PREPQ_MRUN : 0), (int)((unsigned)(p - origin) | ((unsigned)sym << 16) | ((unsigned)q << 24))); }
DEV int prepq_aln(int2 e) { return e.x & ~PREPQ_MRUN; }
DEV int prepq_pos(int2 e, int origin) { return origin + (e.y & 0xFFFF); }
// P1 makes the mismatch queue of k_p2_mism where the accumulate says misq=p1: entry e goes to slot `slot` of RegionDev::mis
// (the caller's atomicAdd on mis_cnt gave the slots of its batch) as the item the plain base pass would have queued
DEV void mis_emit(const RegionDev &R, const UvcParams &P, int2 e, int origin, int slot) {
    if (slot < R.mis_cap) { MisItem it; it.rank = prepq_aln(e); it.epos = prepq_pos(e, origin); it.symval = (int)(((unsigned)e.y >> 16) & 0xFFu) | (base_value((int)((unsigned)e.y >> 24), P) << 8); R.mis[slot] = it; }
    else atomicExch(R.err, UVCGPU_EDEVICE);   // cannot happen: the queue holds every mismatching base of the work list (RegionDev::mis_total)
}
// ------------------------------------------------------------------------------------------------
// k_prep_sums: the P1 counters of the simple alignments that do not depend on the bases, as interval sums (the scheme of k_frag_sums).
// a_dp, a_pcr_dp, a_umi_dp, a_qlen, a_XM1500, a_LIDP, a_RIDP are sums of per-read constants over the reads that cover a position;
// a_LI / a_RI add min(distance to the insert end, MAX_INSERT_SIZE) (main.hpp:1006-1017), which is p * A(p) + B(p) with A the number of
// covering reads on the linear piece and B the sum of their offsets plus MAX_INSERT_SIZE per read on the clamped piece.  One block per
// tile: a lane per read adds +v / -v at the ends of its pieces in LDS, prefix sums, plain stores (the planes are zero; k_prep_fast and
// k_prep_slow add theirs with atomics afterwards).  k_prep_fast keeps the queue of mismatching bases and the counters behind base quality.
// ------------------------------------------------------------------------------------------------
#define PSUM_TILE 1024
enum { PS_DP = 0, PS_PCR, PS_UMI, PS_QLEN, PS_XM, PS_LIDP, PS_RIDP, PS_LIA, PS_RIA, PS_N32 };
__global__ void __launch_bounds__(256) k_prep_sums(RegionDev R, UvcParams P) {
    __shared__ int d[PS_N32][PSUM_TILE + 1];
    __shared__ unsigned long long d64[2][PSUM_TILE + 1];   // B of a_LI, a_RI
    __shared__ int wtot[4];
    __shared__ unsigned long long wtot64[4];
    const int t0 = R.beg + (int)blockIdx.x * PSUM_TILE, t1 = imin(t0 + PSUM_TILE, R.beg + (int)R.npos);
    for (int i = threadIdx.x; i < PS_N32 * (PSUM_TILE + 1); i += 256) (&d[0][0])[i] = 0;
    for (int i = threadIdx.x; i < 2 * (PSUM_TILE + 1); i += 256) (&d64[0][0])[i] = 0ull;
    __syncthreads();
    const int w_first = (int)blockIdx.x * (PSUM_TILE / 64), w_last = imin(w_first + PSUM_TILE / 64, R.nwin) - 1;
    auto put = [&](int f, int a, int b, int v) { if (v != 0) diff_put(d[f], t0, t1, a, b, v); };   // += v on [a, b) of plane f, clipped to the tile
    auto put64 = [&](int f, int a, int b, long long v) { if (v != 0) diff_put(d64[f], t0, t1, a, b, (unsigned long long)v); };
    for (int cls = 0; cls < 4; cls++) {   // the four class sub-lists of the work list: the sums do not depend on the order of the reads
    const int lo = win_lo(R, 1 + cls, w_first), hi = win_hi(R, 1 + cls, w_last);
    for (int k = lo + (int)threadIdx.x; k < hi; k += 256) {
        const int4 *q4 = (const int4 *)(R.frec2 + k);
        const int4 h0 = q4[0], h1 = q4[1];   // pos rend qb_lo aln | fmd isize mpos xm1500
        const int apos = h0.x, rend = h0.y;
        if (rend <= t0 || apos >= t1) continue;
        if (((const int *)q4)[9] & FREC_M_RUN) continue;   // FastRec::xbv: an M run of an InDel read (k_prep_slow has the read)
        const int dflag = (h1.x >> 24) & 0xFF;
        put(PS_DP, apos, rend, 1); put(PS_PCR, apos, rend, (dflag & UVC_DFLAG_AMPLICON) ? 1 : 0); put(PS_UMI, apos, rend, (dflag & UVC_DFLAG_UMI) ? 1 : 0);
        put(PS_QLEN, apos, rend, rend - apos); put(PS_XM, apos, rend, h1.w);
        if (h1.y != 0) {
            const int fl = imin(apos, h1.z);
            if (h1.x & 0x10) {   // a_LI: min(p - fl + 1, MAX) = p + (1 - fl) while p < fl + MAX
                const int brk = imax(apos, imin(rend, (int)lmin((long long)fl + MAX_INSERT_SIZE, (long long)INT32_MAX)));
                put(PS_LIDP, apos, rend, 1);
                put(PS_LIA, apos, brk, 1); put64(0, apos, brk, 1LL - fl); put64(0, brk, rend, MAX_INSERT_SIZE);
            } else {             // a_RI: min(fr - p, MAX) = fr - p once p > fr - MAX
                const long long fr = (long long)fl + (long long)abs(h1.y);
                const int brk = imax(apos, imin(rend, (int)lmax(lmin(fr - MAX_INSERT_SIZE + 1, (long long)INT32_MAX), (long long)INT32_MIN)));
                put(PS_RIDP, apos, rend, 1);
                put64(1, apos, brk, MAX_INSERT_SIZE); put(PS_RIA, brk, rend, 1); put64(1, brk, rend, fr);
            }
        }
    }
    }
    __syncthreads();
    const int n_here = t1 - t0;
    const int64_t xb = (int64_t)blockIdx.x * PSUM_TILE;
    int liA[4] = {0, 0, 0, 0}, riA[4] = {0, 0, 0, 0};
    const int plane_of[PS_N32] = { UVC_P_a_dp, UVC_P_a_pcr_dp, UVC_P_a_umi_dp, UVC_P_a_qlen, UVC_P_a_XM1500, UVC_P_a_LIDP, UVC_P_a_RIDP, -1, -1 };
#pragma unroll 1
    for (int f = 0; f < PS_N32; f++) {   // (one body for the nine planes)
        int v[4];
        const int before = block_excl<4>(diff_run<4>(d[f], v), wtot);
        __syncthreads();   // wtot is written again in the next round
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = threadIdx.x * 4 + i, val = before + v[i];
            if (f == PS_LIA) liA[i] = val; else if (f == PS_RIA) riA[i] = val;
            else if (x < n_here && val != 0) P32(R, plane_of[f], xb + x) = val;
        }
    }
    for (int f = 0; f < 2; f++) {
        unsigned long long v[4];
        const unsigned long long before = block_excl<4>(diff_run<4>(d64[f], v), wtot64);
        __syncthreads();   // wtot64 is written again in the next round
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = threadIdx.x * 4 + i;
            const long long pp = (long long)t0 + x;
            const long long val = (long long)(before + v[i]) + (f == 0 ? pp * liA[i] : -pp * riA[i]);
            if (x < n_here && val != 0) P64(R, f == 0 ? UVC_P_a_LI : UVC_P_a_RI, xb + x) = val;
        }
    }
}

// SPLIT: a region with fewer windows than the chip has wave slots (a deep, short panel region: 200 kb are three waves per SIMD, each walking
// thousands of reads) gives every window to a BLOCK: its four waves take every fourth chunk of the window's reads.  The kernel ends in
// atomics anyway, so the partial sums need no reduction.
// emit (misq=p1): every mismatching base also becomes an item of RegionDev::mis, and the M runs of the InDel reads are visited for that alone.
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_prep_fast(RegionDev R, UvcParams P, int emit) {
    __shared__ int2 prepq[4][PREPQ_CAP];
    const int lane = threadIdx.x & 63;
    const int wave = SPLIT ? wave_uniform((int)xcd_block()) : wave_uniform((int)((xcd_block() * blockDim.x + threadIdx.x) >> 6));
    const int64_t x0 = (int64_t)wave * 64;
    if (x0 >= R.npos) return;
    const int w0 = R.beg + (int)x0;
    const int p = w0 + lane;
    const int64_t x = x0 + lane;
    const bool valid = x < R.npos;
    const int my_ref = valid ? R.refsym[x] : 0;
    const int my_baq = valid ? (int)R.baq[x] : 0;
    int ldist = 0, rdist = 0, hbq = 0;
    long long lbaq = 0, rbaq = 0;
    COARSE_T(ct1)
    const __amdgpu_buffer_rsrc_t rs = bq_rsrc(R);
    // Mismatching bases are rare per lane but present in a large share of the iterations of a wave, and their handling (SNV / DNV
    // run detection, fragment mutation events) is a chain of dependent loads.  They are queued per wave and handled 64 at a time,
    // one per lane, in wave-uniform control flow, so the main loop never waits on them.
    int2 *myq = prepq[threadIdx.x >> 6];
    int nq = 0;   // wave-uniform: only updated in uniform control flow
    auto drain = [&]() {
        int gbase = 0;
        if (emit && lane == 0) gbase = atomicAdd(R.mis_cnt, nq);   // one atomic for the batch, then contiguous stores
        gbase = wave_uniform(gbase);
        for (int i = lane; i < nq; i += 64) {
            const int2 e = myq[i];
            if (emit) mis_emit(R, P, e, w0, gbase + i);
            if (e.x & PREPQ_MRUN) continue;
            const AlnRec &a = R.alns[e.x];
            const int ep = prepq_pos(e, w0);
            snv_dnv_scatter(R, R.bases + a.seq_off, (int)(a.qbase + ep - a.seq_off), a.l_qseq, a.pos, a.rend, ep);
            mut_event(R, P, a, ep, R.refsym[ep - R.beg]);
        }
        nq = 0;
    };
    // the four class sub-lists of the work list, one after the other through the same loop body (every counter here is a sum over the covering
    // reads: their order does not matter)
#pragma unroll 1
    for (int cls = 0; cls < 4; cls++) {
    const int lo = wave_uniform(win_lo(R, 1 + cls, (int)(x0 >> 6))), hi = wave_uniform(win_hi(R, 1 + cls, (int)(x0 >> 6)));
    for (int k0 = lo + (SPLIT ? 64 * (int)(threadIdx.x >> 6) : 0); k0 < hi; k0 += (SPLIT ? 256 : 64)) {
        int c[16];
        load_words(R.frec2 + (k0 + lane), k0 + lane < hi, c);
        const int n = imin(64, hi - k0);
        // the base | quality bytes of the chunk's reads are requested four reads ahead (one load per read and lane, HBM / L2 latency each:
        // with one read of look-ahead the wave waited for most of them)
        auto fetch = [&](int j) { return bq_load(rs, bcast(c[FR_W(qb_lo)], j) + p); };   // low word of qbase + p: exact for lanes inside the read, harmless elsewhere
        auto one = [&](int j, int bqn) {
            const int b = bq_sym(bqn), q = bq_qual(bqn);
            const int apos = bcast(c[FR_W(pos)], j), rend = bcast(c[FR_W(rend)], j);
            const bool mrun = (bcast(c[FR_W(xbv)], j) & FREC_M_RUN) != 0;   // an M run of an InDel read: k_prep_slow has the read, only the items are made here
            if (rend <= w0 || (mrun && !emit)) return;   // behind the window
            const bool cover = (valid && p >= apos && p < rend);
            const wmask mm = BAL(cover && b != my_ref);
            if (mm) {
                if (nq > PREPQ_CAP - 64) drain();
                if (cover && b != my_ref) myq[nq + (int)__builtin_popcountll(mm & ((1ull << lane) - 1ull))] = prepq_entry(bcast(c[FR_W(aln)], j), mrun, p, w0, b, q);
                nq += (int)__builtin_popcountll(mm);
            }
            if (cover && !mrun) {   // (the counters that do not look at the base: k_prep_sums)
                if (q >= P.bias_thres_highBQ) {
                    ldist += p - apos + 1; rdist += rend - p;
                    lbaq += (my_baq - bcast(c[FR_W(baq_pos)], j) + 1);
                    rbaq += (bcast(c[FR_W(baq_last)], j) - my_baq + 1);
                    hbq += 1;
                }
                const int clips = bcast(c[FR_W(clips)], j);
                if (clips != 0) {
                    const int aln = bcast(c[FR_W(aln)], j);
                    const int lclip = frec_clip_len(R, clips & 0xFFFF, aln, false), rclip = frec_clip_len(R, (clips >> 16) & 0xFFFF, aln, true);
                    const int pcr_inc = (((bcast(c[FR_W(fmd)], j) >> 24) & UVC_DFLAG_AMPLICON) ? 1 : 0);
                    if (p == apos && lclip > 0) clip_event(R, P, apos, 0, lclip, pcr_inc);
                    if (p == rend - 1 && rclip > 0) clip_event(R, P, rend, 1, rclip, pcr_inc);   // any index > 0 gives rpos_delta = -1
                }
            }
        };
        int r0 = fetch(0), r1 = (1 < n ? fetch(1) : 0), r2 = (2 < n ? fetch(2) : 0), r3 = (3 < n ? fetch(3) : 0);
        for (int j = 0; j < n; j += 4) {
            { const int v = r0; if (j + 4 < n) r0 = fetch(j + 4); one(j, v); }
            if (j + 1 < n) { const int v = r1; if (j + 5 < n) r1 = fetch(j + 5); one(j + 1, v); }
            if (j + 2 < n) { const int v = r2; if (j + 6 < n) r2 = fetch(j + 6); one(j + 2, v); }
            if (j + 3 < n) { const int v = r3; if (j + 7 < n) r3 = fetch(j + 7); one(j + 3, v); }
        }
    }
    }
    if (nq > 0) drain();
    COARSE_T(ct2)
    if (!valid) return;
    // k_prep_slow runs concurrently on the side stream and adds to the same fields: atomics
    if (hbq) {
        atomicAdd(&P32(R, UVC_P_a_highBQ_dp, x), hbq);
        atomicAdd(&P32(R, UVC_P_a_l_dist_sum, x), ldist); atomicAdd(&P32(R, UVC_P_a_r_dist_sum, x), rdist);
        add64(&P64(R, UVC_P_a_l_BAQ_sum, x), lbaq); add64(&P64(R, UVC_P_a_r_BAQ_sum, x), rbaq);
    }
#ifdef UVC_FRAG_COARSE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    COARSE_T(ct3)
    if (lane == 0 && ((int)(x0 >> 6) % 2999) == 7) printf("coarse prep wave %d lists %llu epilogue %llu\n", (int)(x0 >> 6), ct2 - ct1, ct3 - ct2);
#endif
}

// ------------------------------------------------------------------------------------------------
// k_prep_scan: what k_prep_fast<false> computes, read by read instead of window by window.  The five counters behind the base quality
// (a_highBQ_dp, a_l_dist_sum, a_r_dist_sum, a_l_BAQ_sum, a_r_BAQ_sum) are sums over the covering simple reads whose base at the position
// has quality >= bias_thres_highBQ: the sum over ALL covering reads is an interval sum (k_prep_sums), and every low-quality base takes its
// read's term out again at its own position.  With A the number of covering reads and n the number of low-quality bases at p,
//   a_highBQ_dp  = A - n
//   a_l_dist_sum = (p + 1) (A - n) - (S apos - C apos)                mod 2^32, as the plane's wrapping adds
//   a_r_dist_sum = (S rend - C rend) - p (A - n)
//   a_l_BAQ_sum  = (A - n) d(p) + (S cL - C cL),  d(p) = baq(p) - baq(t0),  cL = baq(t0) - baq(apos) + 1      (t0: the tile's first position)
//   a_r_BAQ_sum  = (S cR - C cR) - (A - n) d(p),                            cR = baq(rend - 1) - baq(t0) + 1
// (S: interval sums over the covering reads, C: sums over the reads that are low at p).  d, cL and cR are wrapping 32-bit differences of
// the LOW words of the 64-bit BAQ prefix sums; k_prep_fast adds (int)(baq(p) - baq(apos) + 1) = d + cL per read, which holds as integers
// while neither side overflows 32 bits -- prep_scan_exact() bounds the differences from the parameters and leaves the rest to k_prep_fast.
// One block per tile of PSCAN_TILE positions takes the work-list entries that reach the tile; eight lanes per entry compare eight bases
// per lane and step with the reference and test eight qualities, as k_aln_bm does (bytes outside [max(apos, tile begin), min(rend, tile
// end)) are masked: every base is scanned by the one tile that owns its position).  S and C share five difference arrays in LDS: a read
// adds +v / -v at the ends of its piece of the tile and -v / +v at p and p + 1 of each of its low-quality bases.  After a block prefix
// sum every plane gets one coalesced global atomic per position (k_prep_slow adds to the same planes meanwhile).  Mismatching bases wait
// in an LDS queue and go through snv_dnv_scatter / mut_event a block at a time; the clip events fire in the tile that owns their position.
// emit (misq=p1): a drain also moves the queue to RegionDev::mis, behind one atomicAdd for the batch, and the scan visits the M runs of the
// InDel reads for their items alone (no sums, no SNV / DNV runs, no mutation or clip events: k_prep_slow has those reads).
// The scan waits on memory (a read's bases and qualities are two or three cache lines each, scattered over the columns): the next
// entry's record and all words of this one are requested before anything is used (tile sizes and variants: DESIGN.md section 6-r6).
// ------------------------------------------------------------------------------------------------
#ifndef PSCAN_TILE
#define PSCAN_TILE 1024
#endif
#define PSCAN_QCAP 512     // LDS queue of the bases that differ from the reference (prepq_entry)
#define PSCAN_ROUND 512    // entries between two looks at the queue
#define PSCAN_WORDS 3      // 8-byte words per lane and trip: 192 bases of an entry (at most 8: a word's flags are every eighth bit of a mask)
enum { PN_A = 0, PN_APOS, PN_REND, PN_N32 };
enum { PN_CL = 0, PN_CR, PN_N64 };
__global__ void __launch_bounds__(256) k_prep_scan(RegionDev R, UvcParams P, int emit) {
    static_assert(PSCAN_TILE % 256 == 0 && PSCAN_TILE % 64 == 0, "a thread owns PSCAN_TILE / 256 consecutive positions in the prefix sums");
    static_assert(PSCAN_WORDS <= 8, "a word's flags are every eighth bit of a mask");
    static_assert(PSCAN_TILE <= 65536, "prepq_entry holds the offset in the tile in 16 bits");
    constexpr int PER = PSCAN_TILE / 256;
    // difference arrays: +v / -v at the ends of a read's piece of the tile, -v / +v around each of its low-quality bases; afterwards the finished counters
    __shared__ unsigned d32[PN_N32][PSCAN_TILE + 1];
    __shared__ unsigned long long d64[PN_N64][PSCAN_TILE + 1];
    __shared__ int2 queue[PSCAN_QCAP];
    __shared__ int qn, qbase;
    __shared__ unsigned wtot[PN_N32][4];
    __shared__ unsigned long long wtot64[PN_N64][4];
    const unsigned long long K7F = 0x7F7F7F7F7F7F7F7FULL, K80 = 0x8080808080808080ULL, K01 = 0x0101010101010101ULL;
    const int tid = threadIdx.x, sub = tid & 7, grp = tid >> 3;
    const int tile = xcd_block();   // neighbouring tiles scan the reads across their boundary: one L2 for both
    const int t0 = R.beg + tile * PSCAN_TILE, t1 = imin(t0 + PSCAN_TILE, R.beg + (int)R.npos);
    const int w_first = tile * (PSCAN_TILE / 64), w_last = imin(w_first + PSCAN_TILE / 64, R.nwin) - 1;
    int lo[4], cum[5];
    cum[0] = 0;
#pragma unroll
    for (int cls = 0; cls < 4; cls++) { lo[cls] = win_lo(R, 1 + cls, w_first); cum[cls + 1] = cum[cls] + imax(win_hi(R, 1 + cls, w_last) - lo[cls], 0); }
    const int total = cum[4];
    if (total == 0) return;   // (the whole block: nothing reaches the tile)
    for (int i = tid; i < PN_N32 * (PSCAN_TILE + 1); i += 256) (&d32[0][0])[i] = 0u;
    for (int i = tid; i < PN_N64 * (PSCAN_TILE + 1); i += 256) (&d64[0][0])[i] = 0ull;
    if (tid == 0) qn = 0;
    __syncthreads();
    const unsigned B0 = (unsigned)R.baq[t0 - R.beg];
    // quality < thr on eight bytes at once: bit 7 of (q & 0x7F) + add says (q & 0x7F) >= thr (thr <= 128) resp. >= thr - 128
    const int thr = P.bias_thres_highBQ;
    const bool thr_hi = (thr > 128);
    const unsigned long long qadd = K01 * (unsigned)(thr_hi ? imax(0x100 - thr, 0) : 0x80 - imax(thr, 0));
    auto mismatch = [&](int aln, int p) {
        const AlnRec &a = R.alns[aln];
        snv_dnv_scatter(R, R.bases + a.seq_off, (int)(a.qbase + p - a.seq_off), a.l_qseq, a.pos, a.rend, p);
        mut_event(R, P, a, p, R.refsym[p - R.beg]);
    };
    for (int base = 0; base < total; base += PSCAN_ROUND) {
        const int stop = imin(base + PSCAN_ROUND, total);
        // the record of the group's next entry is requested before this one's bases are: the group does not wait for the two in turn
        int4 n0 = make_int4(0, 0, 0, 0), n2 = n0, n3 = n0;
        const int4 *nq4 = nullptr;
        auto fetch = [&](int i) {
            const int cls = (i >= cum[1]) + (i >= cum[2]) + (i >= cum[3]);
            nq4 = (const int4 *)(R.frec2 + ((cls == 0 ? lo[0] : cls == 1 ? lo[1] - cum[1] : cls == 2 ? lo[2] - cum[2] : lo[3] - cum[3]) + i));
            n0 = nq4[0]; n2 = nq4[2]; n3 = nq4[3];
        };
        if (base + grp < stop) fetch(base + grp);
        for (int i = base + grp; i < stop; i += 32) {
            const int4 h0 = n0, h2 = n2, h3 = n3;   // pos rend qb_lo aln | bmv xbv bm4c clips | baq_pos baq_last baq2_last ext
            const int4 *q4 = nq4;
            if (i + 32 < stop) fetch(i + 32);
            const int apos = h0.x, rend = h0.y;
            if (rend <= t0 || apos >= t1 || apos >= rend) continue;   // (the eight lanes of the entry leave together)
            const bool mrun = (h2.y & FREC_M_RUN) != 0;   // an M run of an InDel read (k_prep_slow has the read): its items only
            if (mrun && !emit) continue;
            const int s = imax(apos, t0), e = imin(rend, t1);
            const int cL = (int)(B0 - (unsigned)h3.x + 1u), cR = (int)((unsigned)h3.y - B0 + 1u);
            // up to PSCAN_WORDS words per lane are requested together, ahead of the LDS atomics
            const bool whole = (e - s >= 8);
            for (int pb = s + 8 * sub; pb < e; pb += 64 * PSCAN_WORDS) {
                unsigned long long bb[PSCAN_WORDS], qq[PSCAN_WORDS], rr[PSCAN_WORDS];
#pragma unroll
                for (int w = 0; w < PSCAN_WORDS; w++) {
                    const int p0 = pb + 64 * w, nb = imin(8, e - p0);
                    bb[w] = 0; qq[w] = 0; rr[w] = 0;
                    if (nb <= 0) continue;
                    const uint8_t *bp = R.bases + (uint32_t)(h0.z + p0), *qp = R.quals + (uint32_t)(h0.z + p0), *rp = R.refsym + (p0 - R.beg);
                    if (whole) {   // the last e - p0 < 8 bytes come from the word that ends with them: nothing is loaded past the read or the tile
                        const int back = 8 - nb;
                        bb[w] = load8u(bp - back) >> (8 * back); qq[w] = load8u(qp - back) >> (8 * back); rr[w] = load8u(rp - back) >> (8 * back);
                    } else {
                        for (int j = 0; j < nb; j++) { bb[w] |= (unsigned long long)bp[j] << (8 * j); qq[w] |= (unsigned long long)qp[j] << (8 * j); rr[w] |= (unsigned long long)rp[j] << (8 * j); }
                    }
                }
                // bit 8 j + w: byte j of word w, i.e. position pb + 64 w + j, differs from the reference / has a low quality
                unsigned long long mism = 0, low = 0;
#pragma unroll
                for (int w = 0; w < PSCAN_WORDS; w++) {
                    const int nb = imin(8, e - (pb + 64 * w));
                    if (nb <= 0) continue;
                    const unsigned long long vm = K80 >> (8 * (8 - nb));   // bit 7 of the nb bytes that count
                    const unsigned long long x = bb[w] ^ rr[w], t = (qq[w] & K7F) + qadd;
                    mism |= (((((x & K7F) + K7F) | x) & vm) >> 7) << w;
                    low |= (((thr_hi ? ~(qq[w] & t) : ~(qq[w] | t)) & vm) >> 7) << w;
                }
                if (mrun) low = 0;
                while (low) {   // the read's terms leave the sums at this one position: -v at p, +v at p + 1
                    const int bit = __builtin_ctzll(low), xp = pb + 64 * (bit & 7) + (bit >> 3) - t0;
                    low &= low - 1;
                    atomicAdd(&d32[PN_A][xp], 0u - 1u); atomicAdd(&d32[PN_A][xp + 1], 1u);
                    atomicAdd(&d32[PN_APOS][xp], 0u - (unsigned)apos); atomicAdd(&d32[PN_APOS][xp + 1], (unsigned)apos);
                    atomicAdd(&d32[PN_REND][xp], 0u - (unsigned)rend); atomicAdd(&d32[PN_REND][xp + 1], (unsigned)rend);
                    atomicAdd(&d64[PN_CL][xp], 0ull - (unsigned long long)(long long)cL); atomicAdd(&d64[PN_CL][xp + 1], (unsigned long long)(long long)cL);
                    atomicAdd(&d64[PN_CR][xp], 0ull - (unsigned long long)(long long)cR); atomicAdd(&d64[PN_CR][xp + 1], (unsigned long long)(long long)cR);
                }
                while (mism) {
                    const int bit = __builtin_ctzll(mism), p = pb + 64 * (bit & 7) + (bit >> 3);
                    mism &= mism - 1;
                    unsigned long long bw = 0, qw = 0;   // the word of the bit (selects: bb and qq stay in registers)
#pragma unroll
                    for (int w = 0; w < PSCAN_WORDS; w++) if ((bit & 7) == w) { bw = bb[w]; qw = qq[w]; }
                    const int sym = (int)((bw >> (8 * (bit >> 3))) & 0xFF), q = (int)((qw >> (8 * (bit >> 3))) & 0xFF);
                    const int2 it = prepq_entry(h0.w, mrun, p, t0, sym, q);
                    const int slot = atomicAdd(&qn, 1);
                    if (slot < PSCAN_QCAP) queue[slot] = it;
                    else {   // (a full queue: at once, by this lane, and one slot of the global queue)
                        if (emit) mis_emit(R, P, it, t0, atomicAdd(R.mis_cnt, 1));
                        if (!mrun) mismatch(h0.w, p);
                    }
                }
            }
            if (mrun) continue;   // (the eight lanes of the entry)
            // the interval sums, a lane per sum; the clip events
            if (sub < PN_N32) {
                const unsigned v = (sub == PN_A ? 1u : sub == PN_APOS ? (unsigned)apos : (unsigned)rend);
                diff_put_at(d32[sub], s - t0, e - t0, v);   // (s < e are the read's ends clipped to the tile)
            } else if (sub < PN_N32 + PN_N64) {
                const unsigned long long v = (unsigned long long)(long long)(sub == PN_N32 + PN_CL ? cL : cR);
                diff_put_at(d64[sub - PN_N32], s - t0, e - t0, v);
            } else if (sub == 7 && h2.w != 0) {
                const int lclip = frec_clip_len(R, h2.w & 0xFFFF, h0.w, false), rclip = frec_clip_len(R, (h2.w >> 16) & 0xFFFF, h0.w, true);
                const int pcr_inc = (((q4[1].x >> 24) & 0x4) ? 1 : 0);
                if (lclip > 0 && apos >= t0) clip_event(R, P, apos, 0, lclip, pcr_inc);
                if (rclip > 0 && rend <= t1) clip_event(R, P, rend, 1, rclip, pcr_inc);   // any index > 0 gives rpos_delta = -1
            }
        }
        __syncthreads();
        const int n_queued = imin(qn, PSCAN_QCAP);
        const bool drain = (n_queued >= 256 || stop == total);   // a base per thread, or the last look
        if (drain && emit && n_queued) {   // (block-uniform) the batch's place in the global queue: one atomic
            if (tid == 0) qbase = atomicAdd(R.mis_cnt, n_queued);
            __syncthreads();
        }
        if (drain) for (int i = tid; i < n_queued; i += 256) {
            const int2 e = queue[i];
            if (emit) mis_emit(R, P, e, t0, qbase + i);
            if (!(e.x & PREPQ_MRUN)) mismatch(e.x, prepq_pos(e, t0));
        }
        __syncthreads();
        if (drain && tid == 0) qn = 0;
        __syncthreads();
    }
    // prefix sums of the five difference arrays at once: PER consecutive positions per thread, the wave's, the block's
    unsigned v32[PN_N32][PER], inc32[PN_N32];
    unsigned long long v64[PN_N64][PER], inc64[PN_N64];
#pragma unroll
    for (int f = 0; f < PN_N32; f++) inc32[f] = block_scan_begin(diff_run<PER>(d32[f], v32[f]), wtot[f]);
#pragma unroll
    for (int f = 0; f < PN_N64; f++) inc64[f] = block_scan_begin(diff_run<PER>(d64[f], v64[f]), wtot64[f]);
    __syncthreads();   // the one barrier of the five scans
#pragma unroll
    for (int f = 0; f < PN_N32; f++) inc32[f] = block_scan_end<4>(inc32[f], wtot[f]);
#pragma unroll
    for (int f = 0; f < PN_N64; f++) inc64[f] = block_scan_end<4>(inc64[f], wtot64[f]);
    const int n_here = t1 - t0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int x = tid * PER + i;
        if (x >= n_here) continue;
        const unsigned p = (unsigned)(t0 + x);
        const unsigned hb = inc32[PN_A] + v32[PN_A][i];
        const unsigned s_apos = inc32[PN_APOS] + v32[PN_APOS][i], s_rend = inc32[PN_REND] + v32[PN_REND][i];
        const long long s_cl = (long long)(inc64[PN_CL] + v64[PN_CL][i]), s_cr = (long long)(inc64[PN_CR] + v64[PN_CR][i]);
        const long long hd = (long long)hb * (long long)(int)((unsigned)R.baq[p - (unsigned)R.beg] - B0);
        d32[PN_A][x] = hb; d32[PN_APOS][x] = (p + 1u) * hb - s_apos; d32[PN_REND][x] = s_rend - p * hb;
        d64[PN_CL][x] = (unsigned long long)(hd + s_cl); d64[PN_CR][x] = (unsigned long long)(s_cr - hd);
    }
    __syncthreads();
    // (the finished counters went back into LDS so that a wave's atomics cover 64 consecutive positions of a plane)
    const int64_t xb = (int64_t)tile * PSCAN_TILE;
    for (int x = tid; x < n_here; x += 256) {
        const int hb = (int)d32[PN_A][x];
        if (!hb) continue;   // no high-quality base of a simple read here: every sum is empty
        atomicAdd(&P32(R, UVC_P_a_highBQ_dp, xb + x), hb);
        atomicAdd(&P32(R, UVC_P_a_l_dist_sum, xb + x), (int)d32[PN_APOS][x]); atomicAdd(&P32(R, UVC_P_a_r_dist_sum, xb + x), (int)d32[PN_REND][x]);
        add64(&P64(R, UVC_P_a_l_BAQ_sum, xb + x), (long long)d64[PN_CL][x]); add64(&P64(R, UVC_P_a_r_BAQ_sum, xb + x), (long long)d64[PN_CR][x]);
    }
}

// P1 for one alignment whose CIGAR has InDels / unusual clip layouts: one wave per read, lanes stride over the bases of
// each CIGAR op (every update of P1 is an independent integer add once the per-read totals of the first loop are known)
__global__ void __launch_bounds__(64) k_prep_slow(RegionDev R, UvcParams P) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= R.n_complex) return;
    const AlnRec &a = R.alns[R.complex_ids[t]];
    const uint32_t *cigar = R.cigars + a.cigar_off;
    const uint8_t *bases = R.bases + a.seq_off, *quals = R.quals + a.seq_off;
    const int off = R.beg, rend = a.rend, apos = a.pos, n_cigar = a.n_cigar;
    const long long baq_last = R.end - 1;
    int nge = 0, ngo = 0, insbaq_sum = 0, delbaq_sum = 0, inslen_sum = 0, dellen_sum = 0;
    int qpos = 0, rpos = apos;
    for (int i = 0; i < n_cigar; i++) {
        const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
        if (C_INS == op) { nge += len; ngo++; insbaq_sum += (int)(BAQ1(R, lmin((long long)rpos + len, baq_last)) - BAQ1(R, rpos)); inslen_sum += len; qpos += len; }
        else if (C_DEL == op) { nge += len; ngo++; delbaq_sum += (int)(BAQ1(R, lmin((long long)rpos + len, baq_last)) - BAQ1(R, rpos)); dellen_sum += len; rpos += len; }
        else if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) { qpos += len; rpos += len; }
        else if (op == C_REF_SKIP) rpos += len;
        else if (op == C_SOFT_CLIP) qpos += len;
    }
    const int qlen = rend - apos;
    const int xm1500 = a.xm1500, go1500 = a.go1500;
    const int avg_gaplen = nge / imax(1, ngo);
    const int frag_pos_L = imin(apos, a.mpos), frag_pos_R = frag_pos_L + abs(a.isize);
    const bool isrc = (a.flag & 0x10) != 0;
    const int pcr_dp_inc = ((a.dflag & UVC_DFLAG_AMPLICON) ? 1 : 0), umi_dp_inc = ((a.dflag & UVC_DFLAG_UMI) ? 1 : 0);
    const int atd = P.indel_adj_tracklen_dist;
    const int nrtr = (int)R.npos;
    const int isize = a.isize, l_qseq = a.l_qseq;
    const long long baq_apos = BAQ1(R, apos), baq_rlast = BAQ1(R, rend - 1);
    qpos = 0; rpos = apos;
    for (int i = 0; i < n_cigar; i++) {
        const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
        if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) {
            for (int j = lane; j < len; j += 64) {
                const int rp = rpos + j, qp = qpos + j;
                const int64_t x = rp - off;
                if (pcr_dp_inc) atomicAdd(&P32(R, UVC_P_a_pcr_dp, x), pcr_dp_inc);
                if (umi_dp_inc) atomicAdd(&P32(R, UVC_P_a_umi_dp, x), umi_dp_inc);
                atomicAdd(&P32(R, UVC_P_a_dp, x), 1);
                atomicAdd(&P32(R, UVC_P_a_qlen, x), qlen);
                atomicAdd(&P32(R, UVC_P_a_XM1500, x), xm1500);
                atomicAdd(&P32(R, UVC_P_a_GO1500, x), go1500);
                atomicAdd(&P32(R, UVC_P_a_GAPLEN, x), avg_gaplen);
                if (isize != 0) {
                    if (isrc) { add64(&P64(R, UVC_P_a_LI, x), imin(rp - frag_pos_L + 1, MAX_INSERT_SIZE)); atomicAdd(&P32(R, UVC_P_a_LIDP, x), 1); }
                    else      { add64(&P64(R, UVC_P_a_RI, x), imin(frag_pos_R - rp, MAX_INSERT_SIZE));     atomicAdd(&P32(R, UVC_P_a_RIDP, x), 1); }
                }
                snv_dnv_scatter(R, bases, qp, l_qseq, apos, rend, rp);
                if (quals[qp] >= P.bias_thres_highBQ) {
                    atomicAdd(&P32(R, UVC_P_a_l_dist_sum, x), rp - apos + 1);
                    atomicAdd(&P32(R, UVC_P_a_r_dist_sum, x), rend - rp);
                    atomicAdd(&P32(R, UVC_P_a_inslen_sum, x), inslen_sum);
                    atomicAdd(&P32(R, UVC_P_a_dellen_sum, x), dellen_sum);
                    add64(&P64(R, UVC_P_a_l_BAQ_sum, x), (int)(BAQ1(R, rp) - baq_apos + 1));
                    add64(&P64(R, UVC_P_a_r_BAQ_sum, x), (int)(baq_rlast - BAQ1(R, rp) + 1));
                    add64(&P64(R, UVC_P_a_insBAQ_sum, x), insbaq_sum);
                    add64(&P64(R, UVC_P_a_delBAQ_sum, x), delbaq_sum);
                    atomicAdd(&P32(R, UVC_P_a_highBQ_dp, x), 1);
                }
            }
            qpos += len; rpos += len;
        } else if (op == C_INS || op == C_DEL) {
            const int i1 = imax(atd, rpos - off) - atd, i2 = imin(rpos - off + atd, nrtr - 1);
            const int t1 = RTRP(R, UVC_RTR_tracklen, i1), t2 = RTRP(R, UVC_RTR_tracklen, i2);
            const int unitlen2 = imax(1, (t1 > t2) ? RTRP(R, UVC_RTR_unitlen, i1) : RTRP(R, UVC_RTR_unitlen, i2));
            const int rtr_lo = imax((off + RTRP(R, UVC_RTR_begpos, i1)) - atd, apos);
            const int rtr_hi = imin((off + RTRP(R, UVC_RTR_begpos, i2) + t2) + atd, rend);
            const int inv100 = (int)(100u / ((0 == (unsigned)len % (unsigned)unitlen2) ? ((unsigned)len / (unsigned)unitlen2) : 4u));
            if (op == C_INS) {
                const int nbases = (int)((unsigned)len * (unsigned)P.indel_adj_indellen_perc / 100u);
                for (int r2 = imax(rpos - nbases, apos) + lane; r2 < imin(rpos + nbases, rend); r2 += 64) {
                    const int64_t x = r2 - off;
                    atomicAdd(&P32(R, UVC_P_a_near_ins_dp, x), 1);
                    add64(&P64(R, UVC_P_a_near_ins_pow2len, x), (long long)((unsigned)len * (unsigned)len));
                    add64(&P64(R, UVC_P_a_near_ins_l_pow2len, x), (long long)(r2 + 1 - (rpos - nbases)) * (r2 + 1 - (rpos - nbases)));
                    add64(&P64(R, UVC_P_a_near_ins_r_pow2len, x), (long long)((rpos + nbases) - r2) * ((rpos + nbases) - r2));
                    atomicAdd(&P32(R, UVC_P_a_near_ins_inv100len, x), inv100);
                }
                for (int r2 = rtr_lo + lane; r2 < rtr_hi; r2 += 64) atomicAdd(&P32(R, UVC_P_a_near_RTR_ins_dp, r2 - off), 1);
                if (lane == 0) atomicAdd(&P32(R, UVC_P_a_at_ins_dp, rpos - off), 1);
                qpos += len;
            } else {
                for (int r2 = rpos + lane; r2 < rpos + len; r2 += 64) {
                    const int64_t x = r2 - off;
                    if (pcr_dp_inc) atomicAdd(&P32(R, UVC_P_a_pcr_dp, x), pcr_dp_inc);
                    if (umi_dp_inc) atomicAdd(&P32(R, UVC_P_a_umi_dp, x), umi_dp_inc);
                    atomicAdd(&P32(R, UVC_P_a_dp, x), 1);
                    atomicAdd(&P32(R, UVC_P_a_qlen, x), qlen);
                    atomicAdd(&P32(R, UVC_P_a_highBQ_dp, x), 1);
                    atomicAdd(&P32(R, UVC_P_a_XM1500, x), xm1500);
                    atomicAdd(&P32(R, UVC_P_a_GO1500, x), go1500);
                    atomicAdd(&P32(R, UVC_P_a_GAPLEN, x), avg_gaplen);
                    if (isize != 0) {   // sic: the deletion start rpos, not r2 (main.hpp:1137-1145)
                        if (isrc) { add64(&P64(R, UVC_P_a_LI, x), imin(rpos - frag_pos_L + 1, MAX_INSERT_SIZE)); atomicAdd(&P32(R, UVC_P_a_LIDP, x), 1); }
                        else      { add64(&P64(R, UVC_P_a_RI, x), imin(frag_pos_R - rpos, MAX_INSERT_SIZE));     atomicAdd(&P32(R, UVC_P_a_RIDP, x), 1); }
                    }
                    atomicAdd(&P32(R, UVC_P_a_l_dist_sum, x), rpos - apos + 1);
                    atomicAdd(&P32(R, UVC_P_a_r_dist_sum, x), rend - rpos);
                    atomicAdd(&P32(R, UVC_P_a_inslen_sum, x), inslen_sum);
                    atomicAdd(&P32(R, UVC_P_a_dellen_sum, x), dellen_sum);
                    add64(&P64(R, UVC_P_a_l_BAQ_sum, rpos - off), (int)(BAQ1(R, rpos) - baq_apos + 1));   // sic: at rpos (main.hpp:1156-1157)
                    add64(&P64(R, UVC_P_a_r_BAQ_sum, rpos - off), (int)(baq_rlast - BAQ1(R, rpos) + 1));
                    add64(&P64(R, UVC_P_a_insBAQ_sum, x), insbaq_sum);
                    add64(&P64(R, UVC_P_a_delBAQ_sum, x), delbaq_sum);
                }
                const int nbases_l = (int)((unsigned)len * (unsigned)(P.indel_adj_indellen_perc - 100) / 100u);
                const int nbases_r = (int)((unsigned)len * (unsigned)P.indel_adj_indellen_perc / 100u);
                const int lpos = imax(rpos - nbases_l, apos), rpos_r = imin(rpos + nbases_r, rend) - 1;
                for (int r2 = lpos + lane; r2 <= rpos_r; r2 += 64) {
                    const int64_t x = r2 - off;
                    atomicAdd(&P32(R, UVC_P_a_near_del_dp, x), 1);
                    add64(&P64(R, UVC_P_a_near_del_pow2len, x), (long long)((unsigned)len * (unsigned)len));
                    add64(&P64(R, UVC_P_a_near_del_l_pow2len, x), (long long)(r2 - lpos + 1) * (r2 - lpos + 1));
                    add64(&P64(R, UVC_P_a_near_del_r_pow2len, x), (long long)(rpos_r - r2 + 1) * (rpos_r - r2 + 1));
                    atomicAdd(&P32(R, UVC_P_a_near_del_inv100len, x), inv100);
                }
                for (int r2 = rtr_lo + lane; r2 < rtr_hi; r2 += 64) atomicAdd(&P32(R, UVC_P_a_near_RTR_del_dp, r2 - off), 1);
                if (lane == 0) atomicAdd(&P32(R, UVC_P_a_at_del_dp, rpos - off), 1);
                rpos += len;
            }
        } else {
            if ((C_SOFT_CLIP == op || C_HARD_CLIP == op) && lane == 0) clip_event(R, P, rpos, i, len, pcr_dp_inc);
            if (op == C_REF_SKIP) rpos += len; else if (op == C_SOFT_CLIP) qpos += len;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// P1b (update_seg_format_thres_from_prep_sets, main.hpp:1206-1299)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_thres(RegionDev R, UvcParams P, int half_ratio_phred) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= R.npos) return;
    const bool is_normal = P.tumor_vcf_is_provided;
    const int segLIDP = imax(P32(R, UVC_P_a_LIDP, x), 1), segRIDP = imax(P32(R, UVC_P_a_RIDP, x), 1);
    const int ins_dp = P32(R, UVC_P_a_near_ins_dp, x), del_dp = P32(R, UVC_P_a_near_del_dp, x);
    const double ins_l = ceil(sqrt((double)(P64(R, UVC_P_a_near_ins_l_pow2len, x) / imax(ins_dp, 1))));
    const double del_l = ceil(sqrt((double)(P64(R, UVC_P_a_near_del_l_pow2len, x) / imax(del_dp, 1))));
    const double ins_r = ceil(sqrt((double)(P64(R, UVC_P_a_near_ins_r_pow2len, x) / imax(ins_dp, 1))));
    const double del_r = ceil(sqrt((double)(P64(R, UVC_P_a_near_del_r_pow2len, x) / imax(del_dp, 1))));
    const int dnv_border = ((UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform && (P32(R, UVC_P_a_dnv_dp, x) * 2 > P32(R, UVC_P_a_snv_dp, x))) ? 10 : 0);
    TH(R, UVC_T_aLPxT, x) = (int)(fmax(ins_l, fmax(del_l, (double)dnv_border)) + P.bias_thres_aLPxT_add);
    TH(R, UVC_T_aRPxT, x) = (int)(fmax(ins_r, fmax(del_r, (double)dnv_border)) + P.bias_thres_aLPxT_add);
    int ip = RTRP(R, UVC_RTR_indelphred, x);
    if (ins_dp * P.indel_del_to_ins_err_ratio < del_dp) ip += half_ratio_phred;
    if (del_dp * P.indel_del_to_ins_err_ratio < ins_dp) ip -= half_ratio_phred;
    const int pc_inc1 = (int)(3 * 100 * imax(1, ins_dp + del_dp) / (imax(1, P32(R, UVC_P_a_near_ins_inv100len, x) + P32(R, UVC_P_a_near_del_inv100len, x)))) - 3;
    ip += ibetween(pc_inc1, 0, 6);
    RTRP(R, UVC_RTR_indelphred, x) = imax(ip, 0);
    const int p1T = (is_normal ? P.bias_thres_aLRI1NT_perc : P.bias_thres_aLRI1T_perc), p1t = (is_normal ? P.bias_thres_aLRI1Nt_perc : P.bias_thres_aLRI1t_perc);
    const long long LI = P64(R, UVC_P_a_LI, x), RI = P64(R, UVC_P_a_RI, x);
    TH(R, UVC_T_aLI1T, x) = (int)(LI * p1T / (segLIDP * 100) + P.bias_thres_aLRI1T_add);
    TH(R, UVC_T_aLI2T, x) = (int)(LI * P.bias_thres_aLRI2T_perc / (segLIDP * 100) + P.bias_thres_aLRI2T_add);
    TH(R, UVC_T_aLI1t, x) = (int)(LI * p1t / (segLIDP * 100));
    TH(R, UVC_T_aLI2t, x) = (int)(LI * P.bias_thres_aLRI2t_perc / (segLIDP * 100));
    TH(R, UVC_T_aRI1T, x) = (int)(RI * p1T / (segRIDP * 100) + P.bias_thres_aLRI1T_add);
    TH(R, UVC_T_aRI2T, x) = (int)(RI * P.bias_thres_aLRI2T_perc / (segRIDP * 100) + P.bias_thres_aLRI2T_add);
    TH(R, UVC_T_aRI1t, x) = (int)(RI * p1t / (segRIDP * 100));
    TH(R, UVC_T_aRI2t, x) = (int)(RI * P.bias_thres_aLRI2t_perc / (segRIDP * 100));
    const int pP1 = (is_normal ? P.bias_thres_aLRP1Nt_avgmul_perc : P.bias_thres_aLRP1t_avgmul_perc), pP2 = P.bias_thres_aLRP2t_avgmul_perc;
    const int pB1 = (is_normal ? P.bias_thres_aLRB1Nt_avgmul_perc : P.bias_thres_aLRB1t_avgmul_perc), pB2 = P.bias_thres_aLRB2t_avgmul_perc;
    const int hb = P32(R, UVC_P_a_highBQ_dp, x);
    const long long den = imax(1, hb * 100);
    const long long lds = P32(R, UVC_P_a_l_dist_sum, x), rds = P32(R, UVC_P_a_r_dist_sum, x);
    TH(R, UVC_T_aLP1t, x) = (int)nnminus(lds * pP1 / den, P.bias_thres_aLRP1t_minus);
    TH(R, UVC_T_aLP2t, x) = (int)nnminus(lds * pP2 / den, P.bias_thres_aLRP2t_minus);
    TH(R, UVC_T_aRP1t, x) = (int)nnminus(rds * pP1 / den, P.bias_thres_aLRP1t_minus);
    TH(R, UVC_T_aRP2t, x) = (int)nnminus(rds * pP2 / den, P.bias_thres_aLRP2t_minus);
    const long long pdel = P64(R, UVC_P_a_delBAQ_sum, x) / imax(1, hb);
    const long long lb = P64(R, UVC_P_a_l_BAQ_sum, x), rb = P64(R, UVC_P_a_r_BAQ_sum, x);
    TH(R, UVC_T_aLB1t, x) = (int)nnminus(lb * pB1 / den, P.bias_thres_aLRB1t_minus + pdel);
    TH(R, UVC_T_aLB2t, x) = (int)nnminus(lb * pB2 / den, P.bias_thres_aLRB2t_minus);
    TH(R, UVC_T_aRB1t, x) = (int)nnminus(rb * pB1 / den, P.bias_thres_aLRB1t_minus + pdel);
    TH(R, UVC_T_aRB2t, x) = (int)nnminus(rb * pB2 / den, P.bias_thres_aLRB2t_minus);
}

// ------------------------------------------------------------------------------------------------
// contribution of a SIMPLE alignment at reference position p (BASE_QUALITY_MAX values, no bias)
// main.hpp:1918-1924 (LINK_M), 1949-1980 (base)
// ------------------------------------------------------------------------------------------------
DEV int simple_link_value(const RegionDev &R, const UvcParams &P, const AlnRec &a, int p, const uint8_t *quals_qbase, bool proton) {
    const int64_t x = p - R.beg;
    const int noindel = imin(RTRP(R, UVC_RTR_indelphred, x - 1), RTRP(R, UVC_RTR_indelphred, x));
    const int qfromBQ2 = (proton ? imin((int)quals_qbase[p - 1], (int)quals_qbase[p]) : 80);
    return (int)nnminus(imin(qfromBQ2, noindel), a.nogap_penal) + 1;
}
DEV int simple_base_value(const UvcParams &P, const AlnRec &a, int p, const uint8_t *quals_qbase, bool proton) {
    const int q = quals_qbase[p];
    if (proton) {
        const int i2 = p - a.pos, len = a.rend - a.pos;
        if ((0 == i2) || (len - 1 == i2)) {
            // packed neighbouring cigar words never equal the bare op codes (main.hpp:1953-1956), so both flags hold at the op ends
            const bool next_gap = (len - 1 == i2), prev_gap = (0 == i2);
            const bool isrc2 = (0 != i2);
            const int qpos = (int)(p - a.pos) + a.lclip_q;
            int prev_base_phred = 1;
            if (isrc2 && (qpos + 1 < a.l_qseq)) prev_base_phred = quals_qbase[p + 1];
            if ((!isrc2) && (qpos > 0)) prev_base_phred = quals_qbase[p - 1];
            int adj = 100;
            if (next_gap) adj = imin(adj, (a.rclip_oplen > 0 ? a.rclip_oplen : 100));
            if (prev_gap) adj = imin(adj, (a.lclip_oplen > 0 ? a.lclip_oplen : 100));
            if (adj < 3) return imin(q, prev_base_phred) + imin(P.bq_phred_added_misma, P.bq_phred_added_indel);
            return imin(q, prev_base_phred) + P.bq_phred_added_misma;
        }
    }
    return base_value(q, P);
}

// one queued mismatching base of a simple alignment: dealwith_segbias<false> into a scratch record, flushed with atomics
DEV void mis_apply(const RegionDev &R, const UvcParams &P, const MisItem &it) {
    const int64_t x = it.epos - R.beg;
    const int sym = it.symval & 0xFF, inc = it.symval >> 8;
    if ((unsigned)it.rank >= (unsigned)R.n_alns || x < 0 || x >= R.npos || sym > UVC_BASE_NN) { atomicExch(R.err, UVCGPU_EDEVICE); return; }   // corrupt queue entry
    const AlnRec &a = R.alns[it.rank];
    const SegRead sr = make_segread(R, a);
    PosThres T;
    load_thres(R, T, x);
    SegAcc A; A.zero();
    A.bq = inc;
    segbias<false>(A, P, sr, T, it.epos, R.baq[x], R.baq[R.npos + x], inc, a.bm1500[sym], C_MATCH, 0, 10000);
    seg_flush(R, A, sym, x);
}

#ifndef P2_AHEAD
#define P2_AHEAD 2
#endif
#define MISQ_CAP 192   // per-wave LDS queue of mismatching bases (flushed to the global queue when fewer than 64 slots are left)
// ------------------------------------------------------------------------------------------------
// P2 fast: updateByAln<SYMBOL_COUNT_SUM, bias> for simple alignments, one lane per position
// ------------------------------------------------------------------------------------------------
// Two instantiations, <true,false> for LINK_M and <false,true> for the read bases: each keeps one SegAcc in registers,
// which halves the accumulator footprint and doubles the waves per SIMD.
// SPLIT (see k_prep_fast): a block per window, its four waves take every fourth chunk of the window's entries; their counters are added up
// in LDS (red: one slot per counter and lane) and stored by the four waves together.
#define P2_RED_LINK5 (UVC_NSEG32 + 2 * UVC_NSEG64 + 5)   // base pass: the four aDP** rows and the BQSUM row of LINK_M, behind the rows of its own symbol
#define P2_RED_SLOTS (P2_RED_LINK5 + 5)
// the 64-bit counter f of the LDS reduction area: two int rows of 64 = one row of 64 unsigned long long
DEV unsigned long long *red64(int (*red)[64], int f) { return (unsigned long long *)&red[UVC_NSEG32 + 2 * f][0]; }
// NSL > 0 (with SPLIT, for the plain completion pass only): the sparse form, k_p2_link_sparse.  The block serves window `win` with 4 * NSL
// waves; wave w walks slice w >> 2 (uvc_link_slice) of class list w & 3, and the LDS reduction of the split form adds the 4 * NSL partial sets up.
// MQ: the base pass makes the mismatch queue itself (the generic forms, and the plain ones where the accumulate says misq=p2); without it P1
// has made the queue (misq=p1) and no ballot, no LDS queue and no flush are compiled.
template <bool DO_L, bool DO_B, bool PLAIN, bool SPLIT = false, int NSL = 0, bool MQ = DO_B>
DEV void p2_fast_body(const RegionDev &R, const UvcParams &P, int *amp1, int *amp2, MisItem (*misq)[MQ ? MISQ_CAP : 1], int (*red)[64] = nullptr, int win = 0) {
    static_assert(NSL == 0 || (SPLIT && DO_L && !DO_B && PLAIN), "the sparse form exists for the plain completion pass");
    static_assert(!MQ || DO_B, "the queue holds read bases");
    static_assert(MQ || !DO_B || PLAIN, "P1 makes the queue of the plain form only: the generic values need neighbouring qualities and the primer gate");
    constexpr int NWV = (NSL ? 4 * NSL : 4);   // waves of a block
    COARSE_T(ct0)
    if (DO_L && !NSL) {   // the completion pass runs a window only where a reader asked for it and no earlier pass has been (block-uniform; the waves look again below)
        if (SPLIT) { const int w = xcd_block(); if (!uvc_link_window_runs(R.link_need[w], R.link_done[w])) return; }
        else { const int b = xcd_block(); if (!(((const uint32_t *)R.link_need)[b] & ~((const uint32_t *)R.link_done)[b] & 0x01010101u)) return; }
    }
    if (!NSL) {   // (the sparse form's kernel fills the tables once for all its windows)
        for (int v = (int)threadIdx.x - AMP_LO; v < 256; v += 256) {   // (a threshold of 0 would divide by zero for a value below it, as the reference does: uvcgpu_params_check refuses a negative addend beside such a threshold, so that entry is never read)
            const int d1 = P.bias_thres_PFBQ1 * P.bias_thres_PFBQ1, d2 = P.bias_thres_PFBQ2 * P.bias_thres_PFBQ2;
            amp1[v + AMP_LO] = ((v < P.bias_thres_PFBQ1 && d1) ? 100 * (v * v) / d1 : 100);
            amp2[v + AMP_LO] = ((v < P.bias_thres_PFBQ2 && d2) ? 100 * (v * v) / d2 : 100);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = NSL ? wave_uniform(win) : SPLIT ? wave_uniform((int)xcd_block()) : wave_uniform((int)((xcd_block() * blockDim.x + threadIdx.x) >> 6));
    const int64_t x0 = (int64_t)wave * 64;
    if (x0 >= R.npos) return;   // (block-uniform in the split form)
    if (DO_L && !SPLIT && !uvc_link_window_runs(R.link_need[wave], R.link_done[wave])) return;
    if (SPLIT) { for (int i2 = threadIdx.x; i2 < P2_RED_SLOTS * 64; i2 += 64 * NWV) (&red[0][0])[i2] = 0; __syncthreads(); }
    const int w0 = R.beg + (int)x0;
    const int p = w0 + lane;
    const int64_t x = x0 + lane;
    const bool valid = x < R.npos;
    const bool proton = (PLAIN ? false : (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform));
    const bool normal_filter_primers = normal_filters_primers(P);
    const int my_ref = valid ? R.refsym[x] : 0;
    PosThres T;
    long long baq_p = 0, baq2_p = 0;
    if (valid) { load_thres(R, T, x); baq_p = R.baq[x]; baq2_p = R.baq[R.npos + x]; }
    else { for (int f = 0; f < UVC_NTHRES; f++) T.t[f] = 0; }
    SegAcc Aref, Alink;   // only the one selected by the template arguments stays live
    Aref.zero(); Alink.zero();
    // LINK_M value of a simple read at this position is a per-position constant up to the read's penalty (main.hpp:1919-1923)
    // The plain base pass carries the five cells of LINK_M that P3 reads; the generic forms (IonTorrent, amplicon, primer, short reads) keep the
    // parent's split of the work -- there the LINK pass makes all 39 cells, over every window, inside the accumulate (the host forces eager)
    constexpr bool L5_BASE = DO_B && PLAIN, L5_LINK = DO_L && !PLAIN;
    int noindel80 = 80;
    if ((DO_L || L5_BASE) && valid && x > 0) noindel80 = imin(80, imin(RTRP(R, UVC_RTR_indelphred, x - 1), RTRP(R, UVC_RTR_indelphred, x)));
    MisItem *myq = misq[MQ ? (threadIdx.x >> 6) : 0];
    int nq = 0;   // wave-uniform: only updated in uniform control flow
    int l5_bq = 0;   // base pass: BQSUM of LINK_M (see l5_dp)
    auto flush_queue = [&]() {
        int base = 0;
        if (lane == 0) base = atomicAdd(R.mis_cnt, nq);
        base = wave_uniform(base);
        for (int i = lane; i < nq; i += 64) {
            if (base + i < R.mis_cap) R.mis[base + i] = myq[i];
            else atomicExch(R.err, UVCGPU_EDEVICE);   // cannot happen: the queue holds every mismatching base of the simple alignments
        }
        nq = 0;
    };
    const __amdgpu_buffer_rsrc_t rs = bq_rsrc(R);
    // the work list is stored as four pos-sorted sub-lists, one per (is-reverse, bam_get_strand) class
    auto run_list = [&](auto IS, auto ST, int cls) {
    constexpr bool ISRC = decltype(IS)::value, STRAND = decltype(ST)::value;
    int lo = wave_uniform(win_lo(R, 1 + cls, (int)(x0 >> 6))), hi = wave_uniform(win_hi(R, 1 + cls, (int)(x0 >> 6)));
    if (NSL) { int slo, shi; uvc_link_slice(lo, hi, (int)(threadIdx.x >> 8), NSL, &slo, &shi); lo = wave_uniform(slo); hi = wave_uniform(shi); }   // this wave's part of the class
    // The base pass also counts the five cells of LINK_M that the fragment kernels read at every position (maxq_at): the aDP** counter of this
    // list's class and BQSUM, from the cover / hasL / incL expressions of the LINK pass.  The other 34 cells of LINK_M wait for a reader.
    int l5_dp = 0;
    constexpr bool DEAL = SPLIT && !NSL;   // the split form deals a window's chunks of 64 records to its four waves
    for (int k0 = lo + (DEAL ? 64 * (int)(threadIdx.x >> 6) : 0); k0 < hi; k0 += (DEAL ? 256 : 64)) {
        int c[16];
        if (DO_B) load_words(R.frec2 + (k0 + lane), k0 + lane < hi, c);   // (the LINK-only pass reads its records through the scalar cache, below)
        const int n = imin(64, hi - k0);
        // (the base pass requests the base | quality bytes P2_AHEAD reads ahead: one load per read and lane at HBM / L2 latency)
        auto fetch = [&](int j) { return bq_load(rs, bcast(c[FR_W(qb_lo)], j) + p); };   // low word of qbase + p: exact for lanes inside the read, harmless elsewhere
        auto one = [&](auto K, int bqn) {   // K(FR_W(field)): a field of the work-list record
            const int sym = bq_sym(bqn), q = bq_qual(bqn);
            const int apos = K(FR_W(pos)), rend = K(FR_W(rend));
            if (rend <= w0) return;
            const int fmd = K(FR_W(fmd));
            const int ext = K(FR_W(ext));
            SegRead sr;   // [apos, rend) is what this entry covers; the bias arithmetic uses the ends of the whole alignment
            sr.pos = apos - (ext & 0xFFFF); sr.rend = rend + (int)((unsigned)ext >> 16); sr.flag = fmd & 0xFFFF; sr.mapq = (fmd >> 16) & 0xFF; sr.dflag = (fmd >> 24) & 0xFF;
            sr.isize = K(FR_W(isize));
            const int mpos = K(FR_W(mpos));
            sr.frag_pos_L = imin(sr.pos, mpos); sr.frag_pos_R = sr.frag_pos_L + abs(sr.isize);
            sr.xm1500 = K(FR_W(xm1500));
            const int bm4c = K(FR_W(bm4c));
            sr.clip_cnt = (bm4c >> 16) & 0xF;
            const int nogap = (int)(short)(bm4c & 0xFFFF);
            sr.baq_pos = K(FR_W(baq_pos)); sr.baq_last = K(FR_W(baq_last)); sr.baq2_last = K(FR_W(baq2_last));
            const bool amplicon = (PLAIN ? false : is_assay_amplicon(sr.dflag, P));
            bool gate = true;
            if (amplicon && !normal_filter_primers) {   // primer gating, main.hpp:1872-1875, 1895
                constexpr bool isrc = ISRC;
                const int ibeg = ((sr.isize != 0) ? (sr.frag_pos_L + P.primerlen) : ((isrc && (0x0 == (0x1 & sr.flag))) ? 0 : (sr.pos + P.primerlen)));
                const int iend = ((sr.isize != 0) ? (int)nnminus(sr.frag_pos_L + abs(sr.isize), P.primerlen) : ((isrc && (0x0 == (0x1 & sr.flag))) ? (int)nnminus(sr.rend, P.primerlen) : INT32_MAX));
                gate = (ibeg <= p && p < iend);
            }
            // the queue bookkeeping below must run in wave-uniform control flow (nq is a scalar): no divergent `continue` before it
            // (one mask, not a chain of short-circuit tests: every `&&` of per-lane conditions is an exec-mask level of its own -- save, branch, restore)
            const bool cover = (valid & (p >= apos) & (p < rend) & gate);
            const bool hasL = DO_L && (p > apos), hasB = DO_B && (sym == my_ref);
            int inc = 0, incL = 0;
            if (proton) {   // IonTorrent values need neighbouring qualities and clip lengths: take them from the full record
                if (cover) {
                    const AlnRec &a = R.alns[K(FR_W(aln))];
                    if (DO_B) inc = simple_base_value(P, a, p, R.quals + a.qbase, true);
                    if (DO_L) incL = (p > apos ? simple_link_value(R, P, a, p, R.quals + a.qbase, true) : 0);
                }
            } else { inc = base_value(q, P); incL = (int)nnminus(noindel80, nogap) + 1; }
            const wmask mm = MQ ? BAL(cover && !hasB) : 0ull;
            if (MQ && mm) {   // bases that differ from the reference go to the wave's queue; k_p2_mism applies them
                if (nq > MISQ_CAP - 64) flush_queue();
                if (cover && !hasB) { MisItem it; it.rank = K(FR_W(aln)); it.epos = p; it.symval = sym | (inc << 8); myq[nq + (int)__builtin_popcountll(mm & ((1ull << lane) - 1ull))] = it; }
                nq += (int)__builtin_popcountll(mm);
            }
            if (L5_BASE) { const wmask ml = BAL(cover & (p > apos)); addm(l5_dp, ml); l5_bq += selm(ml, incL); }
            // a pass with one side acts on a lane iff that side has something there (one exec-mask level instead of cover, then hasL / hasB inside)
            constexpr bool ONE_SIDE = (DO_B != DO_L);
            if (!ONE_SIDE ? cover : (DO_B ? (cover & hasB) : (cover & hasL))) {
                const int bmv = K(FR_W(bmv)), xbv = K(FR_W(xbv));
                const int bm_inc = (sym < 4 ? ((bmv >> (8 * sym)) & 0xFF) : (xbv & 0xFF)), xm_inc = (xbv >> 8) & 0xFF;
                segbias_simple<ISRC, STRAND, PLAIN>(Alink, Aref, P, sr, T, p, baq_p, baq2_p, ONE_SIDE ? DO_L : hasL, ONE_SIDE ? DO_B : hasB, incL, inc, xm_inc, bm_inc, amp1, amp2);
            }
        };
        if (DO_B) {
            int r0 = fetch(0), r1 = (1 < n ? fetch(1) : 0);
#if P2_AHEAD == 4
            int r2 = (2 < n ? fetch(2) : 0), r3 = (3 < n ? fetch(3) : 0);
            for (int j = 0; j < n; j += 4) {
                { const int v = r0; if (j + 4 < n) r0 = fetch(j + 4); one([&](int i) { return bcast(c[i], j); }, v); }
                if (j + 1 < n) { const int v = r1; if (j + 5 < n) r1 = fetch(j + 5); one([&](int i) { return bcast(c[i], j + 1); }, v); }
                if (j + 2 < n) { const int v = r2; if (j + 6 < n) r2 = fetch(j + 6); one([&](int i) { return bcast(c[i], j + 2); }, v); }
                if (j + 3 < n) { const int v = r3; if (j + 7 < n) r3 = fetch(j + 7); one([&](int i) { return bcast(c[i], j + 3); }, v); }
            }
#else
#ifdef UVC_P2_BASE_VECREC
            for (int j = 0; j < n; j += 2) {
                { const int v = r0; if (j + 2 < n) r0 = fetch(j + 2); one([&](int i) { return bcast(c[i], j); }, v); }
                if (j + 1 < n) { const int v = r1; if (j + 3 < n) r1 = fetch(j + 3); one([&](int i) { return bcast(c[i], j + 1); }, v); }
            }
#else
            // the record's fields through the scalar cache as in the LINK pass; the per-lane copy of the chunk stays for the one field the byte
            // requests need two reads ahead (fetch)
            typedef int v4i_ __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(4))) const v4i_ *crec4;
            v4i_ a0, a1, a2, a3;
            const int kb = wave_uniform(k0), nb = wave_uniform(n);
            { crec4 q = (crec4)(R.frec2 + kb); a0 = q[0]; a1 = q[1]; a2 = q[2]; a3 = q[3]; }
            for (int j = 0; j < nb; j += 2) {
                { const int v = r0; if (j + 2 < nb) r0 = fetch(j + 2);
                  const v4i_ c0 = a0, c1 = a1, c2 = a2, c3 = a3;
                  if (j + 1 < nb) { crec4 q = (crec4)(R.frec2 + (kb + j + 1)); a0 = q[0]; a1 = q[1]; a2 = q[2]; a3 = q[3]; }
                  one([&](int i) { const v4i_ w = (i < 4 ? c0 : i < 8 ? c1 : i < 12 ? c2 : c3); return (int)w[i & 3]; }, v); }
                if (j + 1 < nb) { const int v = r1; if (j + 3 < nb) r1 = fetch(j + 3);
                  const v4i_ c0 = a0, c1 = a1, c2 = a2, c3 = a3;
                  if (j + 2 < nb) { crec4 q = (crec4)(R.frec2 + (kb + j + 2)); a0 = q[0]; a1 = q[1]; a2 = q[2]; a3 = q[3]; }
                  one([&](int i) { const v4i_ w = (i < 4 ? c0 : i < 8 ? c1 : i < 12 ? c2 : c3); return (int)w[i & 3]; }, v); }
            }
#endif
#endif
        } else {
            // The LINK pass reads no read bytes: its only per-read data is the 64-byte work-list record.  Straight into scalar registers (s_load through
            // the constant address space, the next record requested while this one is worked on) instead of a per-lane vector load of 64 records and
            // eleven v_readlane per read.
            typedef int v4i_ __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(4))) const v4i_ *crec4;
            v4i_ a0, a1, a2, a3;
            const int kb = wave_uniform(k0), nb = wave_uniform(n);   // (the split form's k0 depends on the wave's number in the block: uniform, but not to the compiler)
            { crec4 q = (crec4)(R.frec2 + kb); a0 = q[0]; a1 = q[1]; a2 = q[2]; a3 = q[3]; }
            for (int j = 0; j < nb; j++) {
                const v4i_ c0 = a0, c1 = a1, c2 = a2, c3 = a3;   // (sixteen s_mov; two register sets and a loop unrolled by two measured slower: 1.27 against 1.24 ms)
                if (j + 1 < nb) { crec4 q = (crec4)(R.frec2 + (kb + j + 1)); a0 = q[0]; a1 = q[1]; a2 = q[2]; a3 = q[3]; }
                one([&](int i) { const v4i_ w = (i < 4 ? c0 : i < 8 ? c1 : i < 12 ? c2 : c3); return (int)w[i & 3]; }, 0);
            }
        }
        if (DO_B) Aref.fold();
        if (DO_L) Alink.fold();
    }
    if (L5_BASE && l5_dp) {
        constexpr int f = (STRAND ? (ISRC ? UVC_S_aDPrr : UVC_S_aDPrf) : (ISRC ? UVC_S_aDPfr : UVC_S_aDPff));
        if (SPLIT) atomicAdd(&red[P2_RED_LINK5 + cls][lane], l5_dp);
        else if (valid) S32(R, f, UVC_LINK_M, x) = l5_dp;
    }
    };
    COARSE_T(ct1)
    if (NSL) {   // one class per wave: ISRC and STRAND stay compile-time behind a wave-uniform switch
        switch (wave_uniform((int)(threadIdx.x >> 6) & 3)) {
        case 0: run_list(std::false_type{}, std::false_type{}, 0); break;
        case 1: run_list(std::true_type{}, std::false_type{}, 1); break;
        case 2: run_list(std::false_type{}, std::true_type{}, 2); break;
        default: run_list(std::true_type{}, std::true_type{}, 3); break;
        }
    } else {
    run_list(std::false_type{}, std::false_type{}, 0);
    run_list(std::true_type{}, std::false_type{}, 1);
    run_list(std::false_type{}, std::true_type{}, 2);
    run_list(std::true_type{}, std::true_type{}, 3);
    }
    if (MQ && nq > 0) flush_queue();
    COARSE_T(ct2)
    if (SPLIT) {   // the four partial sets -> LDS -> one set (the two passes own different symbols: one symbol per kernel)
        const SegAcc &A = (DO_B ? Aref : Alink);
#pragma unroll
        for (int f = 0; f < UVC_NSEG32; f++) if (A.s[f] && !(DO_L && !L5_LINK && seg_is_adp(f))) atomicAdd(&red[f][lane], A.s[f]);
#pragma unroll
        for (int f = 0; f < UVC_NSEG64; f++) if (A.l[f]) atomicAdd(&red64(red, f)[lane], (unsigned long long)A.l[f]);
        if (A.a1BQf) atomicAdd(&red[UVC_NSEG32 + 2 * UVC_NSEG64 + 0][lane], A.a1BQf);
        if (A.a1BQr) atomicAdd(&red[UVC_NSEG32 + 2 * UVC_NSEG64 + 1][lane], A.a1BQr);
        if (A.a2BQf) atomicAdd(&red[UVC_NSEG32 + 2 * UVC_NSEG64 + 2][lane], A.a2BQf);
        if (A.a2BQr) atomicAdd(&red[UVC_NSEG32 + 2 * UVC_NSEG64 + 3][lane], A.a2BQr);
        if ((DO_B || L5_LINK) && A.bq) atomicAdd(&red[UVC_NSEG32 + 2 * UVC_NSEG64 + 4][lane], A.bq);
        if (L5_BASE && l5_bq) atomicAdd(&red[P2_RED_LINK5 + 4][lane], l5_bq);
        __syncthreads();
        if (DO_L && threadIdx.x == 0) R.link_done[wave] = 1;   // once per window, behind the block's barrier
        if (!valid) return;
        const int sym = (DO_B ? my_ref : UVC_LINK_M), wv = (int)(threadIdx.x >> 6);
        // the base pass is the first writer of its cells: plain stores.  The completion pass adds to what k_p2_items has put there (seg_add_link)
        auto put = [](auto &cell, auto v) { if (DO_L) cell += v; else cell = v; };
        for (int f = wv; f < UVC_NSEG32; f += NWV) { const int v = red[f][lane]; if (v) put(S32(R, f, sym, x), v); }
        for (int f = wv; f < UVC_NSEG64; f += NWV) { const long long v = (long long)red64(red, f)[lane]; if (v) put(S64(R, f, sym, x), v); }
        if (wv == 0) {
            const int b0 = UVC_NSEG32 + 2 * UVC_NSEG64;
            if (red[b0][lane]) put(VQP(R, UVC_VQ_a1BQf, sym, x), red[b0][lane]);
            if (red[b0 + 1][lane]) put(VQP(R, UVC_VQ_a1BQr, sym, x), red[b0 + 1][lane]);
            if (red[b0 + 2][lane]) put(VQP(R, UVC_VQ_a2BQf, sym, x), red[b0 + 2][lane]);
            if (red[b0 + 3][lane]) put(VQP(R, UVC_VQ_a2BQr, sym, x), red[b0 + 3][lane]);
            if ((DO_B || L5_LINK) && red[b0 + 4][lane]) put(BQS(R, sym, x), red[b0 + 4][lane]);
        }
        if (L5_BASE && wv == 1) {   // the five cells of LINK_M
            const int l0 = P2_RED_LINK5;
            if (red[l0][lane]) S32(R, UVC_S_aDPff, UVC_LINK_M, x) = red[l0][lane];
            if (red[l0 + 1][lane]) S32(R, UVC_S_aDPfr, UVC_LINK_M, x) = red[l0 + 1][lane];
            if (red[l0 + 2][lane]) S32(R, UVC_S_aDPrf, UVC_LINK_M, x) = red[l0 + 2][lane];
            if (red[l0 + 3][lane]) S32(R, UVC_S_aDPrr, UVC_LINK_M, x) = red[l0 + 3][lane];
            if (red[l0 + 4][lane]) BQS(R, UVC_LINK_M, x) = red[l0 + 4][lane];
        }
        return;
    }
    if (DO_L && lane == 0) R.link_done[wave] = 1;
    if (!valid) return;
    // the base pass is the only writer of the reference symbol's cells in front of k_p2_items (k_p2_mism writes the other symbols'): plain stores, also for its five cells of LINK_M
    if (DO_B) { seg_store(R, Aref, my_ref, x); if (L5_BASE && l5_bq) BQS(R, UVC_LINK_M, x) = l5_bq; }
    if (DO_L) seg_add_link<L5_LINK>(R, Alink, x);
#ifdef UVC_FRAG_COARSE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    COARSE_T(ct3)
    if (lane == 0 && (wave % 2999) == 7) printf("coarse p2<%d,%d> wave %d prologue %llu lists %llu epilogue %llu\n", (int)DO_L, (int)DO_B, wave, ct1 - ct0, ct2 - ct1, ct3 - ct2);
#endif
}
// The plain base pass under these names reads a queue that P1 made; the generic base pass makes its own.  k_p2_fast_q / k_p2_fast_split_q
// are the plain base pass that still makes the queue (misq=p2: UVCGPU_MISQ=p2, for comparison item by item).
template <bool DO_L, bool DO_B, bool PLAIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) k_p2_fast(RegionDev R, UvcParams P) {
    constexpr bool MQ = DO_B && !PLAIN;
    __shared__ int amp1[256 + AMP_LO], amp2[256 + AMP_LO];
    __shared__ MisItem misq[MQ ? 4 : 1][MQ ? MISQ_CAP : 1];
    p2_fast_body<DO_L, DO_B, PLAIN, false, 0, MQ>(R, P, amp1, amp2, misq);
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) k_p2_fast_q(RegionDev R, UvcParams P) {
    __shared__ int amp1[256 + AMP_LO], amp2[256 + AMP_LO];
    __shared__ MisItem misq[4][MISQ_CAP];
    p2_fast_body<false, true, true, false, 0, true>(R, P, amp1, amp2, misq);
}
template <bool DO_L, bool DO_B, bool PLAIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_p2_fast_split(RegionDev R, UvcParams P) {
    constexpr bool MQ = DO_B && !PLAIN;
    __shared__ int amp1[256 + AMP_LO], amp2[256 + AMP_LO];
    __shared__ MisItem misq[MQ ? 4 : 1][MQ ? MISQ_CAP : 1];
    __shared__ __attribute__((aligned(8))) int red[P2_RED_SLOTS][64];
    p2_fast_body<DO_L, DO_B, PLAIN, true, 0, MQ>(R, P, amp1, amp2, misq, red);
}
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_p2_fast_split_q(RegionDev R, UvcParams P) {
    __shared__ int amp1[256 + AMP_LO], amp2[256 + AMP_LO];
    __shared__ MisItem misq[4][MISQ_CAP];
    __shared__ __attribute__((aligned(8))) int red[P2_RED_SLOTS][64];
    p2_fast_body<false, true, true, true, 0, true>(R, P, amp1, amp2, misq, red);
}
// The sparse form of the plain completion pass: where few windows are needed the wave-per-window form is bound by the length of
// one wave's walk over a window's four class lists, not by the number of windows.  Here a block of 4 * NSL waves shares one window, and the
// blocks stride over the list that k_link_mark made (RegionDev::link_list, link_cnt); a listed window that an earlier launch has run is
// skipped on its link_done byte.  A window is in the list once, so no two blocks meet; no block waits for another.
template <int NSL>
__global__ void __launch_bounds__(256 * NSL) k_p2_link_sparse(RegionDev R, UvcParams P) {
    __shared__ int amp1[256 + AMP_LO], amp2[256 + AMP_LO];
    __shared__ MisItem misq[1][1];
    __shared__ __attribute__((aligned(8))) int red[P2_RED_SLOTS][64];
    const int n = imin(*R.link_cnt, R.nwin);
    if ((int)blockIdx.x >= n) return;
    for (int v = (int)threadIdx.x - AMP_LO; v < 256; v += (int)blockDim.x) {   // as in p2_fast_body
        const int d1 = P.bias_thres_PFBQ1 * P.bias_thres_PFBQ1, d2 = P.bias_thres_PFBQ2 * P.bias_thres_PFBQ2;
        amp1[v + AMP_LO] = ((v < P.bias_thres_PFBQ1 && d1) ? 100 * (v * v) / d1 : 100);
        amp2[v + AMP_LO] = ((v < P.bias_thres_PFBQ2 && d2) ? 100 * (v * v) / d2 : 100);
    }
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int w = wave_uniform(R.link_list[i]);
        if ((unsigned)w < (unsigned)R.nwin && uvc_link_window_runs(R.link_need[w], R.link_done[w])) p2_fast_body<true, false, true, true, NSL, false>(R, P, amp1, amp2, misq, red, w);
        __syncthreads();   // the next window zeroes the reduction area
    }
}

// ------------------------------------------------------------------------------------------------
// k_p2_mism: the queued mismatching bases of simple alignments, one lane per item
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_p2_mism(RegionDev R, UvcParams P) {
    const int n = imin(*R.mis_cnt, R.mis_cap);
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) mis_apply(R, P, R.mis[t]);
}

// ------------------------------------------------------------------------------------------------
// sequential updateByAln for one complex alignment (main.hpp:1762-2296).
//   BIAS = true : SYMBOL_COUNT_SUM + dealwith_segbias, flushed with atomics (P2)
//   BIAS = false: BASE_QUALITY_MAX values written to the contribution table (used by P3/P4/P5)
// ------------------------------------------------------------------------------------------------
DEV int indel_len_rusize_phred_dev(int indel_len, int repeatunit_size) {   // main.hpp:757-790
    const int t[19] = { 0, 0, 3, 5, 6, 7, 8, 8, 9, 10, 10, 10, 11, 11, 11, 12, 12, 12, 13 };
    if (0 == (indel_len % repeatunit_size)) return t[imin(indel_len / repeatunit_size, 18)];
    return t[imin(indel_len, 18)];
}
DEV int indel_phred_dev(double ampfact, int rs, int rn) {   // main.hpp:794-801
    const int region_size = rs * rn;
    const double num_slips = (region_size > 64 ? (double)(region_size - 8) : log1p(exp((double)region_size - (double)8))) * ampfact / ((double)(rs * rs));
    const double pr = (1.0 - 2.220446049250313e-16) / (num_slips + 1.0);
    return (int)floor(-10 * log(pr) / log(10.0));
}
DEV bool more_STR(int rulen1, int rc1, int rulen2, int rc2, int strmax) {   // is_indel_context_more_STR, main.hpp:699-721
    if (rulen2 * rc2 == 0) return true;
    if (rulen1 > strmax || rulen2 > strmax) return (rulen1 < rulen2 || (rulen1 == rulen2 && rc1 > rc2));
    int rank1 = (rc1 <= 1 ? (-rc1 * rulen1) : ((rc1 - 1) * rulen1));
    int rank2 = (rc2 <= 1 ? (-rc2 * rulen1) : ((rc2 - 1) * rulen2));
    if (0 == rc1 || 0 == rulen1) rank1 = -100;
    if (0 == rc2 || 0 == rulen2) rank2 = -100;
    return rank1 > rank2;
}
DEV int ref_to_phredvalue_dev(int &n_units, int &max_rn, int &rs_at_max, const RegionDev &R, const UvcParams &P, int refidx, int max_phred, double ampfact, int oplen, int op) {   // main.hpp:876-922
    const int n = (int)R.npos - 1;   // refstring.size()
    max_rn = 0; rs_at_max = 0;
    for (int rs = 1; rs <= P.indel_str_repeatsize_max; rs++) {
        int q = refidx;
        while (q + rs < n && R.refsym[q] == R.refsym[q + rs]) q++;
        const int rn = (q - refidx) / rs + 1;
        if (more_STR(rs, rn, rs_at_max, max_rn, P.indel_str_repeatsize_max)) { max_rn = rn; rs_at_max = rs; }
    }
    if (oplen == rs_at_max && op == C_DEL) ampfact *= P.indel_del_to_ins_err_ratio;
    const int decphred = indel_phred_dev(ampfact, rs_at_max, max_rn);
    if (rs_at_max * (max_rn - 1) >= 6 - 1) n_units = ((0 == oplen % rs_at_max) ? (oplen / rs_at_max) : ((1 == oplen) ? 1 : 0));
    else n_units = 1 + (oplen / 6);
    return max_phred - imin(max_phred, decphred) + indel_len_rusize_phred_dev(oplen, rs_at_max);
}
DEV int proton_cigarlen2phred(int cigarlen) { const int t[13] = { 0, 0, 9, 14, 18, 21, 23, 25, 27, 29, 30, 31, 32 }; return t[imin(cigarlen, 12)]; }

DEV void table_put(const RegionDev &R, Contrib *row, int sym, int v) {
    const uint16_t vv = (uint16_t)imin(imax(v, 0), 65535);
    if (sym <= UVC_BASE_NN) {
        if (row->bsym_p1 == 0 || row->bsym_p1 == sym + 1) { row->bval = (row->bsym_p1 == sym + 1) ? (uint16_t)imax((int)row->bval, (int)vv) : vv; row->bsym_p1 = (uint8_t)(sym + 1); }
        else atomicExch(R.err, UVCGPU_EDEVICE);   // two different bases of one read at one reference position: no CIGAR does that
        return;
    }
    const int k = sym - UVC_LINK_M;   // one slot per LINK symbol: any pile fits
    if (row->lmask & (1 << k)) row->lval[k] = (uint16_t)imax((int)row->lval[k], (int)vv);
    else { row->lmask = (uint8_t)(row->lmask | (1 << k)); row->lval[k] = vv; }
}

template <bool BIAS>
__global__ void __launch_bounds__(64) k_p2_slow(RegionDev R, UvcParams P) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R.n_complex) return;
    const AlnRec a = R.alns[R.complex_ids[t]];
    const uint32_t *cigar = R.cigars + a.cigar_off;
    const uint8_t *bases = R.bases + a.seq_off, *quals = R.quals + a.seq_off;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const int off = R.beg, rend = a.rend, n_cigar = a.n_cigar;
    const bool amplicon = is_assay_amplicon(a.dflag, P);
    const bool normal_filter_primers = normal_filters_primers(P);
    const int addMis = P.bq_phred_added_misma, addInd = P.bq_phred_added_indel;
    Contrib *table = BIAS ? nullptr : (R.table + a.table_off);
    auto Q = [&](int q) -> int { return (int)quals[imin(imax(q, 0), a.l_qseq - 1)]; };
    Item *items = BIAS ? (R.items + a.item_off) : nullptr;
    int n_items = 0;
    auto emit = [&](bool gap, int epos, int sym, int v, int bm, int op, int indel_len, int dist) {
        if (BIAS) {   // the bias update itself is applied by k_p2_items, in parallel over the items
            Item it; it.epos = epos; it.sym = (uint8_t)sym; it.flags = (uint8_t)((gap ? 1 : 0) | (op << 1)); it.val = v;
            it.dist = (uint16_t)imin(imax(dist, 0), 65535); it.indel_len = (uint16_t)imin(indel_len, 65535); it.pad1_ = 0;
            items[n_items++] = it;
        } else if (epos >= a.pos && epos <= a.rend) table_put(R, table + (epos - a.pos), sym, v);
        else atomicExch(R.err, UVCGPU_EDEVICE);   // would leave the read's rows
    };
    // low-BQ InDel positions (main.hpp:1817-1859): a list of the read's own in global memory (one slot per I / D op + two sentinels), so
    // that a read with any number of them is walked like every other read
    int32_t *indel_rposs = R.ir_list + a.gap_off + 2 * (int64_t)t; int n_ir = 0;
    if (BIAS) indel_rposs[n_ir++] = 0;
    int nge = 0;
    {
        int qpos = 0, rpos = a.pos;
        for (int i = 0; i < n_cigar; i++) {
            const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
            if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) { qpos += len; rpos += len; }
            else if (op == C_INS) {
                nge += len;
                bool low = false;
                for (int q2 = qpos - imin(qpos, 1); q2 < imin(qpos + len + 1, rend); q2++) if (Q(q2) < P.bias_thres_interfering_indel_BQ) low = true;
                if (low && BIAS) indel_rposs[n_ir++] = rpos;
                qpos += len;
            } else if (op == C_DEL) {
                nge += len;
                const bool low = (imin(Q(imax(1, qpos) - 1), Q(qpos)) <= P.bias_thres_interfering_indel_BQ);
                if (low && BIAS) indel_rposs[n_ir++] = rpos;
                rpos += len;
            } else if (op == C_REF_SKIP) rpos += len;
            else if (op == C_SOFT_CLIP) qpos += len;
        }
        if (BIAS) indel_rposs[n_ir++] = INT32_MAX;
    }
    int ir_idx = 0;
    int ibeg, iend;
    primer_window(P, a, ibeg, iend);
    const int atd = P.indel_adj_tracklen_dist, nrtr = (int)R.npos;
    const int xm1500 = a.xm1500;
    int qpos = 0, rpos = a.pos, incvalue = 1;
    int gi = 0;   // ordinal of the I / D op: slot of its AlnGap event
    auto gap_event = [&](int sym, int len, int weight) {
        AlnGap g; g.epos = rpos; g.sym = sym; g.len = len; g.qpos = qpos; g.weight = weight; g.aln = a.id; g.mark = 0; g.pad_ = 0;
        R.gap.ev[a.gap_off + gi] = g;
    };
    for (int i = 0; i < n_cigar; i++) {
        const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
        if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) {
            if (BIAS && a.kind == 2) { rpos += len; qpos += len; continue; }   // the M runs of this read are on the P2 work list of k_p2_fast
            for (int i2 = 0; i2 < len; i2++) {
                if ((normal_filter_primers || !amplicon) || (ibeg <= rpos && rpos < iend)) {
                    int dist = 10000;
                    if (BIAS && nge > 0) {
                        if (indel_rposs[ir_idx] <= rpos) ir_idx++;
                        const int prev_ir = indel_rposs[ir_idx - 1], next_ir = indel_rposs[ir_idx];
                        const int i1 = imax(rpos - off, atd) - atd, i2r = imin(rpos - off + atd, nrtr - 1);
                        const long long prevlen = nnminus(rpos - prev_ir, imax(rpos - (off + RTRP(R, UVC_RTR_begpos, i1)), TH(R, UVC_T_aLP1t, rpos - off)));
                        const long long nextlen = nnminus((long long)next_ir - rpos, imax((off + RTRP(R, UVC_RTR_begpos, i2r) + RTRP(R, UVC_RTR_tracklen, i2r)) - rpos, TH(R, UVC_T_aRP1t, rpos - off)));
                        dist = (int)lmin(prevlen, nextlen);
                    }
                    if (i2 > 0) {
                        const int noindel = imin(RTRP(R, UVC_RTR_indelphred, rpos - off - 1), RTRP(R, UVC_RTR_indelphred, rpos - off));
                        const int qfromBQ2 = (proton ? imin(Q(qpos - 1), Q(qpos)) : 80);
                        incvalue = (int)nnminus(imin(qfromBQ2, noindel), a.nogap_penal) + 1;
                        emit(true, rpos, UVC_LINK_M, incvalue, 0, op, 0, dist);
                    }
                    const int symbol = bases[qpos];
                    if (proton && ((0 == i2) || (len - 1 == i2))) {
                        const bool next_gap = (len - 1 == i2), prev_gap = (0 == i2);   // packed words != op codes, main.hpp:1953-1956
                        const bool isrc2 = (0 != i2);
                        int prev_base_phred = 1;
                        if (isrc2 && (qpos + 1 < a.l_qseq)) prev_base_phred = Q(qpos + 1);
                        if ((!isrc2) && (qpos > 0)) prev_base_phred = Q(qpos - 1);
                        int adj = 100;
                        if (next_gap) adj = imin(adj, ((i + 1 < n_cigar) ? cig_len(cigar[i + 1]) : 100));
                        if (prev_gap) adj = imin(adj, ((0 < i) ? cig_len(cigar[i - 1]) : 100));
                        if (adj < 3) incvalue = imin(Q(qpos), prev_base_phred) + imin(addMis, addInd);
                        else incvalue = imin(Q(qpos), prev_base_phred) + addMis;
                    } else incvalue = Q(qpos) + addMis;
                    emit(false, rpos, symbol, incvalue, a.bm1500[symbol], op, 0, dist);
                }
                rpos += 1; qpos += 1;
            }
        } else if (op == C_INS) {
            bool gapped = false;
            if ((normal_filter_primers || !amplicon) || (ibeg <= rpos && rpos < iend)) {
                const int nbases2end = imin(qpos, a.l_qseq - (qpos + len));
                int inslen = len;
                if (nbases2end <= 0) {
                    incvalue = (0 != qpos ? Q(qpos - 1) : ((qpos + len < a.l_qseq) ? Q(qpos + len) : 1)) + addInd;
                } else {
                    int max_rn, rs_at_max;
                    int phredvalue = ref_to_phredvalue_dev(inslen, max_rn, rs_at_max, R, P, rpos - off, P.indel_BQ_max, P.indel_polymerase_slip_rate, len, op);
                    const int64_t x = rpos - off;
                    const int adp = P32(R, UVC_P_a_dp, x);
                    // adp == 0 is undefined behaviour in the reference (round(-inf) -> int); defined here and in the oracle as "no bonus"
                    const int phredinc = (adp > 0 ? (int)round(2 * ((10.0 / log(10.0)) * log((double)adp / (double)(1.0 + nnminus(adp, P32(R, UVC_P_a_at_ins_dp, x) + P32(R, UVC_P_a_at_del_dp, x)))))) : -1000000);
                    const int ratiothres = (!P.tumor_vcf_is_provided ? 2 : 4);
                    const bool multiallelic = (P64(R, UVC_P_a_near_ins_pow2len, x) * ratiothres > (long long)imax(1, P32(R, UVC_P_a_near_ins_dp, x)) * (long long)((unsigned)len * 3u));
                    if (1 == inslen && !multiallelic) phredvalue += ibetween(phredinc - 3, 0, 4);
                    const int thisdp = P32(R, UVC_P_a_at_ins_dp, x);
                    const int neardp = imax(P32(R, UVC_P_a_near_ins_dp, x), P32(R, UVC_P_a_near_RTR_ins_dp, x));
                    int insbase_minphred = 80;
                    for (int q2 = qpos; q2 < qpos + len; q2++) insbase_minphred = imin(insbase_minphred, Q(q2));
                    int ancbase_minphred = 80;
                    if (qpos > 0) ancbase_minphred = imin(ancbase_minphred, Q(qpos - 1));
                    if (qpos + len + 1 < a.l_qseq) ancbase_minphred = imin(ancbase_minphred, Q(qpos + len + 1));
                    int minq = 80;
                    if (proton && (1 == len) && (1 == rs_at_max) && (1 < max_rn))
                        for (int qinc = 0; (qinc < max_rn + 2) && (qpos + qinc) < a.l_qseq; qinc++) if (bases[qpos + qinc] == bases[qpos]) minq = imin(minq, Q(qpos + qinc));
                    const bool isrc = (a.flag & 0x10) != 0;
                    const int qfromBQ1 = (proton ? imin(ancbase_minphred, minq) : imin(ancbase_minphred, insbase_minphred));
                    const int qfromBQ2 = ((thisdp * ratiothres <= neardp || (1 == len && (xm1500 >= P.microadjust_xm
                                 || ((a.lclip_len + P.microadjust_cliplen >= rpos - a.pos) && isrc) || ((a.rclip_len + P.microadjust_cliplen >= rend - a.pos) && !isrc))))
                            ? qfromBQ1 : (proton ? imin(qfromBQ1 + proton_cigarlen2phred(len), imax(3, qfromBQ1) * len) : 80));
                    incvalue = (int)nnminus(imin(qfromBQ2, phredvalue + addInd), a.indel_penal) + 1;
                }
                if (nbases2end >= P.indel_filter_edge_dist) {
                    const int symbol = (1 == inslen ? UVC_LINK_I1 : ((2 == inslen) ? UVC_LINK_I2 : UVC_LINK_I3P));
                    emit(true, rpos, symbol, imax(1, incvalue), 0, op, len, 10000);
                    if (!BIAS) {   // incIns, main.hpp:2101-2113
                        int incvalue2 = incvalue;
                        for (int i2 = 0; i2 < len; i2++) incvalue2 = imin(incvalue2, Q(qpos + i2) + addInd);
                        gap_event(symbol, len, imax(1, incvalue2)); gapped = true;
                    }
                }
            }
            if (!BIAS) { if (!gapped) gap_event(-1, len, 0); gi++; }
            qpos += len;
        } else if (op == C_DEL) {
            bool gapped = false;
            if ((normal_filter_primers || !amplicon) || (ibeg <= rpos && rpos < iend)) {
                const int nbases2end = imin(qpos, a.l_qseq - qpos);
                int dellen = len;
                if (nbases2end <= 0) {
                    incvalue = (0 != qpos ? Q(qpos - 1) : ((qpos < a.l_qseq) ? Q(qpos) : 1)) + addInd;
                } else {
                    int max_rn, rs_at_max;
                    int phredvalue = ref_to_phredvalue_dev(dellen, max_rn, rs_at_max, R, P, rpos - off, P.indel_BQ_max, P.indel_polymerase_slip_rate, len, op);
                    const int64_t x = rpos - off;
                    const int adp = P32(R, UVC_P_a_dp, x);
                    // adp == 0 is undefined behaviour in the reference (round(-inf) -> int); defined here and in the oracle as "no bonus"
                    const int phredinc = (adp > 0 ? (int)round(2 * ((10.0 / log(10.0)) * log((double)adp / (double)(1.0 + nnminus(adp, P32(R, UVC_P_a_at_ins_dp, x) + P32(R, UVC_P_a_at_del_dp, x)))))) : -1000000);
                    if (1 == dellen) phredvalue += ibetween(phredinc - 3, 0, 4);
                    const int thisdp = P32(R, UVC_P_a_at_del_dp, x);
                    const int neardp = imax(P32(R, UVC_P_a_near_del_dp, x), P32(R, UVC_P_a_near_RTR_del_dp, x));
                    int minq = 80;
                    if (proton && (1 == len) && (1 == rs_at_max) && (1 < max_rn))
                        for (int qinc = 0; qinc < (max_rn + 2) && (qpos + qinc) < a.l_qseq; qinc++) if (bases[qpos + qinc] == bases[qpos]) minq = imin(minq, Q(qpos + qinc));
                    const int qfromBQ1 = imin(Q(qpos), imin(Q(qpos - 1), minq));
                    const int ratiothres = (!P.tumor_vcf_is_provided ? 2 : 4);
                    const int qfromBQ2 = ((thisdp * ratiothres <= neardp) ? (int)nnminus(qfromBQ1, 1) : (proton ? imin(qfromBQ1 + proton_cigarlen2phred(len), imax(3, qfromBQ1) * len) : 80));
                    const double delFA = ((double)(thisdp + 0.5) / (double)(adp + 1));
                    const int delFAQ = imax(0, P.microadjust_delFAQmax + (int)round(P.powlaw_exponent * ((10.0 / log(10.0)) * log(delFA))));
                    int prev_cidx = i, prev_rpos = rpos;
                    while ((0 != prev_cidx) && (C_INS != cig_op(cigar[prev_cidx]) || len != cig_len(cigar[prev_cidx]))) {
                        prev_cidx--;
                        const int o = cig_op(cigar[prev_cidx]);
                        if (C_MATCH == o || C_EQUAL == o || C_DIFF == o || C_DEL == o || C_REF_SKIP == o) prev_rpos -= cig_len(cigar[prev_cidx]);
                    }
                    int next_cidx = i, next_rpos = rpos + len;
                    while ((n_cigar - 1 != next_cidx) && (C_INS != cig_op(cigar[next_cidx]) || len != cig_len(cigar[next_cidx]))) {
                        next_cidx++;
                        const int o = cig_op(cigar[next_cidx]);
                        if (C_MATCH == o || C_EQUAL == o || C_DIFF == o || C_DEL == o || C_REF_SKIP == o) next_rpos += cig_len(cigar[next_cidx]);
                    }
                    const int qfromBAQl = (int)(BAQ1(R, rpos) - BAQ1(R, prev_rpos));
                    const int qfromBAQr = (int)(BAQ1(R, next_rpos) - BAQ1(R, rpos + len));
                    const int qfromBAQ = imax(delFAQ, imax(qfromBQ1, imin(qfromBAQl, qfromBAQr)));
                    incvalue = (int)nnminus(imin(qfromBQ2, imin(qfromBAQ, phredvalue + addInd)), a.indel_penal) + 1;
                }
                if (nbases2end >= P.indel_filter_edge_dist) {
                    const int symbol = (1 == dellen ? UVC_LINK_D1 : ((2 == dellen) ? UVC_LINK_D2 : UVC_LINK_D3P));
                    emit(true, rpos, symbol, imax(1, incvalue), 0, op, len, 10000);
                    if (!BIAS) { gap_event(symbol, len, imax(1, incvalue)); gapped = true; }   // incDel, main.hpp:2216
                    for (int r2 = rpos; r2 < imin(rpos + len, rend); r2++) {   // padded deletion, main.hpp:2219-2253
                        for (int k = 0; k < 2; k++) {
                            const int s = (k == 0 ? UVC_BASE_NN : UVC_LINK_NN);
                            const int pp = ((UVC_BASE_NN == s) ? r2 : (r2 + 1));
                            if (pp >= rend) continue;
                            int dist = 0;
                            if (BIAS) {
                                if (indel_rposs[ir_idx] <= rpos) ir_idx++;
                                const unsigned prev_ir = (unsigned)indel_rposs[ir_idx - 1], next_ir = (unsigned)indel_rposs[ir_idx];
                                const unsigned d1 = (unsigned)rpos - prev_ir, d2 = next_ir - (unsigned)rpos;
                                dist = (int)(d1 < d2 ? d1 : d2);
                            }
                            emit(true, pp, s, imax(1, incvalue), 0, op, len, dist);
                        }
                    }
                }
            }
            if (!BIAS) { if (!gapped) gap_event(-1, len, 0); gi++; }
            rpos += len;
        } else {
            if (op == C_REF_SKIP) rpos += len; else if (op == C_SOFT_CLIP) qpos += len;
        }
    }
    if (BIAS) R.item_cnt[t] = n_items;
}

template __global__ void k_p2_slow<true>(RegionDev, UvcParams);
template __global__ void k_p2_slow<false>(RegionDev, UvcParams);

// applies the items of one InDel read: one wave per read, lanes stride over the items
__global__ void __launch_bounds__(64) k_p2_items(RegionDev R, UvcParams P) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= R.n_complex) return;
    const AlnRec &a = R.alns[R.complex_ids[t]];
    const SegRead sr = make_segread(R, a);
    const Item *items = R.items + a.item_off;
    const int n = R.item_cnt[t];
    for (int k = lane; k < n; k += 64) {
        const Item it = items[k];
        const int64_t x = it.epos - R.beg;
        SegAcc A; A.zero(); A.bq = it.val;
        PosThres T; load_thres(R, T, x);
        const int op = (it.flags >> 1) & 0xF;
        const int dist = (it.dist == 65535 ? 10000 : (int)it.dist);   // 10000 / large distances are clamped on emit; every use compares with small thresholds
        if (it.flags & 1) segbias<true>(A, P, sr, T, it.epos, R.baq[x], R.baq[R.npos + x], it.val, 0, op, it.indel_len, dist);
        else              segbias<false>(A, P, sr, T, it.epos, R.baq[x], R.baq[R.npos + x], it.val, a.bm1500[it.sym], op, it.indel_len, dist);
        seg_flush(R, A, it.sym, x);
    }
}

// ------------------------------------------------------------------------------------------------
// contribution of ANY alignment at position p: simple ones are computed on the fly, complex ones
// come from the table.  Values are merged into the per-fragment symbol counts with MAX.
// ------------------------------------------------------------------------------------------------
DEV void aln_contrib_max(const RegionDev &R, const UvcParams &P, const AlnRec &a, int p, bool proton, int *cnt /*[NSYM]*/) {
    // an InDel read can carry an insertion symbol at rpos == rend (CIGAR ...M I [S]): its table has one row more than the read spans
    if (p < a.pos || p > a.rend || (p == a.rend && a.kind == 0)) return;
    if (a.kind == 0) {
        if (amplicon_gated(a.dflag, P)) {
            int ibeg, iend; primer_window(P, a, ibeg, iend);
            if (!(ibeg <= p && p < iend)) return;
        }
        const uint8_t *qq = R.quals + a.qbase;
        if (p > a.pos) { const int v = simple_link_value(R, P, a, p, qq, proton); cnt[UVC_LINK_M] = imax(cnt[UVC_LINK_M], v); }
        const int sym = R.bases[a.qbase + p];
        const int v = simple_base_value(P, a, p, qq, proton);
        cnt[sym] = imax(cnt[sym], v);
    } else {
        const Contrib c = R.table[a.table_off + (p - a.pos)];
        if (c.bsym_p1) cnt[c.bsym_p1 - 1] = imax(cnt[c.bsym_p1 - 1], (int)c.bval);
        if (c.lmask) {
#pragma unroll
            for (int k = 0; k < 8; k++) if (c.lmask & (1 << k)) cnt[UVC_LINK_M + k] = imax(cnt[UVC_LINK_M + k], (int)c.lval[k]);
        }
    }
}

DEV void frag_counts(const RegionDev &R, const UvcParams &P, const FragRec &f, int p, bool proton, int *cnt) {
#pragma unroll
    for (int s = 0; s < NSYM; s++) cnt[s] = 0;
    for (int k = f.aln_beg; k < f.aln_end; k++) aln_contrib_max(R, P, R.alns[k], p, proton, cnt);
}

// ------------------------------------------------------------------------------------------------
// per fragment: counts of covered and near-mutation positions (b10xSeqTlen / b10xSeqTNevents, main.hpp:2738-2756)
// ------------------------------------------------------------------------------------------------
// one wave per fragment: lanes classify positions (covered / mutated) into LDS, then count covered positions and those within
// +-syserr_mut_region_n_bases of a mutation (fragments with InDel reads, > 2 reads, primer gating, or > UVC_MAXEV events).
#define SWEEP_MAXSPAN 4096
__global__ void __launch_bounds__(64) k_fragstat_sweep(RegionDev R, UvcParams P, const int32_t *list, const int32_t *n_dev, int n_host) {
    __shared__ uint8_t flag[SWEEP_MAXSPAN];
    __shared__ int tot[2];
    const int lane = threadIdx.x;
    const int n = (n_dev ? *n_dev : n_host);
    const int nb = P.syserr_mut_region_n_bases;
    // spans beyond the LDS window are taken in chunks with a halo of nb positions either side (a mutation reaches nb positions far)
    const int step = SWEEP_MAXSPAN - 2 * nb;
    if (step < 64) { if (lane == 0 && blockIdx.x < n) atomicExch(R.err, UVCGPU_EUNSUPPORTED); return; }   // syserr_mut_region_n_bases beyond 2 000
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    // the list may be longer than the grid (the overflow form is launched before its length is known on the host): blocks stride over it
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
    const int fi = list[t];
    const FragRec &f = R.frags[fi];
    const int span = f.end - f.beg;
    __syncthreads();   // the previous fragment's totals have been read
    if (lane < 2) tot[lane] = 0;
    int cnt[NSYM];
    int n_cov = 0, n_near = 0;
    for (int c0 = 0; c0 < span; c0 += step) {
        const int w0 = imax(0, c0 - nb), w1 = imin(span, c0 + step + nb);
        __syncthreads();   // the previous chunk's flags have been read
        for (int i = w0 + lane; i < w1; i += 64) {
            const int p = f.beg + i;
            frag_counts(R, P, f, p, proton, cnt);
            int fl = 0;
            const int refsymbol = R.refsym[p - R.beg];
            for (int vi = 0; vi < 2; vi++) {
                const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
                int cs, cc, ct;
                fill_consensus(cnt, cs, cc, ct, st, st == UVC_LINK_SYMBOL, false);
                if (0 == ct) continue;
                fl |= 1;
                const int con_qual = cc * 2 - ct;
                const bool highBQ = (proton ? (UVC_BASE_SYMBOL == st || con_qual + 3 >= P.bias_thres_highBQ) : (UVC_LINK_SYMBOL == st || con_qual >= P.bias_thres_highBQ));
                if (symbols_mutated(refsymbol, cs) && highBQ) fl |= 2;
            }
            flag[i - w0] = (uint8_t)fl;
        }
        __syncthreads();
        for (int i = c0 + lane; i < imin(span, c0 + step); i += 64) {
            if (!(flag[i - w0] & 1)) continue;
            n_cov++;
            bool near = false;
            for (int j = imax(0, i - nb); j <= imin(span - 1, i + nb) && !near; j++) near = (flag[j - w0] & 2) != 0;
            if (near) n_near++;
        }
    }
    atomicAdd(&tot[0], n_cov); atomicAdd(&tot[1], n_near);
    __syncthreads();
    if (lane == 0) { R.frags[fi].n_cov = tot[0]; R.frags[fi].n_near = tot[1]; FragFast &ff = R.ffast[R.frag_rank[fi]]; ff.n_cov = tot[0]; ff.n_near = tot[1]; }
    }
}

// M runs and special range of one alignment for k_frag; false when it has more than one InDel or a reference skip
DEV bool aln_runs(const RegionDev &R, const AlnRec &a, int &pA, int &eA, int &qA, int &pB, int &eB, int &qB, int &sp_beg, int &sp_len) {
    const uint32_t *cigar = R.cigars + a.cigar_off;
    int rp = a.pos; long long qp = 0; int n_runs = 0, n_indel = 0;
    pA = eA = qA = pB = eB = qB = 0; sp_beg = a.pos; sp_len = 0;
    for (int i = 0; i < a.n_cigar; i++) {
        const int op = cig_op(cigar[i]), len = cig_len(cigar[i]);
        if (op == C_MATCH || op == C_EQUAL || op == C_DIFF) {
            const int qb = (int)((a.seq_off + qp - rp) & 0xFFFFFFFFLL);
            if (n_runs == 0) { pA = rp; eA = rp + len; qA = qb; } else if (n_runs == 1) { pB = rp; eB = rp + len; qB = qb; } else return false;
            n_runs++; rp += len; qp += len;
        } else if (op == C_INS) { if (++n_indel > 1) return false; sp_beg = rp; sp_len = 1; qp += len; }
        else if (op == C_DEL) { if (++n_indel > 1) return false; sp_beg = rp; sp_len = len + 1; rp += len; }
        else if (op == C_SOFT_CLIP) qp += len;
        else if (op == C_HARD_CLIP) {}
        else return false;
    }
    if (sp_beg + sp_len > a.rend + 1) sp_len = imax(0, a.rend + 1 - sp_beg);   // the last position that can carry a symbol is rend itself (insertion behind the last base)
    return n_runs >= 1 && sp_len < 32768;
}

// closed form for fragments of <= 2 simple alignments: coverage = union of the alignment spans, mutations = the event list
__global__ void __launch_bounds__(256) k_fragstat_fast(RegionDev R, UvcParams P) {
    const int fi = blockIdx.x * blockDim.x + threadIdx.x;
    if (fi >= R.n_frags) return;
    const FragRec f = R.frags[fi];
    FragFast ff;
    memset(&ff, 0, sizeof(ff));
    ff.beg = f.beg; ff.end = f.end; ff.fi = fi;
    ff.flags = (f.stat_kind != FRAG_STAT_EVENTS ? FF_GENERIC : 0) | (f.strand * FF_STRAND) | (f.singleton * FF_SINGLETON) | ((f.aln_end - f.aln_beg) << FF_NALN_SHIFT);
    ff.sq = (f.normMQ * f.normMQ) / SQR_QUAL_DIV;
    if (f.stat_kind != FRAG_STAT_EVENTS) {
        // fragments with InDel reads: k_frag can still take every position outside the InDels' neighbourhoods when the alignments
        // decompose into <= 2 M runs each (n_cov / n_near arrive from k_fragstat_sweep)
        const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
        const int n_aln = f.aln_end - f.aln_beg;
        bool ok = (!proton && !amplicon_gated(f.dflag, P) && n_aln <= 2 && f.end - f.beg < 65536 && f.stat_kind != FRAG_STAT_ZERO_VALUE);   // (a base of value 0: k_frag would count it)
        int sb, sl;
        if (ok) {
            const AlnRec &x0 = R.alns[f.aln_beg];
            ok = aln_runs(R, x0, ff.pos0, ff.rend0, ff.qb0, ff.bpos0, ff.brend0, ff.bqb0, sb, sl);
            ff.nogap0 = x0.nogap_penal; ff.sp0 = (sb - f.beg) | (sl << 16);
            if (sb < f.beg) ok = false;
        }
        if (ok && n_aln == 2) {
            const AlnRec &x1 = R.alns[f.aln_beg + 1];
            ok = aln_runs(R, x1, ff.pos1, ff.rend1, ff.qb1, ff.bpos1, ff.brend1, ff.bqb1, sb, sl);
            ff.nogap1 = x1.nogap_penal; ff.sp1 = (sb - f.beg) | (sl << 16);
            if (sb < f.beg) ok = false;
        }
        if (ok) ff.flags = (ff.flags & ~FF_GENERIC) | FF_RUNS_B;
        R.ffast[R.frag_rank[fi]] = ff; R.ffast_u[fi] = *(const FragUnit *)&ff; return;
    }
    const int nm = R.frag_nmut[fi];
    // coverage intervals [a1,b1) u [a2,b2), disjoint and ordered
    const AlnRec &x0 = R.alns[f.aln_beg];
    ff.pos0 = x0.pos; ff.rend0 = x0.rend; ff.qb0 = (int32_t)(x0.qbase & 0xFFFFFFFFLL); ff.nogap0 = x0.nogap_penal;
    int a1 = x0.pos, b1 = x0.rend, a2 = 0, b2 = 0;
    if (f.aln_end - f.aln_beg == 2) {
        const AlnRec &x1 = R.alns[f.aln_beg + 1];
        ff.pos1 = x1.pos; ff.rend1 = x1.rend; ff.qb1 = (int32_t)(x1.qbase & 0xFFFFFFFFLL); ff.nogap1 = x1.nogap_penal;
        int c = x1.pos, d = x1.rend;
        if (c < a1) { int t = a1; a1 = c; c = t; t = b1; b1 = d; d = t; }
        if (c <= b1) { b1 = imax(b1, d); } else { a2 = c; b2 = d; }
    }
    // k_frag_sums counts LINK_M by micro_nogap_penal class 1..5 (main.hpp:1882-1885 gives min(4, ..) + 1; below 1 only when NM is smaller than
    // the InDel lengths it should contain): anything else keeps the per-position form
    if (ff.nogap0 < 1 || ff.nogap0 > 5 || (f.aln_end - f.aln_beg == 2 && (ff.nogap1 < 1 || ff.nogap1 > 5))) ff.flags |= FF_LINK_PER_POS;
    const int n_cov = (b1 - a1) + (b2 - a2);
    int n_near = 0;
    if (nm > UVC_MAXEV) {   // too many events for the closed form: the sweep kernel (overflow pass) fills n_cov / n_near of this record
        const int k = atomicAdd(R.n_overflow, 1); R.overflow_frags[k] = fi;
        R.ffast[R.frag_rank[fi]] = ff; R.ffast_u[fi] = *(const FragUnit *)&ff; return;
    }
    if (nm > 0) {
        const int nb = P.syserr_mut_region_n_bases;
        int ev[UVC_MAXEV];
        for (int i = 0; i < nm; i++) ev[i] = R.frag_mut[(size_t)fi * UVC_MAXEV + i];
        for (int i = 1; i < nm; i++) { const int v = ev[i]; int j = i - 1; while (j >= 0 && ev[j] > v) { ev[j + 1] = ev[j]; j--; } ev[j + 1] = v; }
        int lo = ev[0] - nb, hi = ev[0] + nb + 1;   // merged dilation interval [lo, hi)
        for (int i = 1; i <= nm; i++) {
            if (i < nm && ev[i] - nb <= hi) { hi = ev[i] + nb + 1; continue; }
            n_near += imax(0, imin(hi, b1) - imax(lo, a1)) + imax(0, imin(hi, b2) - imax(lo, a2));
            if (i < nm) { lo = ev[i] - nb; hi = ev[i] + nb + 1; }
        }
    }
    R.frags[fi].n_cov = n_cov; R.frags[fi].n_near = n_near;
    ff.n_cov = n_cov; ff.n_near = n_near;
    R.ffast[R.frag_rank[fi]] = ff; R.ffast_u[fi] = *(const FragUnit *)&ff;
}

// ------------------------------------------------------------------------------------------------
// k_frag_sums: what the plain fragments add to LINK_M and to "a base is here" at every position, as interval sums.
// For a fragment of <= 2 simple alignments the LINK_M consensus at p is max(noindel80(p) - micro_nogap_penal, 0) + 1 of the better mate that
// has a link at p (main.hpp:1919-1923, 339-349): given the position it depends on the fragment through the penalty class only, and bDP / bTA /
// bTB / bMQ / the singleton votes are per-fragment constants.  One block per (tile of FSUM_TILE positions, strand): a lane per fragment adds
// +v at the begin and -v at the end of each of its <= 3 class pieces in LDS, a block-wide prefix sum turns the differences into sums.
// k_frag then spends nothing per (fragment, position) on LINK_M, and on the base side only what depends on the base and its quality.
// ------------------------------------------------------------------------------------------------
#define FSUM_TILE 1024
__global__ void __launch_bounds__(256) k_frag_sums(RegionDev R, UvcParams P) {
    __shared__ int d[UVC_FSUM_N][FSUM_TILE + 1];
    __shared__ int wtot[4];
    const int strand = blockIdx.y;
    const int t0 = R.beg + (int)blockIdx.x * FSUM_TILE, t1 = imin(t0 + FSUM_TILE, R.beg + (int)R.npos);
    for (int i = threadIdx.x; i < UVC_FSUM_N * (FSUM_TILE + 1); i += 256) (&d[0][0])[i] = 0;
    __syncthreads();
    // the fragments that can reach the tile, from the window index (k_win_index, lists 5 / 6): first with beg >= t0 - max_frag_span + 1 ..
    // first with beg >= the end of the tile's last 64-position window; two binary searches over the list by every thread (forty dependent
    // loads in front of the block's work) otherwise
    const int lo = win_lo(R, 5 + strand, (int)blockIdx.x * (FSUM_TILE / 64)), hi = win_hi(R, 5 + strand, (t1 - 1 - R.beg) >> 6);
    auto put = [&](int f, int a, int b, int v) { diff_put(d[f], t0, t1, a, b, v); };   // += v on [a, b) of plane f, clipped to the tile
    for (int k = lo + (int)threadIdx.x; k < hi; k += 256) {
        const int4 *q4 = (const int4 *)(R.ffast + k);
        const int4 h0 = q4[0]; const int flags = h0.w;   // beg, end, fi, flags (FF_W(flags) == 3: static_assert beside the struct)
        if ((flags & FF_NOT_IN_SUMS) || h0.y <= t0) continue;
        const int4 h1 = q4[1], h2 = q4[2], h3 = q4[3];   // pos0 rend0 pos1 rend1 | qb0 qb1 nogap0 nogap1 | sq n_cov n_near
        const bool has2 = (ff_naln(flags) == 2);
        const int sing = ((flags & FF_SINGLETON) ? 1 : 0), sq = h3.x, n_cov = h3.y, n_near = h3.z;
        // k_frag only looks at positions of [beg, end)
        const int a0 = imax(h1.x, h0.x), a1 = imin(h1.y, h0.y), b0 = (has2 ? imax(h1.z, h0.x) : 0), b1 = (has2 ? imin(h1.w, h0.y) : 0);
        {   // base side: the union of [a0, a1) and [b0, b1)
            auto base = [&](int a, int b) { put(UVC_FSUM_BDP, a, b, 1); put(UVC_FSUM_BTA, a, b, n_cov); put(UVC_FSUM_BTB, a, b, n_near); put(UVC_FSUM_BMQ, a, b, sq); };
            if (a0 < a1 && b0 < b1 && imax(a0, b0) <= imin(a1, b1)) base(imin(a0, b0), imax(a1, b1));
            else { if (a0 < a1) base(a0, a1); if (b0 < b1) base(b0, b1); }
        }
        {   // LINK_M exists from the second base of a run on: (pos, rend); the better (smaller) penalty wins where the mates overlap
            const int la0 = imax(h1.x + 1, h0.x), lb0 = (has2 ? imax(h1.z + 1, h0.x) : 0);
            const int ea = h2.z, eb = h2.w;
            auto link = [&](int a, int b, int e) {
                if (a >= b) return;
                put(UVC_FSUM_LCNT + e - 1, a, b, 1); put(UVC_FSUM_LTA, a, b, n_cov); put(UVC_FSUM_LTB, a, b, n_near); put(UVC_FSUM_LMQ, a, b, sq);
                if (sing) put(UVC_FSUM_LSING, a, b, 1);
            };
            const int o0 = imax(la0, lb0), o1 = imin(a1, b1);
            if (la0 < a1 && lb0 < b1 && o0 < o1) {
                link(imin(la0, lb0), o0, la0 < lb0 ? ea : eb);
                link(o0, o1, imin(ea, eb));
                link(o1, imax(a1, b1), a1 > b1 ? ea : eb);
            } else { link(la0, a1, ea); link(lb0, b1, eb); }
        }
    }
    __syncthreads();
    // prefix sums: four consecutive positions per thread, the block's 256 partial sums by wave scan + the waves' totals
    int32_t *out = R.fsum + (size_t)strand * UVC_FSUM_N * R.npos + (size_t)blockIdx.x * FSUM_TILE;
    const int n_here = t1 - t0;
#pragma unroll 1
    for (int f = 0; f < UVC_FSUM_N; f++) {   // (one body for all planes)
        int v[4];
        const int before = block_excl<4>(diff_run<4>(d[f], v), wtot);
        __syncthreads();   // wtot is written again in the next round
        int32_t *o4 = out + (size_t)f * R.npos + threadIdx.x * 4;
        if (threadIdx.x * 4 + 4 <= n_here && (((uintptr_t)o4) & 15) == 0) *(int4 *)o4 = make_int4(before + v[0], before + v[1], before + v[2], before + v[3]);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++) { const int x = threadIdx.x * 4 + i; if (x < n_here) o4[i] = before + v[i]; }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_frag_generic: the P3 / singleton P4-P5 contribution of the fragments k_frag cannot take in registers (InDel reads,
// more than two alignments, primer-gated reads; every fragment on IonTorrent).  One wave per fragment, lanes over its
// positions, everything added to the planes with atomics; the bucket histogram goes to the global bucket plane, which
// k_frag merges in P3b.  Runs before k_frag.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_frag_generic(RegionDev R, UvcParams P, const int32_t *list, int n_list) {
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const bool padded_ignored = (P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0;
    const bool vcfgen = P.inferred_is_vcf_generated;
    // grid = (fragments, 64-position chunks of the longest fragment): the work of a fragment is a chain of dependent loads per
    // position, so more, shorter waves hide it better than one wave striding over the whole span
    for (int t = blockIdx.x; t < n_list; t += gridDim.x) {
        const int fi = (list ? list[t] : t);
        const FragRec &f = R.frags[fi];
        const int strand = f.strand;
        const bool singleton = f.singleton;
        const int fsq = (f.normMQ * f.normMQ) / SQR_QUAL_DIV;
        const FragFast &ff = R.ffast[R.frag_rank[fi]];
        const bool special_only = (ff.flags & FF_RUNS_B) != 0;   // k_frag takes every other position of this fragment
        const int sp0 = ff.sp0, sp1 = ff.sp1;
        const int n0 = (special_only ? (sp0 >> 16) : 0), n1 = (special_only ? (sp1 >> 16) : 0);
        const int p_lo = imax(f.beg, R.beg), p_hi = imin(f.end, R.end);
        const int n_work = (special_only ? n0 + n1 : p_hi - p_lo);
        for (int w = (int)(blockIdx.y * 64 + threadIdx.x); w < n_work; w += 64 * gridDim.y) {
            int p;
            if (!special_only) p = p_lo + w;
            else {
                p = (w < n0 ? f.beg + (sp0 & 0xFFFF) + w : f.beg + (sp1 & 0xFFFF) + (w - n0));
                // a position in both ranges is done once, by the first
                if (w >= n0 && (unsigned)(p - (f.beg + (sp0 & 0xFFFF))) < (unsigned)n0) continue;
                if (p < p_lo || p >= p_hi) continue;
            }
            const int64_t x = p - R.beg;
            const int my_ref = R.refsym[x];
            int cnt[NSYM];
            frag_counts(R, P, f, p, proton, cnt);
            for (int vi = 0; vi < 2; vi++) {
                const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
                int cs, cc, ct;
                fill_consensus(cnt, cs, cc, ct, st, st == UVC_LINK_SYMBOL, false);
                if (0 == ct) continue;
                int cs4 = cs, cc4 = cc, ct4 = ct;
                if (st == UVC_BASE_SYMBOL && padded_ignored) fill_consensus(cnt, cs4, cc4, ct4, st, false, true);
                if (vcfgen) {
                    const int ad = S32(R, UVC_S_aDPff, cs, x) + S32(R, UVC_S_aDPfr, cs, x) + S32(R, UVC_S_aDPrf, cs, x) + S32(R, UVC_S_aDPrr, cs, x);
                    const int max_qual = 8 + BQS(R, cs, x) / imax(1, ad);   // get_avgBQ, main_conversion.hpp:791-796
                    int phredlike = imin(cc * 2 - ct, max_qual);
                    if (0x1 & P.fam_flag) phredlike = imin(phredlike, sscs_phred(P, my_ref, cs));
                    const int pbucket = imax(0, max_qual - phredlike);
                    if (pbucket < NBUCKETS) atomicAdd(&BKP(R, 0, cs, pbucket, x), 1);
                    mark_sym(R, cs, x);
                    atomicAdd(&FRP(R, strand, UVC_FRAG_bDP, cs, x), 1); atomicAdd(&FRP(R, strand, UVC_FRAG_bTA, cs, x), f.n_cov); atomicAdd(&FRP(R, strand, UVC_FRAG_bTB, cs, x), f.n_near);
                    atomicAdd(&VQP(R, UVC_VQ_bMQ, cs, x), fsq);
                }
                if (singleton) {   // con / mmm identities of a one-fragment unit (main.hpp:466-520)
                    const int adj = imax(cc4 * 2, ct4) - ct4;
                    const int thr = (st == UVC_BASE_SYMBOL ? P.fam_thres_highBQ_snv : 0);
                    if (adj >= thr && adj > 0) { mark_sym(R, cs4, x); atomicAdd(&FAP(R, strand, UVC_FAM_cDP12, cs4, x), 1); atomicAdd(&FAP(R, strand, UVC_FAM_cDP21, cs4, x), 1); }
                    const int adj5 = imax(cc * 2, ct) - ct;
                    if (adj5 > 0 && vcfgen) { mark_sym(R, cs, x); atomicAdd(&FAP(R, strand, UVC_FAM_cDP1, cs, x), 1); }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_frag: P3 + P3b for every fragment, and P4/P5 of singleton family-strand units.  One lane per
// position; per-lane bucket histograms of the two dense symbols live in LDS, rare symbols use the
// global bucket plane (each position has exactly one writer in this kernel).
// ------------------------------------------------------------------------------------------------
// PLAIN: VCF run, Illumina-like values, no SSCS table cap (fam_flag & 1), padded deletions counted: the common case without those arms
// H16: no position is covered by 65 536 fragments or more (host bound, RegionDev::max_frag_depth), so two buckets share one LDS word:
// 16 KiB per block instead of 32, six waves per SIMD instead of five.
#define RQ_CAP 128   // events per wave between two flushes (one record adds at most 64)
// SPLIT (see k_prep_fast): a block per window.  The four waves take every fourth chunk of the window's fragments and add into ONE set of LDS
// columns (bucket histogram, lacc, racc: a column per position, LDS atomics); behind the lists wave 0 alone holds the sums and runs the rest.
template <bool PLAIN, bool H16, bool SPLIT = false>
DEV void frag_body(const RegionDev &R, const UvcParams &P, unsigned (*hist)[NBUCKETS / (H16 ? 2 : 1)][SPLIT ? 64 : 256], unsigned long long (*rq)[RQ_CAP], int (*lacc)[SPLIT ? 64 : 256], int (*racc)[64] = nullptr) {
    const int col = (SPLIT ? (int)(threadIdx.x & 63) : (int)threadIdx.x);   // this thread's column of the LDS arrays
    auto hist_add = [&](int dense, int b) {   // ds_add_u32 without return
        if (H16) atomicAdd(&hist[dense][b >> 1][col], 1u << (16 * (b & 1))); else atomicAdd(&hist[dense][b][col], 1u);
    };
    auto hist_get = [&](int dense, int b) -> int {
        return H16 ? (int)((hist[dense][b >> 1][col] >> (16 * (b & 1))) & 0xFFFFu) : (int)hist[dense][b][col];
    };
    COARSE_T(ct0)
    const int lane = threadIdx.x & 63;
    const int wave = SPLIT ? wave_uniform((int)xcd_block()) : wave_uniform((int)((xcd_block() * blockDim.x + threadIdx.x) >> 6));
    const int wv = (int)(threadIdx.x >> 6);
    const int64_t x0 = (int64_t)wave * 64;
    if (x0 >= R.npos) return;
    const int w0 = R.beg + (int)x0;
    const int p = w0 + lane;
    const int64_t x = x0 + lane;
    const bool valid = x < R.npos;
    const bool proton = (PLAIN ? false : (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform));
    const bool padded_ignored = (PLAIN ? false : ((P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0));
    const bool vcfgen = (PLAIN ? true : (P.inferred_is_vcf_generated != 0));   // P3 belongs to updateByAlns3UsingBQ, skipped on FASTQ-only runs (main.hpp:3691)
    const int my_ref = valid ? R.refsym[x] : 0;
    if (!SPLIT || wv == 0) {
        for (int b = 0; b < NBUCKETS / (H16 ? 2 : 1); b++) { hist[0][b][col] = 0; hist[1][b][col] = 0; }
        for (int i = 0; i < (SPLIT ? 10 : 5); i++) lacc[i][col] = 0;
        if (SPLIT) for (int i = 0; i < 11; i++) racc[i][col] = 0;
    }
    if (SPLIT) __syncthreads();   // (block-uniform: the four waves share the window)
    // avgBQ + 8 (get_avgBQ, main_conversion.hpp:791-796) of the five read symbols and of LINK_M; LINK_M value of a simple read here
    auto maxq_at = [&](int sym) {
        const int ad = S32(R, UVC_S_aDPff, sym, x) + S32(R, UVC_S_aDPfr, sym, x) + S32(R, UVC_S_aDPrf, sym, x) + S32(R, UVC_S_aDPrr, sym, x);
        return 8 + BQS(R, sym, x) / imax(1, ad);
    };
    // the five per-symbol values are packed 16 bits each (a value is 8 + an average base quality) so that the per-lane lookup by
    // consensus symbol is a shift, not an indexed local array (which would live in scratch memory)
    unsigned long long mq_acgt = 0x0008000800080008ull;
    int mqN = 8, maxq_link = 8, noindel80 = 80;
    if (valid) {
        // (signed: the sum of the values, and with it the average, is below 0 where a negative bq_phred_added_misma outweighs the qualities;
        // 8 + a quality byte + an addend that uvcgpu_params_check keeps within -256 .. 3840 fits 16 signed bits, so the clamp never acts)
        auto h16 = [&](int sym) { return (unsigned long long)(unsigned short)imax(imin(maxq_at(sym), 32767), -32768); };
        mq_acgt = h16(UVC_BASE_A) | (h16(UVC_BASE_C) << 16) | (h16(UVC_BASE_G) << 32) | (h16(UVC_BASE_T) << 48);
        mqN = maxq_at(UVC_BASE_N);
        maxq_link = maxq_at(UVC_LINK_M);
        if (x > 0) noindel80 = imin(80, imin(RTRP(R, UVC_RTR_indelphred, x - 1), RTRP(R, UVC_RTR_indelphred, x)));
    }
    auto maxq_base = [&](int cs) { return cs >= UVC_BASE_N ? mqN : (int)(short)(mq_acgt >> (16 * cs)); };   // cs in A..N
    // dense accumulators of the reference symbol: [strand] x {bDP, bTA, bTB, cDP12 (== cDP21), cDP1}, bMQ.  Named structs, selected by
    // a wave-uniform branch on the strand: runtime-indexed local arrays would live in scratch memory (one VMEM round trip per update).
    struct DAcc { int bDP, bTA, bTB, c12, c1; };
    DAcc a_fr = {0,0,0,0,0}, a_rr = {0,0,0,0,0};   // {fwd,rev} of the reference symbol (LINK_M: interval sums + lacc, see the end)
    int bMQ_r = 0;
    // One (fragment, position, symbol type) consensus (cs = symbol, cc = its value, ct = total) -> P3 outputs and, for singleton units,
    // the P4/P5 identities:
    //   con = 1 vote for the fragment consensus when 2*max - tot passes the threshold (main.hpp:466-495) => cDP12, cDP21 (tot_count == 1)
    //   mmm = 2*max - tot when positive (main.hpp:497-520)                                              => cDP1
    // The reference symbol accumulates in registers / LDS.  Every other symbol is rare and becomes an EVENT in the wave's LDS queue:
    // the loop itself issues no store or atomic to memory, so the s_waitcnt vmcnt(0) in front of the next record's prefetched bytes
    // waits for those bytes only (with the atomics in the loop it waited for every one of them to reach the L2: two thirds of
    // the kernel's wave-cycles, SQ_WAIT_ANY).  flush_events turns the queue into fire-and-forget atomics, a lane per event.
    //   event: bit 63 valid | fragment index k << 24 | p3 << 23 | c12 << 22 | c1 << 21 | strand << 20 | bucket (31 = none) << 14 | cs4 << 10 | cs << 6 | lane
    unsigned long long *myq = rq[threadIdx.x >> 6];
    int nq = 0;   // wave-uniform: only updated in uniform control flow
    auto flush_events = [&]() {
#ifdef UVC_ABLATE_RARE
        nq = 0; return;
#endif
        for (int i = lane; i < nq; i += 64) {
            const unsigned long long e = myq[i];
            const int le = (int)(e & 63), cs = (int)((e >> 6) & 15), cs4 = (int)((e >> 10) & 15), pb = (int)((e >> 14) & 31), st = (int)((e >> 20) & 1);
            const int64_t xe = x0 + le;
            const FragFast *ff = R.ffast + (int)((e >> 24) & 0x7FFFFFFFull);
            // The cells of a position belong to its wave in this kernel: the adds need to be atomic among the lanes of this flush only, so
            // they are L2 atomics of workgroup scope.  (Agent scope sends each one to the memory side and makes the fence below a write-back +
            // invalidate of the XCD's whole L2 -- per wave, 15 000 times per launch: it was what kept every load of the kernel slow.)
            auto add_own = [](int32_t *cell, int v) { __hip_atomic_fetch_add(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
            const int sq = ff->sq, n_cov = ff->n_cov, n_near = ff->n_near;
            mark_sym(R, cs, xe); mark_sym(R, cs4, xe);
            if ((e >> 23) & 1) {
                if (pb < NBUCKETS) add_own(&BKP(R, 0, cs, pb, xe), 1);
                add_own(&FRP(R, st, UVC_FRAG_bDP, cs, xe), 1); add_own(&FRP(R, st, UVC_FRAG_bTA, cs, xe), n_cov); add_own(&FRP(R, st, UVC_FRAG_bTB, cs, xe), n_near);
                add_own(&VQP(R, UVC_VQ_bMQ, cs, xe), sq);
            }
            if ((e >> 22) & 1) { add_own(&FAP(R, st, UVC_FAM_cDP12, cs4, xe), 1); add_own(&FAP(R, st, UVC_FAM_cDP21, cs4, xe), 1); }
            if ((e >> 21) & 1) add_own(&FAP(R, st, UVC_FAM_cDP1, cs, xe), 1);
        }
        nq = 0;
    };
    // FULL: the fragment is not in k_frag_sums' interval sums, its per-fragment constants are added here.  Otherwise the sums hold them for
    // every position with a base, as if the base were the reference: a rare symbol takes its share back out of the reference's accumulators.
    // K(FF_W(field)): a field of the fragment's record.  Returns the event of a rare symbol, or 0.
    auto apply = [&](bool full, DAcc &ar, int cs, int cc, int ct, int cs4, int cc4, int ct4, int max_qual, int strand, auto K, bool singleton, int k) -> unsigned long long {
        const bool is_ref = (cs == my_ref);
        int pb = 31;
        if (vcfgen) {
            const int con_qual = cc * 2 - ct;
            int phredlike = imin(con_qual, max_qual);
            if (!PLAIN && (0x1 & P.fam_flag)) phredlike = imin(phredlike, sscs_phred(P, my_ref, cs));
            const int pbucket = imax(0, max_qual - phredlike);
            if (is_ref) {
                if (pbucket < NBUCKETS) hist_add(0, pbucket);
                if (full) { ar.bDP += 1; ar.bTA += K(FF_W(n_cov)); ar.bTB += K(FF_W(n_near)); bMQ_r += K(FF_W(sq)); }
            } else {
                pb = imin(pbucket, 31);
                if (!full) { ar.bDP -= 1; ar.bTA -= K(FF_W(n_cov)); ar.bTB -= K(FF_W(n_near)); bMQ_r -= K(FF_W(sq)); }
            }
        }
        // (conditions as values, increments as adds of 0 / 1: a nest of per-lane ifs is an exec-mask level each -- save, branch, restore -- per record)
        const int adj = imax(cc4 * 2, ct4) - ct4;
        const bool v12 = singleton & (adj >= P.fam_thres_highBQ_snv) & (adj > 0);   // cDP12 == cDP21 for a singleton unit
        const bool r4 = (cs4 == my_ref);
        ar.c12 += ((v12 & r4) ? 1 : 0);
        const bool e12 = v12 & !r4;
        const int adj5 = imax(cc * 2, ct) - ct;
        const bool v1 = singleton & (adj5 > 0) & vcfgen;
        ar.c1 += ((v1 & is_ref) ? 1 : 0);
        const bool e1 = v1 & !is_ref;
        const bool e3 = (vcfgen && !is_ref);
        if (!(e3 || e12 || e1)) return 0ull;
        return (1ull << 63) | ((unsigned long long)(unsigned)k << 24) | ((unsigned long long)e3 << 23) | ((unsigned long long)e12 << 22) | ((unsigned long long)e1 << 21)
             | ((unsigned long long)strand << 20) | ((unsigned long long)pb << 14) | ((unsigned long long)(cs4 & 15) << 10) | ((unsigned long long)(cs & 15) << 6) | (unsigned long long)lane;
    };
    // LINK_M of a fragment outside the interval sums (few): value lv > 0 at this position, its consensus is a vote (threshold 0) and an mmm > 0.
    // Bucket and sums in LDS (lacc: bDP, bTA, bTB, bMQ, singleton votes of the strand being walked; moved to the planes after each list).
    auto link_full = [&](int lv, int strand, auto K, bool singleton) {
        if (vcfgen) {
            int phredlike = imin(lv, maxq_link);
            if (!PLAIN && (0x1 & P.fam_flag)) phredlike = imin(phredlike, sscs_phred(P, my_ref, UVC_LINK_M));
            const int pbucket = imax(0, maxq_link - phredlike);
            if (pbucket < NBUCKETS) hist_add(1, pbucket);
            const int lr = (SPLIT ? 5 * strand : 0);
            atomicAdd(&lacc[lr + 0][col], 1); atomicAdd(&lacc[lr + 1][col], K(FF_W(n_cov))); atomicAdd(&lacc[lr + 2][col], K(FF_W(n_near))); atomicAdd(&lacc[lr + 3][col], K(FF_W(sq)));
        }
        if (singleton) atomicAdd(&lacc[(SPLIT ? 5 * strand : 0) + 4][col], 1);
    };
    auto maxq_generic = [&](int cs) { return cs == UVC_LINK_M ? maxq_link : (cs <= UVC_BASE_N ? maxq_base(cs) : maxq_at(cs)); };
    const __amdgpu_buffer_rsrc_t rs = bq_rsrc(R);
    auto run_list = [&](auto ST, DAcc &ar) {
    constexpr int strand = decltype(ST)::value ? 1 : 0;
    const int lo = wave_uniform(win_lo(R, 5 + strand, (int)(x0 >> 6))), hi = wave_uniform(win_hi(R, 5 + strand, (int)(x0 >> 6)));
    for (int k0 = lo + (SPLIT ? 64 * wv : 0); k0 < hi; k0 += (SPLIT ? 256 : 64)) {
        // one FragFast (24 dwords) per lane, fields of record j broadcast with v_readlane; base/qual bytes of record j+1 are
        // requested before record j is processed
        int c[24];
        load_words(R.ffast + (k0 + lane), k0 + lane < hi, c);
        const int n = imin(64, hi - k0);
        int bq0n = 0, bq1n = 0;
        int n_fl = 0, n_fend = 0;   // of the record whose bytes are on their way: read once, used by its iteration too
        auto issue = [&](int j) {
            const int fl = n_fl = bcast(c[FF_W(flags)], j);
            n_fend = bcast(c[FF_W(end)], j);
            // the list holds every fragment that could reach the window (begin within the longest span): four in ten end in front of it,
            // and a fragment of the generic kind is not read here at all -- no bytes for those
            if (n_fend <= w0 || (fl & FF_GENERIC)) return;
            int i0 = bcast(c[FF_W(qb0)], j), i1 = bcast(c[FF_W(qb1)], j);
            if (fl & FF_RUNS_B) {   // the lane's position may lie in run B of either alignment
                if (p >= bcast(c[FF_W(bpos0)], j) && p < bcast(c[FF_W(brend0)], j)) i0 = bcast(c[FF_W(bqb0)], j);
                if (p >= bcast(c[FF_W(bpos1)], j) && p < bcast(c[FF_W(brend1)], j)) i1 = bcast(c[FF_W(bqb1)], j);
            }
            bq0n = bq_load(rs, i0 + p);
            if (ff_naln(fl) == 2) bq1n = bq_load(rs, i1 + p);
        };
        if (proton) break;   // IonTorrent values need neighbouring qualities: every fragment takes k_frag_generic
        issue(0);
        for (int j = 0; j < n; j++) {
            const int bq0 = bq0n, bq1 = bq1n;
            const int flags = n_fl, fend = n_fend;
            if (j + 1 < n) issue(j + 1);
            if (fend <= w0) continue;
            const int fbeg = bcast(c[FF_W(beg)], j);
            if (flags & FF_GENERIC) continue;   // done by k_frag_generic
            // from here on the control flow stays wave-uniform down to the queue bookkeeping (nq is a scalar): per-lane conditions are predicates
            bool cover = (valid && p >= fbeg && p < fend);
            const bool singleton = (flags & FF_SINGLETON) != 0;
            auto K = [&](int i) { return bcast(c[i], j); };
            // consensus of <= 2 alignments in registers (pair_consensus, link_better_mate)
            const int pos0 = bcast(c[FF_W(pos0)], j), rend0 = bcast(c[FF_W(rend0)], j), pos1 = bcast(c[FF_W(pos1)], j), rend1 = bcast(c[FF_W(rend1)], j);
            const bool has2 = (ff_naln(flags) == 2);
            bool in0 = (p >= pos0 && p < rend0), in1 = (has2 && p >= pos1 && p < rend1);
            const bool full = (flags & FF_FULL) != 0;   // wave-uniform: not in k_frag_sums
            if (full) {
                const int nogap0 = bcast(c[FF_W(nogap0)], j), nogap1 = bcast(c[FF_W(nogap1)], j);
                bool lk0 = (in0 && p > pos0), lk1 = (in1 && p > pos1);   // LINK_M exists from the second base of a run on
                if (flags & FF_RUNS_B) {
                    const int bpos0 = bcast(c[FF_W(bpos0)], j), brend0 = bcast(c[FF_W(brend0)], j), bpos1 = bcast(c[FF_W(bpos1)], j), brend1 = bcast(c[FF_W(brend1)], j);
                    const int sp0 = bcast(c[FF_W(sp0)], j), sp1 = bcast(c[FF_W(sp1)], j);
                    const bool inb0 = (p >= bpos0 && p < brend0), inb1 = (p >= bpos1 && p < brend1);
                    in0 = in0 || inb0; in1 = in1 || inb1;
                    lk0 = lk0 || (inb0 && p > bpos0); lk1 = lk1 || (inb1 && p > bpos1);
                    // positions next to an InDel carry InDel symbols / padded-deletion symbols: k_frag_generic does them for this fragment
                    const unsigned off = (unsigned)(p - fbeg);
                    if (off - (unsigned)(sp0 & 0xFFFF) < (unsigned)(sp0 >> 16) || off - (unsigned)(sp1 & 0xFFFF) < (unsigned)(sp1 >> 16)) cover = false;
                }
                const int lv = link_better_mate(lk0, lk1, noindel80, nogap0, nogap1);
                if (cover && lv > 0) link_full(lv, strand, K, singleton);
            }
            unsigned long long ev = 0ull;
            if (cover && (in0 || in1)) {
                const PairCons pc = pair_consensus(in0, in1, bq0, bq1, P, padded_ignored);
                const int mq = maxq_base(pc.cs);
                ev = apply(full, ar, pc.cs, pc.cc, pc.ct, pc.cs4, pc.cc4, pc.ct4, mq, strand, K, singleton, k0 + j);
            }
            const wmask mm = BAL(ev != 0ull);
            if (mm) {
                if (nq > RQ_CAP - 64) flush_events();
                if (ev != 0ull) myq[nq + (int)__builtin_popcountll(mm & ((1ull << lane) - 1ull))] = ev;
                nq += (int)__builtin_popcountll(mm);
            }
        }
    }
    };
    COARSE_T(ct1)
    // LINK_M sums of the fragments outside the interval sums, strand by strand: plain read-modify-write (these cells are this lane's)
    auto lacc_out = [&](int strand) {
        const int lr = (SPLIT ? 5 * strand : 0);
        const int n = lacc[lr + 0][col], ta = lacc[lr + 1][col], tb = lacc[lr + 2][col], mq = lacc[lr + 3][col], sg = lacc[lr + 4][col];
        if (valid && (n | sg)) {
            const int v0 = FRP(R, strand, UVC_FRAG_bDP, UVC_LINK_M, x), v1 = FRP(R, strand, UVC_FRAG_bTA, UVC_LINK_M, x), v2 = FRP(R, strand, UVC_FRAG_bTB, UVC_LINK_M, x);
            const int v3 = VQP(R, UVC_VQ_bMQ, UVC_LINK_M, x), v4 = FAP(R, strand, UVC_FAM_cDP12, UVC_LINK_M, x), v5 = FAP(R, strand, UVC_FAM_cDP21, UVC_LINK_M, x), v6 = FAP(R, strand, UVC_FAM_cDP1, UVC_LINK_M, x);
            if (n) { FRP(R, strand, UVC_FRAG_bDP, UVC_LINK_M, x) = v0 + n; FRP(R, strand, UVC_FRAG_bTA, UVC_LINK_M, x) = v1 + ta; FRP(R, strand, UVC_FRAG_bTB, UVC_LINK_M, x) = v2 + tb; VQP(R, UVC_VQ_bMQ, UVC_LINK_M, x) = v3 + mq; }
            if (sg) { FAP(R, strand, UVC_FAM_cDP12, UVC_LINK_M, x) = v4 + sg; FAP(R, strand, UVC_FAM_cDP21, UVC_LINK_M, x) = v5 + sg; if (vcfgen) FAP(R, strand, UVC_FAM_cDP1, UVC_LINK_M, x) = v6 + sg; }
        }
        if (!SPLIT) { for (int i = 0; i < 5; i++) lacc[i][col] = 0; }
    };
    run_list(std::false_type{}, a_fr);
    if (!SPLIT) lacc_out(0);
    run_list(std::true_type{}, a_rr);
    if (!SPLIT) lacc_out(1);
    if (nq > 0) flush_events();
    if (SPLIT) {
        // the partial sums of the four waves -> racc; every wave's adds to the planes must have reached the L2 before wave 0 reads them back
        const int part[11] = { a_fr.bDP, a_fr.bTA, a_fr.bTB, a_fr.c12, a_fr.c1, a_rr.bDP, a_rr.bTA, a_rr.bTB, a_rr.c12, a_rr.c1, bMQ_r };
#pragma unroll
        for (int i = 0; i < 11; i++) if (part[i]) atomicAdd(&racc[i][col], part[i]);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __syncthreads();
        if (wv != 0) return;
        a_fr.bDP = racc[0][col]; a_fr.bTA = racc[1][col]; a_fr.bTB = racc[2][col]; a_fr.c12 = racc[3][col]; a_fr.c1 = racc[4][col];
        a_rr.bDP = racc[5][col]; a_rr.bTA = racc[6][col]; a_rr.bTB = racc[7][col]; a_rr.c12 = racc[8][col]; a_rr.c1 = racc[9][col]; bMQ_r = racc[10][col];
        lacc_out(0); lacc_out(1);
    }
    COARSE_T(ct2)
    if (!valid) return;
    // the adds above must have reached the L2 before the planes are read back (they pass through this CU's L1, which drops its copy of the line)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    COARSE_T(ce0)
    // the interval sums of the plain fragments (k_frag_sums): LINK_M by penalty class into the bucket histogram, the rest into the accumulators
    DAcc a_fl = {0,0,0,0,0}, a_rl = {0,0,0,0,0};
    int bMQ_l = 0;
    asm volatile("" ::: "memory");
    if (!proton) {
        int lcnt[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int32_t *S = R.fsum + (size_t)s * UVC_FSUM_N * R.npos + x;
            DAcc &ar = (s ? a_rr : a_fr), &al = (s ? a_rl : a_fl);
            const int sing = S[(size_t)UVC_FSUM_LSING * R.npos];
            al.c12 += sing;   // a LINK_M consensus is a vote of its own value > 0: cDP12 / cDP21, and cDP1 with P3
            if (vcfgen) {
                int n = 0;
#pragma unroll
                for (int e = 0; e < 5; e++) { const int c = S[(size_t)(UVC_FSUM_LCNT + e) * R.npos]; lcnt[e] += c; n += c; }
                al.bDP += n; al.bTA += S[(size_t)UVC_FSUM_LTA * R.npos]; al.bTB += S[(size_t)UVC_FSUM_LTB * R.npos]; bMQ_l += S[(size_t)UVC_FSUM_LMQ * R.npos];
                al.c1 += sing;
                ar.bDP += S[(size_t)UVC_FSUM_BDP * R.npos]; ar.bTA += S[(size_t)UVC_FSUM_BTA * R.npos]; ar.bTB += S[(size_t)UVC_FSUM_BTB * R.npos]; bMQ_r += S[(size_t)UVC_FSUM_BMQ * R.npos];
            }
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int e = 0; e < 5; e++) {
            if (lcnt[e] == 0) continue;
            const int lv = imax(noindel80 - (e + 1), 0) + 1;
            int phredlike = imin(lv, maxq_link);
            if (!PLAIN && (0x1 & P.fam_flag)) phredlike = imin(phredlike, sscs_phred(P, my_ref, UVC_LINK_M));
            const int b = imax(0, maxq_link - phredlike);
            if (b < NBUCKETS) { if (H16) hist[1][b >> 1][col] += (unsigned)lcnt[e] << (16 * (b & 1)); else hist[1][b][col] += (unsigned)lcnt[e]; }
        }
    }
    // ---- the rest reads and writes this position's planes.  A read-modify-write per counter, one after the other, costs a memory round
    // trip each (measured with s_memtime: a quarter of a wave's life went here): every stage below issues all of its loads, then computes,
    // then stores.  Nobody else touches these cells in this kernel and the atomics above have landed.
    const bool has_generic = (R.n_sweep > 0 || proton);
    // (1) fragment depth of every symbol with the dense accumulators folded in; which symbols are present
    int totDP_b = 0, totDP_l = 0; unsigned present = 0;
#define STAGE_FENCE asm volatile("" ::: "memory");   // keeps the compiler from hoisting the next stage's loads into this one (registers: no scratch here)
    auto depth_stage = [&](auto LINKS) {
        constexpr int sb = decltype(LINKS)::value ? UVC_LINK_M : UVC_BASE_A, se = decltype(LINKS)::value ? UVC_LINK_NN : UVC_BASE_NN;
        int f0[se - sb + 1], f1[se - sb + 1];
#pragma unroll
        for (int s = sb; s <= se; s++) { f0[s - sb] = FRP(R, 0, UVC_FRAG_bDP, s, x); f1[s - sb] = FRP(R, 1, UVC_FRAG_bDP, s, x); }
#pragma unroll
        for (int s = sb; s <= se; s++) {
            int d0 = 0, d1 = 0;
            if (s <= UVC_BASE_NN && s == my_ref) { d0 = a_fr.bDP; d1 = a_rr.bDP; }
            if (s == UVC_LINK_M) { d0 = a_fl.bDP; d1 = a_rl.bDP; }
            if (d0) FRP(R, 0, UVC_FRAG_bDP, s, x) = f0[s - sb] + d0;
            if (d1) FRP(R, 1, UVC_FRAG_bDP, s, x) = f1[s - sb] + d1;
            const int nfr = f0[s - sb] + f1[s - sb] + d0 + d1;
            if (s <= UVC_BASE_NN) totDP_b += nfr; else totDP_l += nfr;
            if (nfr) present |= 1u << s;
        }
    };
    STAGE_FENCE
    depth_stage(std::false_type{});
    STAGE_FENCE
    depth_stage(std::true_type{});
    STAGE_FENCE
    COARSE_T(ce1)
    // (2) the other dense accumulators, one (symbol, strand) at a time: five loads, five stores
    auto flush5 = [&](const DAcc &a, int t, int sym) {
        if (!(a.bTA | a.bTB | a.c12 | a.c1)) return;
        const int v0 = FRP(R, t, UVC_FRAG_bTA, sym, x), v1 = FRP(R, t, UVC_FRAG_bTB, sym, x);
        const int v2 = FAP(R, t, UVC_FAM_cDP12, sym, x), v3 = FAP(R, t, UVC_FAM_cDP21, sym, x), v4 = FAP(R, t, UVC_FAM_cDP1, sym, x);
        if (a.bTA) FRP(R, t, UVC_FRAG_bTA, sym, x) = v0 + a.bTA;
        if (a.bTB) FRP(R, t, UVC_FRAG_bTB, sym, x) = v1 + a.bTB;
        if (a.c12) { FAP(R, t, UVC_FAM_cDP12, sym, x) = v2 + a.c12; FAP(R, t, UVC_FAM_cDP21, sym, x) = v3 + a.c12; }
        if (a.c1) FAP(R, t, UVC_FAM_cDP1, sym, x) = v4 + a.c1;
    };
    flush5(a_fr, 0, my_ref); STAGE_FENCE
    flush5(a_rr, 1, my_ref); STAGE_FENCE
    flush5(a_fl, 0, UVC_LINK_M); STAGE_FENCE
    flush5(a_rl, 1, UVC_LINK_M); STAGE_FENCE
    if (bMQ_r | bMQ_l) {
        const int q0 = VQP(R, UVC_VQ_bMQ, my_ref, x), q1 = VQP(R, UVC_VQ_bMQ, UVC_LINK_M, x);
        if (bMQ_r) VQP(R, UVC_VQ_bMQ, my_ref, x) = q0 + bMQ_r;
        if (bMQ_l) VQP(R, UVC_VQ_bMQ, UVC_LINK_M, x) = q1 + bMQ_l;
    }
    STAGE_FENCE
    COARSE_T(ce2)
    // (3) P3b (main.hpp:2801-2828): one pass per symbol that some lane of the wave has; its 16 buckets and three outputs in one batch of loads
    if (vcfgen) {
        unsigned long long todo = 0;   // wave-uniform set of symbols
#pragma unroll
        for (int s = 0; s < NSYM; s++) if (BAL((present >> s) & 1u)) todo |= 1ull << s;
        while (todo) {
            const int s = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            if (!((present >> s) & 1u)) continue;   // empty histogram -> all three outputs are 0
            const int dense = (s == my_ref ? 0 : (s == UVC_LINK_M ? 1 : -1));
            const bool global_b = (dense < 0 || has_generic);   // the global buckets hold the rare symbols and everything k_frag_generic added
            int h[NBUCKETS];
#pragma unroll
            for (int b = 0; b < NBUCKETS; b++) h[b] = (global_b ? BKP(R, 0, s, b, x) : 0);
            const int o0 = VQP(R, UVC_VQ_bIAQb, s, x), o1 = VQP(R, UVC_VQ_bIADb, s, x), o2 = VQP(R, UVC_VQ_bIDQb, s, x);
            const int max_qual = maxq_generic(s);
            if (global_b) {
#pragma unroll
                for (int b = 0; b < NBUCKETS; b++) if (h[b]) BKP(R, 0, s, b, x) = 0;   // clearSymbolBucketCount, main.hpp:2827
            }
            if (dense >= 0) {
#pragma unroll
                for (int b = 0; b < NBUCKETS; b++) h[b] += hist_get(dense, b);
            }
            int mv, ad2, bq2;
            infer_max_qual_regs(mv, ad2, bq2, max_qual, (s <= UVC_BASE_NN ? totDP_b : totDP_l), h);
            if (mv | ad2 | bq2) { VQP(R, UVC_VQ_bIAQb, s, x) = o0 + mv; VQP(R, UVC_VQ_bIADb, s, x) = o1 + ad2; VQP(R, UVC_VQ_bIDQb, s, x) = o2 + bq2; }
            STAGE_FENCE
        }
    }
#ifdef UVC_FRAG_COARSE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    COARSE_T(ct3)
    if (lane == 0 && (wave % 1499) == 7) printf("coarse wave %d prologue %llu lists %llu epilogue %llu = fence %llu sums+depth %llu flush %llu p3b %llu\n", wave, ct1 - ct0, ct2 - ct1, ct3 - ct2, ce0 - ct2, ce1 - ce0, ce2 - ce1, ct3 - ce2);
#endif
}

template <bool PLAIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5,5))) k_frag(RegionDev R, UvcParams P) {
    __shared__ unsigned hist[2][NBUCKETS][256];   // [dense symbol][bucket][thread]: conflict-free
    __shared__ unsigned long long rq[4][RQ_CAP];
    __shared__ int lacc[5][256];
    frag_body<PLAIN, false>(R, P, hist, rq, lacc);
}
template <bool PLAIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5,6))) k_frag16_split(RegionDev R, UvcParams P) {
    __shared__ unsigned hist[2][NBUCKETS / 2][64];
    __shared__ unsigned long long rq[4][RQ_CAP];
    __shared__ int lacc[10][64];
    __shared__ int racc[11][64];
    frag_body<PLAIN, true, true>(R, P, hist, rq, lacc, racc);
}
template <bool PLAIN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6,6))) k_frag16(RegionDev R, UvcParams P) {
    __shared__ unsigned hist[2][NBUCKETS / 2][256];   // 16 + 4 + 5 KiB: six blocks share a CU
    __shared__ unsigned long long rq[4][RQ_CAP];
    __shared__ int lacc[5][256];
    frag_body<PLAIN, true>(R, P, hist, rq, lacc);
}

// ------------------------------------------------------------------------------------------------
// generic family-strand units (more than one fragment, or UMI / duplex): one thread per (unit, position)
// ------------------------------------------------------------------------------------------------
// indel_len of the FAM2 position-bias test (main.hpp:3236-3246) for an insertion consensus: the number of fragments of the unit that carry
// the majority inserted sequence.  While the unit has no more insertion votes than microadjust_nobias_pos_indel_maxlen the value cannot
// matter (non_neg_minus gives 0 either way); above it the exact count comes from the allele pipeline (k_gap_alleles), found by the
// (family, position) key of the sorted candidates.
DEV int fam2_ins_len(const RegionDev &R, const UvcParams &P, const FsRec &u, int p, int votes) {
    if (votes <= P.microadjust_nobias_pos_indel_maxlen || R.gap.n_ev <= 0) return votes;
    const unsigned long long key = ((unsigned long long)u.fam << 26) | (unsigned long long)(p - R.beg);
    int lo = 0, hi = R.gap.n_ev;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (R.gap.ckey_s[m] < key) lo = m + 1; else hi = m; }
    if (lo >= R.gap.n_ev || R.gap.ckey_s[lo] != key) return votes;   // cannot happen: an insertion vote comes from an insertion event
    return R.gap.maj[2 * lo + u.strand];
}
DEV int find_unit(const RegionDev &R, int64_t w) {   // last generic unit with work_off <= w
    int lo = 0, hi = R.n_generic_fs;
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (R.fss[R.generic_fs[mid]].work_off <= w) lo = mid; else hi = mid; }
    return R.generic_fs[lo];
}

// builds con (votes) and optionally mmm (major-minus-minor BQ sums) of one unit at position p
// HAS_MMM selects the second output.  Fragments of <= 2 simple alignments (the FragFast record k_frag uses) are evaluated with the same
// select-based consensus as in k_frag; the others go through the per-alignment contribution path.
template <bool HAS_MMM, class Arr>
DEV void unit_counts(const RegionDev &R, const UvcParams &P, const FsRec &u, int p, bool proton, Arr con, Arr mmm) {
    const bool padded_ignored = (P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0;
    for (int s = 0; s < NSYM; s++) { con[s] = 0; if (HAS_MMM) mmm[s] = 0; }
    const int64_t x = p - R.beg;
    const int noindel80 = (x > 0 ? imin(80, imin(RTRP(R, UVC_RTR_indelphred, x - 1), RTRP(R, UVC_RTR_indelphred, x))) : 80);
    const __amdgpu_buffer_rsrc_t rs = bq_rsrc(R);
    int cnt[NSYM];
    for (int fi = u.frag_beg; fi < u.frag_end; fi++) {
        const FragFast &ff = R.ffast[R.frag_rank[fi]];
        const int fbeg = ff.beg, fend = ff.end, flags = ff.flags;
        if (p < fbeg || p >= fend) continue;
        if ((flags & FF_NOT_REGISTER) == 0 && !proton) {
            // register path (see k_frag): link_better_mate, pair_consensus
            const int pos0 = ff.pos0, rend0 = ff.rend0, pos1 = ff.pos1, rend1 = ff.rend1;
            const bool has2 = (ff_naln(flags) == 2);
            const bool in0 = (p >= pos0 && p < rend0), in1 = (has2 && p >= pos1 && p < rend1);
            const int lv = link_better_mate(in0 && p > pos0, in1 && p > pos1, noindel80, ff.nogap0, ff.nogap1);
            if (lv > 0) { con[UVC_LINK_M] += 1; if (HAS_MMM) mmm[UVC_LINK_M] += lv; }   // one symbol: 2*max - tot = lv, threshold 0 (main.hpp:466-520)
            if (in0 || in1) {
                const int bq0 = (in0 ? bq_load(rs, ff.qb0 + p) : 0), bq1 = (in1 ? bq_load(rs, ff.qb1 + p) : 0);
                const PairCons pc = pair_consensus(in0, in1, bq0, bq1, P, padded_ignored);
                const int adj = imax(pc.cc4 * 2, pc.ct4) - pc.ct4;
                if (adj >= P.fam_thres_highBQ_snv && adj > 0) con[pc.cs4] += 1;
                if (HAS_MMM) { const int adj5 = imax(pc.cc * 2, pc.ct) - pc.ct; if (adj5 > 0) mmm[pc.cs] += adj5; }
            }
            continue;
        }
        const FragRec &f = R.frags[fi];
        frag_counts(R, P, f, p, proton, cnt);
        for (int st = 0; st < 2; st++) {
            int cs, cc, ct;
            if (st == UVC_LINK_SYMBOL) fill_consensus(cnt, cs, cc, ct, st, true, false);
            else fill_consensus(cnt, cs, cc, ct, st, false, padded_ignored);
            const int adj = imax(cc * 2, ct) - ct;
            if (adj >= (st == UVC_BASE_SYMBOL ? P.fam_thres_highBQ_snv : 0) && adj > 0) con[cs] += 1;
            if (HAS_MMM) {
                if (st == UVC_BASE_SYMBOL && padded_ignored) fill_consensus(cnt, cs, cc, ct, st, false, false);
                const int adj5 = imax(cc * 2, ct) - ct;
                if (adj5 > 0) mmm[cs] += adj5;
            }
        }
    }
}

// per-unit scalars: medians of read ends "as filled" (main.hpp:2916-2940) and the no-strict-bias window (:2959-2998)
__global__ void __launch_bounds__(64) k_fam_stat(RegionDev R, UvcParams P) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R.n_generic_fs) return;
    const int ui = R.generic_fs[t];
    FsRec u = R.fss[ui];
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    int n_l2r = 0, n_r2l = 0, qsum = 0, nq = 0;
    const int a_beg = R.frags[u.frag_beg].aln_beg, a_end = R.frags[u.frag_end - 1].aln_end;
    for (int k = a_beg; k < a_end; k++) { const AlnRec &a = R.alns[k]; if (a.flag & 0x10) n_r2l++; else n_l2r++; qsum += a.l_qseq; nq++; }
    auto nth = [&](bool rev, int idx) -> int {
        int c = 0;
        for (int k = a_beg; k < a_end; k++) { const AlnRec &a = R.alns[k]; if (((a.flag & 0x10) != 0) == rev) { if (c == idx) return rev ? a.pos : a.rend; c++; } }
        return 0;
    };
    u.l2r_end_median = (n_l2r > 0 ? (nth(false, (n_l2r - 1) / 2) + nth(false, n_l2r / 2)) / 2 : u.end);
    u.r2l_end_median = (n_r2l > 0 ? (nth(true, (n_r2l - 1) / 2) + nth(true, n_r2l / 2)) / 2 : u.beg);
    int nsb_min = u.end, nsb_max = u.beg;
    const int nfrags = u.frag_end - u.frag_beg;
    // the scan can only succeed for UMI families (or fam_flag & 0x2): is_fam_good needs it (main.hpp:2988-2989)
    if ((nfrags >= P.fam_thres_dup1add) && (qsum >= nq * P.fam_thres_qseqlen) && unit_may_be_good(u.dflag, P)) {
        int con[NSYM];
        for (int dir = 0; dir < 2; dir++) {
            int b = (dir ? (u.end - 1) : u.beg), e = (dir ? (u.beg - 1) : u.end), step = (dir ? -1 : 1);
            for (int p = b; p != e; p += step) {
                unit_counts<false>(R, P, u, p, proton, con, con);
                int cs, cc, ct;
                fill_consensus(con, cs, cc, ct, UVC_BASE_SYMBOL, false, false);
                if (0 == ct) continue;
                const bool good = is_fam_good(cc, ct, u.dflag, P);
                if (good && (UVC_BASE_N != cs) && (UVC_BASE_NN != cs)) { if (dir) nsb_max = p; else nsb_min = p; break; }
            }
        }
    }
    u.nsb_min = nsb_min; u.nsb_max = nsb_max;
    // k_fam_p4d leaves the (unit, position) cells under a fragment of the general kind (InDel reads, > 2 alignments) to k_fam_p4d_rest
    int has_general = (proton ? 1 : 0);
    for (int f = u.frag_beg; f < u.frag_end && !has_general; f++) if (R.ffast_u[f].flags & FF_NOT_REGISTER) has_general = 1;
    u.pad_ = has_general;
    R.fss[ui] = u;
}

// The increments of the family passes.  FamAcc collects them: a window kernel (a32 set) adds those of its two dense symbols (reference
// base, LINK_M) in LDS and writes them once per position (fam_flush); without LDS accumulators every increment is a global atomic.
#define FAMW_SLOTS (2 * UVC_NFAM + UVC_NFAMINFO32)   // [strand][FAM field], then the FamFormatInfoSet i32 fields
struct FamAcc {
    int (*a32)[FAMW_SLOTS][64]; unsigned long long (*a64)[UVC_NFAMINFO64][64]; int (*bk)[2][NBUCKETS][64];
    const RegionDev *R; int64_t x; int lane, my_ref;
    DEV static FamAcc global(const RegionDev &R, int64_t x) { FamAcc A; A.a32 = nullptr; A.a64 = nullptr; A.bk = nullptr; A.R = &R; A.x = x; A.lane = 0; A.my_ref = -1; return A; }
    DEV int dense(int cs) const { return !a32 ? -1 : (cs == my_ref ? 0 : (cs == UVC_LINK_M ? 1 : -1)); }
    // a window kernel (a32 set) owns its positions: its adds to the planes are L2 atomics of workgroup scope (add_own)
    DEV void gadd(int32_t *p, int v) const { if (a32) add_own(p, v); else atomicAdd(p, v); }
    // the marks of a symbol's cells outside the dense paths (fam_flush marks those), once per (unit, position, symbol) before its increments:
    // mark for the FAM / bucket planes and the occupancy, fi_mark for the FamFormatInfoSet planes
    DEV void mark(int cs) const { if (dense(cs) < 0) mark_sym(*R, cs, x); }
    DEV void fi_mark(int cs) const { if (dense(cs) < 0) mark_fi(*R, cs, x); }
    DEV void fap(int strand, int f, int cs, int v) const { const int d = dense(cs); if (d >= 0) atomicAdd(&a32[d][strand * UVC_NFAM + f][lane], v); else gadd(&FAP(*R, strand, f, cs, x), v); }
    DEV void fi(int f, int cs, int v) const { const int d = dense(cs); if (d >= 0) atomicAdd(&a32[d][2 * UVC_NFAM + f][lane], v); else gadd(&FIP(*R, f, cs, x), v); }
    DEV void fi64(int f, int cs, long long v) const { const int d = dense(cs); if (d >= 0) atomicAdd(&a64[d][f][lane], (unsigned long long)v); else if (a32) add64_own(&FI64P(*R, f, cs, x), v); else add64(&FI64P(*R, f, cs, x), v); }
    DEV void bucket(int strand, int cs, int b) const { const int d = dense(cs); if (d >= 0) atomicAdd(&bk[d][strand][b][lane], 1); else gadd(&BKP(*R, strand, cs, b, x), 1); R->p5flag[(size_t)strand * R->npos + x] = 1; }
};

// what p4_apply reads of the position alone (thresholds, BAQ prefix sums): a window kernel loads it once per lane, not once per unit
struct P4Pos { int LPxT, RPxT, LP1t, LP2t, RP1t, RP2t; long long baq1, baq2;
               const long long *lb1, *lb2; int lb_lo; };   // k_fam_p4d: the two BAQ prefix-sum arrays of [lb_lo, lb_lo + P4_BAQ_WIN) staged in LDS
#define P4_BAQ_WIN (64 + 2 * MAX_STR_N_BASES + 2)   // every BAQ index of a window's cells lies within MAX_STR_N_BASES of the window
DEV P4Pos p4_pos(const RegionDev &R, int p) {
    const int64_t x = p - R.beg;
    P4Pos Q;
    Q.LPxT = TH(R, UVC_T_aLPxT, x); Q.RPxT = TH(R, UVC_T_aRPxT, x); Q.LP1t = TH(R, UVC_T_aLP1t, x); Q.LP2t = TH(R, UVC_T_aLP2t, x); Q.RP1t = TH(R, UVC_T_aRP1t, x); Q.RP2t = TH(R, UVC_T_aRP2t, x);
    Q.baq1 = BAQ1(R, p); Q.baq2 = BAQ2(R, p);
    Q.lb1 = nullptr; Q.lb2 = nullptr; Q.lb_lo = 0;
    return Q;
}

// The P4 increments of one (unit, position, symbol type) once the vote consensus (cs = symbol, cc = its votes, ct = all votes of the type) is
// known (main.hpp:2999-3355; consensus FASTQ left out).  Qw: the position's values with the window's BAQ prefix sums in LDS (k_fam_p4d), or
// NULL: loaded here, for the cells that reach the bias tests only.
DEV void p4_apply(const FamAcc &A, const RegionDev &R, const UvcParams &P, const FsRec &u, int p, int64_t x, int st, int cs, int cc, int ct, const P4Pos *Qw) {
    const int strand = u.strand;
    const bool fam_good = is_fam_good(cc, ct, u.dflag, P);
    A.mark(cs);
    A.fap(strand, UVC_FAM_cDP12, cs, 1);
    if (1 == ct) A.fap(strand, UVC_FAM_cDP21, cs, 1);
    if (!P.inferred_is_vcf_generated) return;
    if (fam_good) {
        A.fi_mark(cs);
        A.fap(strand, UVC_FAM_cDP2, cs, 1);
        int rbeg = imin(u.nsb_min, p), rend = imax(u.nsb_max, p);
        const bool nonconf_middle = (u.l2r_end_median <= (u.r2l_end_median + P.indel_adj_tracklen_dist));
        if (nonconf_middle && p < u.r2l_end_median) rend = imax(imin(u.l2r_end_median, imin(u.r2l_end_median, rend)), p);
        if (nonconf_middle && u.l2r_end_median < p) rbeg = imin(imax(u.l2r_end_median, imax(u.r2l_end_median, rbeg)), p);
        const bool isGap = (UVC_LINK_SYMBOL == st);
        const int bq = 90, dist = 1024 * 1024;
        if (((!isGap) && bq >= P.bias_thres_highBQ) || (isGap && dist >= P.bias_thres_highBQ)) {
            const bool tier2 = (isGap || bq >= P.bias_thres_highBQ);
            const P4Pos Q = (Qw ? *Qw : p4_pos(R, p));
            auto baq1_at = [&](long long a) -> long long { if (Qw) return Q.lb1[(int)a - Q.lb_lo]; return BAQ1(R, a); };
            auto baq2_at = [&](long long a) -> long long { if (Qw) return Q.lb2[(int)a - Q.lb_lo]; return BAQ2(R, a); };
            const int l_nb = (int)nnminus(p + 1, rbeg), r_nb = (int)nnminus(rend, p);
            const int LPxT = (isGap ? Q.LPxT : imin(Q.LPxT, Q.RPxT));
            // indel_len = majority COUNT of one inserted sequence among the unit's fragments (main.hpp:3239-3243): see fam2_ins_len
            const int indel_len = (is_ins(cs) ? fam2_ins_len(R, P, u, p, cc) : 0);   // cc = con[cs] of the vote consensus (a deletion's count is never read: main.hpp:3245)
            const bool far = (l_nb + (is_ins(cs) ? (int)nnminus(indel_len, P.microadjust_nobias_pos_indel_maxlen) : 0) >= LPxT) && (r_nb >= Q.RPxT);
            if (far) {
                int LP1 = 0, LP2 = 0, RP1 = 0, RP2 = 0; long long LPL = 0, RPL = 0;
                bidir(LP1, LP2, RP1, RP2, LPL, RPL, Q.LP1t, Q.LP2t, Q.RP1t, Q.RP2t, l_nb, r_nb, true, 0);
                if (LP1) A.fi(UVC_FI_c2LP1, cs, LP1);
                if (LP2) A.fi(UVC_FI_c2LP2, cs, LP2);
                if (RP1) A.fi(UVC_FI_c2RP1, cs, RP1);
                if (RP2) A.fi(UVC_FI_c2RP2, cs, RP2);
                A.fi(UVC_FI_c2LPL, cs, (int)LPL); A.fi(UVC_FI_c2RPL, cs, (int)RPL);
            }
            if ((int)nnminus(p + 1, u.nsb_min) >= P.bias_thres_strict_c2LRP0) A.fi(UVC_FI_c2LP0, cs, 1);
            if ((int)nnminus(u.nsb_max, p) >= P.bias_thres_strict_c2LRP0) A.fi(UVC_FI_c2RP0, cs, 1);
            const long long baq_last = R.end - 1;
            const int seg_l_baq = (int)(Q.baq1 - baq1_at(lmax((long long)rbeg, nnminus(p, MAX_STR_N_BASES))) + 1);
            const long long rr = lmin((long long)rend - 1, lmin((long long)p + MAX_STR_N_BASES, baq_last));
            const int _seg_r_baq = (int)(baq1_at(rr) - Q.baq1 + 1);
            const int seg_r_baq = (isGap ? (int)lmin((long long)_seg_r_baq, baq2_at(rr) - Q.baq2 + 7) : _seg_r_baq);
            const int thres_highBAQ = P.bias_thres_highBAQ + (isGap ? 0 : 3);
            if (seg_l_baq >= thres_highBAQ && seg_r_baq >= thres_highBAQ) {
                int LB1 = 0, LB2 = 0, RB1 = 0, RB2 = 0; long long LBL = 0, RBL = 0;
                bidir(LB1, LB2, RB1, RB2, LBL, RBL, P.bias_thres_BAQ1, P.bias_thres_BAQ2, P.bias_thres_BAQ1, P.bias_thres_BAQ2, seg_l_baq, seg_r_baq, tier2, 0);
                if (LB1) A.fi(UVC_FI_c2LB1, cs, LB1);
                if (LB2) A.fi(UVC_FI_c2LB2, cs, LB2);
                if (RB1) A.fi(UVC_FI_c2RB1, cs, RB1);
                if (RB2) A.fi(UVC_FI_c2RB2, cs, RB2);
                A.fi64(UVC_FI64_c2LBL, cs, LBL); A.fi64(UVC_FI64_c2RBL, cs, RBL);
            }
            A.fi(UVC_FI_c2BQ2, cs, 1);
        }
    }
    if (P.fam_thres_dup2add <= ct && (cc * 100 >= ct * P.fam_thres_dup2perc)) A.fap(strand, UVC_FAM_cDP3, cs, 1);
    const int flat = (is_subst(cs) ? P.fam_thres_emperr_all_flat_snv : P.fam_thres_emperr_all_flat_indel);
    const int perc = (is_subst(cs) ? P.fam_thres_emperr_con_perc_snv : P.fam_thres_emperr_con_perc_indel);
    if (ct < flat) return;
    if (cc * 100 < ct * perc) return;
    const int sb = (st == 0 ? UVC_BASE_A : UVC_LINK_M), se = (st == 0 ? UVC_BASE_NN : UVC_LINK_NN);
    const int m = ct - cc, M = ct * (se - sb);   // sum over the other symbols of the type of (their votes, all votes)
    if (m) A.fap(strand, UVC_FAM_cDPm, cs, m);
    A.fap(strand, UVC_FAM_cDPM, cs, M);
}

// ---- p4_apply for the cells whose consensus symbol is one of the window kernel's two dense symbols (nearly all of them) ----
// p4_apply spends its time in the control flow around its ~20 conditional increments (exec-mask bookkeeping, the dense / rare select of every
// FamAcc call): 2.35 of k_fam_p4d's 5.4 ms on a 200 kb x 2000x tile.  Here every condition is a 0 / 1 value and every increment an
// unconditional LDS add of a value that may be 0, and what depends on (unit, position) only -- the two distances, the BAQ differences, the
// position-bias flags -- is computed once for the cell's LINK and BASE consensus (P4Cell) instead of once per symbol type.  Same sums.
struct P4Cell { int good_unit, l_nb, r_nb, lp1, lp2, rp1, rp2, lp0, rp0, seg_l_baq, seg_r_base, seg_r_gap; };
DEV void p4_cell(P4Cell &W, const RegionDev &R, const UvcParams &P, const FsRec &u, int p, const P4Pos &Q) {
    W.good_unit = (unit_may_be_good(u.dflag, P) ? 1 : 0);
    int rbeg = imin(u.nsb_min, p), rend = imax(u.nsb_max, p);
    const bool nonconf_middle = (u.l2r_end_median <= (u.r2l_end_median + P.indel_adj_tracklen_dist));
    if (nonconf_middle && p < u.r2l_end_median) rend = imax(imin(u.l2r_end_median, imin(u.r2l_end_median, rend)), p);
    if (nonconf_middle && u.l2r_end_median < p) rbeg = imin(imax(u.l2r_end_median, imax(u.r2l_end_median, rbeg)), p);
    W.l_nb = (int)nnminus(p + 1, rbeg); W.r_nb = (int)nnminus(rend, p);
    // update_bidirectional_bias with tier2 = true, n_indel = 0 (bidir above)
    W.lp1 = (W.l_nb >= Q.LP1t); W.lp2 = (W.l_nb >= Q.LP2t); W.rp1 = (W.r_nb >= Q.RP1t); W.rp2 = (W.r_nb >= Q.RP2t);
    W.lp0 = ((int)nnminus(p + 1, u.nsb_min) >= P.bias_thres_strict_c2LRP0); W.rp0 = ((int)nnminus(u.nsb_max, p) >= P.bias_thres_strict_c2LRP0);
    const long long baq_last = R.end - 1;
    W.seg_l_baq = (int)(Q.baq1 - Q.lb1[(int)lmax((long long)rbeg, nnminus(p, MAX_STR_N_BASES)) - Q.lb_lo] + 1);
    const int rr = (int)lmin((long long)rend - 1, lmin((long long)p + MAX_STR_N_BASES, baq_last)) - Q.lb_lo;
    W.seg_r_base = (int)(Q.lb1[rr] - Q.baq1 + 1);
    W.seg_r_gap = (int)lmin((long long)W.seg_r_base, Q.lb2[rr] - Q.baq2 + 7);
}
// d = FamAcc::dense(cs) >= 0; GAP = the LINK symbol type (cs == LINK_M, never an insertion: indel_len = 0)
template <bool GAP>
DEV void p4_apply_dense(const FamAcc &A, int d, const UvcParams &P, const FsRec &u, int cc, int ct, const P4Pos &Q, const P4Cell &W) {
    int *b32 = &A.a32[d][0][A.lane];
    unsigned long long *b64 = &A.a64[d][0][A.lane];
#define P4ADD_FAP(f, v) atomicAdd(b32 + (u.strand * UVC_NFAM + (f)) * 64, (v))
#define P4ADD_FI(f, v) atomicAdd(b32 + (2 * UVC_NFAM + (f)) * 64, (v))
    P4ADD_FAP(UVC_FAM_cDP12, 1);
    P4ADD_FAP(UVC_FAM_cDP21, (1 == ct) ? 1 : 0);
    if (!P.inferred_is_vcf_generated) return;   // (uniform)
    const int good = ((P.fam_thres_dup1add <= ct) && (cc * 100 >= ct * P.fam_thres_dup1perc) && W.good_unit) ? 1 : 0;
    P4ADD_FAP(UVC_FAM_cDP2, good);
    const int bq = 90, dist = 1024 * 1024;
    if (GAP ? (dist >= P.bias_thres_highBQ) : (bq >= P.bias_thres_highBQ)) {   // (uniform; then tier2 is true for both types)
        const int LPxT = (GAP ? Q.LPxT : imin(Q.LPxT, Q.RPxT));
        const int gf = (good && (W.l_nb >= LPxT) && (W.r_nb >= Q.RPxT)) ? 1 : 0;
        P4ADD_FI(UVC_FI_c2LP1, gf & W.lp1); P4ADD_FI(UVC_FI_c2LP2, gf & W.lp2); P4ADD_FI(UVC_FI_c2RP1, gf & W.rp1); P4ADD_FI(UVC_FI_c2RP2, gf & W.rp2);
        P4ADD_FI(UVC_FI_c2LPL, gf ? W.l_nb : 0); P4ADD_FI(UVC_FI_c2RPL, gf ? W.r_nb : 0);
        P4ADD_FI(UVC_FI_c2LP0, good & W.lp0); P4ADD_FI(UVC_FI_c2RP0, good & W.rp0);
        const int seg_r_baq = (GAP ? W.seg_r_gap : W.seg_r_base);
        const int thres_highBAQ = P.bias_thres_highBAQ + (GAP ? 0 : 3);
        const int gb = (good && W.seg_l_baq >= thres_highBAQ && seg_r_baq >= thres_highBAQ) ? 1 : 0;
        P4ADD_FI(UVC_FI_c2LB1, gb & (W.seg_l_baq >= P.bias_thres_BAQ1 ? 1 : 0)); P4ADD_FI(UVC_FI_c2LB2, gb & (W.seg_l_baq >= P.bias_thres_BAQ2 ? 1 : 0));
        P4ADD_FI(UVC_FI_c2RB1, gb & (seg_r_baq >= P.bias_thres_BAQ1 ? 1 : 0)); P4ADD_FI(UVC_FI_c2RB2, gb & (seg_r_baq >= P.bias_thres_BAQ2 ? 1 : 0));
        atomicAdd(b64 + UVC_FI64_c2LBL * 64, (unsigned long long)(long long)(gb ? W.seg_l_baq : 0));
        atomicAdd(b64 + UVC_FI64_c2RBL * 64, (unsigned long long)(long long)(gb ? seg_r_baq : 0));
        P4ADD_FI(UVC_FI_c2BQ2, good);
    }
    P4ADD_FAP(UVC_FAM_cDP3, ((P.fam_thres_dup2add <= ct) && (cc * 100 >= ct * P.fam_thres_dup2perc)) ? 1 : 0);
    const int flat = (GAP ? P.fam_thres_emperr_all_flat_indel : P.fam_thres_emperr_all_flat_snv);
    const int perc = (GAP ? P.fam_thres_emperr_con_perc_indel : P.fam_thres_emperr_con_perc_snv);
    const bool e = (ct >= flat) && (cc * 100 >= ct * perc);
    P4ADD_FAP(UVC_FAM_cDPm, e ? ct - cc : 0);
    P4ADD_FAP(UVC_FAM_cDPM, e ? ct * (GAP ? (UVC_LINK_NN - UVC_LINK_M) : (UVC_BASE_NN - UVC_BASE_A)) : 0);
#undef P4ADD_FAP
#undef P4ADD_FI
}

// P4 of generic units, the generic form: one thread per (unit, position), every increment a global atomic
__global__ void __launch_bounds__(256) k_fam_p4(RegionDev R, UvcParams P) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= R.n_generic_work) return;
    const FsRec u = R.fss[find_unit(R, w)];
    const int p = u.beg + (int)(w - u.work_off);
    const int64_t x = p - R.beg;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    __shared__ int con_s[NSYM][256];
    const LdsCounts<256> con = { &con_s[0][threadIdx.x] };
    unit_counts<false>(R, P, u, p, proton, con, con);
    const FamAcc A = FamAcc::global(R, x);
    for (int vi = 0; vi < 2; vi++) {
        const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
        int cs, cc, ct;
        fill_consensus(con, cs, cc, ct, st, false, false);
        if (0 != ct) p4_apply(A, R, P, u, p, x, st, cs, cc, ct, nullptr);
    }
}

// The BQ-sum consensus of one symbol type at a (unit, position), with the votes of its symbol and of the whole type: what P5 reads
struct P5Cons { int cs, con_nfrags, tot_nfrags, con_sumBQs, tot_sumBQs; };
template <class Arr>
DEV P5Cons p5_cons(const Arr &con, const Arr &mmm, int st) {
    P5Cons c;
    fill_consensus(mmm, c.cs, c.con_sumBQs, c.tot_sumBQs, st, false, false);
    c.con_nfrags = con[c.cs];
    c.tot_nfrags = 0;
    const int sb = (st == 0 ? UVC_BASE_A : UVC_LINK_M), se = (st == 0 ? UVC_BASE_NN : UVC_LINK_NN);
    for (int s = sb; s <= se; s++) c.tot_nfrags += con[s];
    return c;
}

// The empirical family quality of P5 (main.hpp:3472-3488): confam_qual of the consensus c (symbol type st) of a unit on `strand` at x, and the
// average BQ it starts from.  majorcount / minorcount are complete: P4 ran before.
// realphred = -10 log10(prob) enters through round(k * realphred) and round(realphred) only.  Given p2p (an LDS table of phred2prob for the
// average qualities 0..127, see k_fam_p5d), a single-precision evaluation (error of realphred < 1e-5) decides both roundings unless a product
// lies within its error bound of a half: only then (one wave iteration in ten) the fp64 expression of the reference is evaluated, which a
// caller without the table always takes.  Two fp64 divisions and a log per cell and symbol type were most of k_fam_p5d.
DEV double phred2prob(int phred) { return pow(10.0, (double)(-((float)phred) / 10)); }   // phred2prob's float cast, main_conversion.hpp:885-888
DEV double phred2prob_tab(const double *p2p, int avgBQ) { return (p2p && (unsigned)avgBQ < 128u) ? p2p[avgBQ] : phred2prob(avgBQ); }
DEV int fam_qual(const RegionDev &R, const UvcParams &P, int strand, int64_t x, int st, const P5Cons &c, const double *p2p, int &avgBQ) {
    avgBQ = ((0 == c.tot_nfrags) ? 1 : (c.con_sumBQs / c.tot_nfrags));
    const int majorcount = FAP(R, strand, UVC_FAM_cDPM, c.cs, x), minorcount = FAP(R, strand, UVC_FAM_cDPm, c.cs, x);
    const int kfr = (c.con_nfrags * 2) - c.tot_nfrags;
    int indep_frag_phred = 0, round_realphred = 0;
    bool safe = false;
    if (p2p) {
        const float wf = __builtin_amdgcn_rcpf((float)minorcount + 1.0f);
        const float p2pf = ((unsigned)avgBQ < 128u) ? (float)p2p[avgBQ] : 0.0f;
        const float probf = ((float)minorcount + wf) * __builtin_amdgcn_rcpf((float)majorcount + (float)minorcount + wf * __builtin_amdgcn_rcpf(p2pf));
        const float rf = -3.0102999566f * __builtin_amdgcn_logf(probf);   // v_log_f32 is log2
        const float v1 = (float)kfr * rf;
        const float tol1 = 5.0e-4f + 4.0e-5f * fabsf((float)kfr) + 1.0e-6f * fabsf(v1), tol0 = 5.0e-4f;
        safe = ((unsigned)avgBQ < 128u) && (majorcount + minorcount < (1 << 22)) && rf > 0.0f && rf < 1000.0f
               && fabsf(v1 - floorf(v1) - 0.5f) > tol1 && fabsf(rf - floorf(rf) - 0.5f) > tol0;
        if (safe) { indep_frag_phred = (int)roundf(v1); round_realphred = (int)roundf(rf); }
    }
    if (!safe) {
        const double prior_weight = 1.0 / (minorcount + 1.0);
        const double p2pd = phred2prob_tab(p2p, avgBQ);
        const double prob = (minorcount + prior_weight) / (majorcount + minorcount + prior_weight / p2pd);
        const double realphred = -10 * log(prob) / log(10.0);
        indep_frag_phred = (int)round(kfr * realphred); round_realphred = (int)round(realphred);
    }
    if (UVC_LINK_SYMBOL == st) return imax(1, imin(indep_frag_phred, P.fam_phred_indel_inc_before_barcode_labeling + round_realphred));
    return imax(1, imin(indep_frag_phred, (c.con_sumBQs * 2) - c.tot_sumBQs));
}

// The P5 increments of one (unit, position, symbol type) (main.hpp:3392-3513): cDP1, cDPD and the quality bucket of the consensus c
DEV void p5_apply(const FamAcc &A, const RegionDev &R, const UvcParams &P, const FsRec &u, int64_t x, int st, const P5Cons &c, const double *p2p) {
    if (0 == c.tot_sumBQs) return;
    const int strand = u.strand;
    const bool is_duplex_fam = ((u.dflag & UVC_DFLAG_DUPLEX) != 0);
    const bool other_present = (u.other_fs >= 0);
    const bool will_inc_dscs = is_duplex_fam && other_present;
    const bool will_inc_sscs = is_duplex_fam && !other_present;
    A.mark(c.cs);
    A.fap(strand, UVC_FAM_cDP1, c.cs, 1);
    if (will_inc_sscs && (!will_inc_dscs) && (c.tot_nfrags >= P.fam_thres_dup1add) && (c.con_nfrags * 100 >= c.tot_nfrags * P.fam_thres_dup1perc))
        A.fap(strand, UVC_FAM_cDPD, c.cs, 1);
    int avgBQ;
    const int confam_qual = fam_qual(R, P, strand, x, st, c, p2p, avgBQ);
    const int max_qual = sscs_phred(P, R.refsym[x], c.cs) + (!P.tumor_vcf_is_provided ? 0 : 4);
    const int confam_qual2 = imin(confam_qual, max_qual);
    if (c.tot_nfrags >= P.fam_thres_dup1add) {
        const int pbucket = (max_qual - confam_qual2 + 2) / 4;
        if (pbucket >= 0 && pbucket < NBUCKETS) A.bucket(strand, c.cs, pbucket);
    }
}

// P5 of generic units, the generic form (main.hpp:3392-3513)
__global__ void __launch_bounds__(256) k_fam_p5(RegionDev R, UvcParams P) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= R.n_generic_work) return;
    const FsRec u = R.fss[find_unit(R, w)];
    const int p = u.beg + (int)(w - u.work_off);
    const int64_t x = p - R.beg;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    __shared__ int con_s[NSYM][256], mmm_s[NSYM][256];
    const LdsCounts<256> con = { &con_s[0][threadIdx.x] }, mmm = { &mmm_s[0][threadIdx.x] };
    unit_counts<true>(R, P, u, p, proton, con, mmm);
    const FamAcc A = FamAcc::global(R, x);
    for (int vi = 0; vi < 2; vi++) {
        const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
        p5_apply(A, R, P, u, x, st, p5_cons(con, mmm, st), nullptr);
    }
}

// ---- the digest form: deep data ----
// On deep data (many units per position, e.g. UMI panels) the family passes run per 64-position window: the four waves of a block share the
// units that overlap the window, every lane keeps its position, and the increments of the two dense symbols are collected in LDS (FamAcc).
// k_fam_p4d (+ k_fam_p4d_rest) walks the fragments of a unit once and leaves a digest per (unit, position) cell -- the BQ-sum consensus P5
// needs and the {1, 1}-threshold vote consensus of the duplex pass -- which k_fam_p5d and k_duplex_d only read (R.fam_digest, 8 words).
// Digest words 3 vi .. 3 vi + 2 per symbol type vi (0 = LINK, 1 = BASE): cs | con_nfrags << 4 | tot_nfrags << 18 (the low 14 bits of each
// count), con_sumBQs, tot_sumBQs; word 6, byte vi: the duplex vote (its symbol | 16 if it votes); word 7, bytes 2 vi and 2 vi + 1: the high 8
// bits of con_nfrags and tot_nfrags.  A count is at most the unit's fragment count, below UVC_DIGEST_MAX_VOTES (set_reads); P5 reads word 7
// only for a unit of more than 16 383 fragments.
DEV int64_t digest_cell(const FsRec &u, int p) { return u.work_off + (int64_t)(p - u.beg); }
DEV void digest_store(const RegionDev &R, int64_t cell, const P5Cons m[2], const int dcs[2], const int dadj[2]) {
    uint32_t w[8];
    w[6] = 0; w[7] = 0;
    for (int vi = 0; vi < 2; vi++) {
        w[3 * vi] = (uint32_t)m[vi].cs | (((uint32_t)m[vi].con_nfrags & 16383u) << 4) | ((uint32_t)m[vi].tot_nfrags << 18);
        w[3 * vi + 1] = (uint32_t)m[vi].con_sumBQs; w[3 * vi + 2] = (uint32_t)m[vi].tot_sumBQs;
        w[6] |= ((uint32_t)dcs[vi] | ((dadj[vi] >= 1) ? 16u : 0u)) << (8 * vi);
        w[7] |= (((uint32_t)m[vi].con_nfrags >> 14) | (((uint32_t)m[vi].tot_nfrags >> 14) << 8)) << (16 * vi);
    }
    uint4 *dst = (uint4 *)(R.fam_digest + 8 * cell);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]); dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
DEV void digest_load(const RegionDev &R, const FsRec &u, int p, P5Cons m[2]) {
    const uint32_t *src = R.fam_digest + 8 * digest_cell(u, p);
    const uint4 d0 = *(const uint4 *)src;
    const uint2 d1 = *(const uint2 *)(src + 4);
    const uint32_t w7 = (u.frag_end - u.frag_beg > 16383 ? src[7] : 0u);   // (wave-uniform)
    const uint32_t lo[2] = { d0.x, d0.w };
    for (int vi = 0; vi < 2; vi++) {
        const uint32_t hi = w7 >> (16 * vi);
        m[vi].cs = (int)(lo[vi] & 15u);
        m[vi].con_nfrags = (int)(((lo[vi] >> 4) & 16383u) | ((hi & 255u) << 14));
        m[vi].tot_nfrags = (int)((lo[vi] >> 18) | (((hi >> 8) & 255u) << 14));
    }
    m[0].con_sumBQs = (int)d0.y; m[0].tot_sumBQs = (int)d0.z; m[1].con_sumBQs = (int)d1.x; m[1].tot_sumBQs = (int)d1.y;
}
DEV uint32_t digest_dup_word(const RegionDev &R, int64_t cell) { return R.fam_digest[8 * cell + 6]; }
DEV bool digest_dup_vote(uint32_t w6, int vi, int &sym) { const uint32_t a = (w6 >> (8 * vi)) & 31u; sym = (int)(a & 15u); return (a & 16u) != 0; }

// Calls f(u) for every unit of this wave's share of a window's units [lo, hi) (window index list 7, by begin; the four waves of a block
// take every fourth one) that overlaps the window [w0, w0 + 64).  The unit records are read 64 at a time, one per lane; those that reach
// the window are picked by ballot and their fields broadcast, so a unit that ends in front of the window costs no memory round trip of its
// own.  u is wave-uniform.
template <class F>
DEV void for_window_units(const RegionDev &R, int w0, int lo, int hi, int wv, int lane, F &&f) {
    for (int kb = lo + wv; kb < hi; kb += 4 * 64) {
        int ur[16];
        const int kmine = kb + 4 * lane;
        if (kmine < hi) {
            const int4 *q4 = (const int4 *)(R.fss + R.generic_sorted[kmine]);
#pragma unroll
            for (int i = 0; i < 4; i++) { const int4 t = q4[i]; ur[4 * i] = t.x; ur[4 * i + 1] = t.y; ur[4 * i + 2] = t.z; ur[4 * i + 3] = t.w; }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) ur[i] = 0;
        }
        unsigned long long todo = __ballot(kmine < hi && ur[3] > w0 && ur[2] < w0 + 64);   // FsRec::end, FsRec::beg
        while (todo) {
            const int uj = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            FsRec u;
            u.frag_beg = bcast(ur[0], uj); u.frag_end = bcast(ur[1], uj); u.beg = bcast(ur[2], uj); u.end = bcast(ur[3], uj);
            u.strand = bcast(ur[4], uj); u.dflag = bcast(ur[5], uj); u.fam = bcast(ur[6], uj); u.generic = bcast(ur[7], uj);
            u.work_off = (int64_t)(((unsigned long long)(unsigned)bcast(ur[9], uj) << 32) | (unsigned long long)(unsigned)bcast(ur[8], uj));
            u.l2r_end_median = bcast(ur[10], uj); u.r2l_end_median = bcast(ur[11], uj); u.nsb_min = bcast(ur[12], uj); u.nsb_max = bcast(ur[13], uj);
            u.other_fs = bcast(ur[14], uj); u.pad_ = 0;
            f(u);
        }
    }
}

// The LDS accumulators of a window kernel (FamAcc; a64 / bk may be NULL): zeroed before the units, then one add per non-zero (field, dense
// symbol, position) of the window
DEV void fam_lds_zero(int (*a32)[FAMW_SLOTS][64], unsigned long long (*a64)[UVC_NFAMINFO64][64], int (*bk)[2][NBUCKETS][64]) {
    for (int i = threadIdx.x; i < 2 * FAMW_SLOTS * 64; i += 256) (&a32[0][0][0])[i] = 0;
    if (a64) for (int i = threadIdx.x; i < 2 * UVC_NFAMINFO64 * 64; i += 256) (&a64[0][0][0])[i] = 0ull;
    if (bk) for (int i = threadIdx.x; i < 2 * 2 * NBUCKETS * 64; i += 256) (&bk[0][0][0][0])[i] = 0;
}
DEV void fam_flush(const RegionDev &R, int64_t x0, int (*a32)[FAMW_SLOTS][64], unsigned long long (*a64)[UVC_NFAMINFO64][64], int (*bk)[2][NBUCKETS][64]) {
    for (int i = threadIdx.x; i < 2 * FAMW_SLOTS * 64; i += 256) {
        const int v = (&a32[0][0][0])[i];
        if (!v) continue;
        const int ln = i & 63, slot = (i >> 6) % FAMW_SLOTS, d = (i >> 6) / FAMW_SLOTS;
        const int64_t xx = x0 + ln;
        const int sym = (d == 0 ? (int)R.refsym[xx] : UVC_LINK_M);
        if (slot < 2 * UVC_NFAM) add_own(&FAP(R, slot / UVC_NFAM, slot % UVC_NFAM, sym, xx), v);
        else { mark_fi(R, sym, xx); add_own(&FIP(R, slot - 2 * UVC_NFAM, sym, xx), v); }
    }
    if (a64) for (int i = threadIdx.x; i < 2 * UVC_NFAMINFO64 * 64; i += 256) {
        const unsigned long long v = (&a64[0][0][0])[i];
        if (!v) continue;
        const int ln = i & 63, f = (i >> 6) % UVC_NFAMINFO64, d = (i >> 6) / UVC_NFAMINFO64;
        const int64_t xx = x0 + ln;
        mark_fi(R, (d == 0 ? (int)R.refsym[xx] : UVC_LINK_M), xx);
        add64_own(&FI64P(R, f, (d == 0 ? (int)R.refsym[xx] : UVC_LINK_M), xx), (long long)v);
    }
    if (bk) for (int i = threadIdx.x; i < 2 * 2 * NBUCKETS * 64; i += 256) {
        const int v = (&bk[0][0][0][0])[i];
        if (!v) continue;
        const int ln = i & 63, b = (i >> 6) % NBUCKETS, strand = ((i >> 6) / NBUCKETS) % 2, d = (i >> 6) / (2 * NBUCKETS);
        const int64_t xx = x0 + ln;
        add_own(&BKP(R, strand, (d == 0 ? (int)R.refsym[xx] : UVC_LINK_M), b, xx), v);
    }
}

// the consensus numbers of a (unit, position) that has a fragment of the general kind, for k_fam_p4d_rest: per symbol type the vote
// consensus (vcs, vcc, vct), the BQ-sum consensus (m) and the duplex vote (dcs, dadj)
DEV void general_unit(const RegionDev &R, const UvcParams &P, const FsRec &u, int p, bool proton, bool padded_ignored,
                      int *vcs, int *vcc, int *vct, P5Cons *m, int *dcs, int *dadj) {
    int con_l[NSYM], mmm_l[NSYM];
    unit_counts<true>(R, P, u, p, proton, con_l, mmm_l);
    for (int vi = 0; vi < 2; vi++) {
        const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
        fill_consensus(con_l, vcs[vi], vcc[vi], vct[vi], st, false, false);
        m[vi] = p5_cons(con_l, mmm_l, st);
        int dc, dt;
        fill_consensus(con_l, dcs[vi], dc, dt, st, false, st == UVC_BASE_SYMBOL && padded_ignored);
        dadj[vi] = imax(dc * 2, dt) - dt;
    }
}

// k_fam_p4d: P4 of the generic units on deep data, writing the digest.  The votes (con) and the BQ sums (mmm) of a (unit, position) live in
// registers: a fragment of <= 2 simple alignments can only vote for LINK_M and for one of A C G T N, so the updates are a fixed LINK_M add
// and a select chain over five symbols.  Without per-wave LDS count arrays the block needs 17 KiB of LDS instead of 45, and the
// read-modify-write chains through LDS are gone.  A cell under a fragment of the general kind (InDel next to the position, > 2 alignments)
// is left to k_fam_p4d_rest.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_fam_p4d(RegionDev R, UvcParams P) {
    __shared__ int a32[2][FAMW_SLOTS][64];
    __shared__ unsigned long long a64[2][UVC_NFAMINFO64][64];
    __shared__ long long baq_s[2][P4_BAQ_WIN];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t x0 = (int64_t)xcd_block() * 64;
    if (x0 >= R.npos) return;
    const int w0 = R.beg + (int)x0;
    const int lo = win_lo(R, 7, (int)(x0 >> 6)), hi = win_hi(R, 7, (int)(x0 >> 6));
    if (lo >= hi) return;   // block-uniform
    fam_lds_zero(a32, a64, nullptr);
    // the BAQ prefix sums the position-bias tests of this window can ask for (p4_apply: within MAX_STR_N_BASES of the cell), staged once:
    // six dependent global gathers per (unit, window) otherwise
    const int lb_lo = w0 - MAX_STR_N_BASES - 1;
    for (int i = threadIdx.x; i < P4_BAQ_WIN; i += 256) {
        const long long q = lmin(lmax((long long)lb_lo + i, (long long)R.beg), (long long)R.beg + R.npos - 1);
        baq_s[0][i] = BAQ1(R, q); baq_s[1][i] = BAQ2(R, q);
    }
    __syncthreads();
    const int p = w0 + lane;
    const int64_t x = x0 + lane;
    const bool valid = x < R.npos;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const bool padded_ignored = (P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0;
    FamAcc A; A.a32 = a32; A.a64 = a64; A.bk = nullptr; A.R = &R; A.x = x; A.lane = lane; A.my_ref = (valid ? (int)R.refsym[x] : 0);
    const int noindel80 = ((valid && x > 0) ? imin(80, imin(RTRP(R, UVC_RTR_indelphred, x - 1), RTRP(R, UVC_RTR_indelphred, x))) : 80);
    const __amdgpu_buffer_rsrc_t rs = bq_rsrc(R);
    P4Pos Q = { 0, 0, 0, 0, 0, 0, 0, 0, nullptr, nullptr, 0 };
    if (valid) Q = p4_pos(R, p);
    Q.lb1 = &baq_s[0][0]; Q.lb2 = &baq_s[1][0]; Q.lb_lo = lb_lo;
    for_window_units(R, w0, lo, hi, wv, lane, [&](const FsRec &u) {
        const bool mine = (valid && p >= u.beg && p < u.end);
        // votes / BQ sums of LINK_M and of A C G T N (registers); the other eight symbols only through the general path
        int cL = 0, mL = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
        bool general = false;
        // the fragment records of the unit: one per lane (FragUnit: the first 12 dwords of FragFast), fields of record j broadcast with v_readlane, the base / quality
        // bytes of record j + 1 requested before record j is evaluated -- three dependent memory round trips per unit instead of three per fragment
        const int nfr = u.frag_end - u.frag_beg;
        for (int f0 = 0; f0 < nfr; f0 += 64) {
            int c[12];
            load_words(R.ffast_u + u.frag_beg + f0 + lane, f0 + lane < nfr, c);
            const int n = imin(64, nfr - f0);
            int bq0n = 0, bq1n = 0;
            auto issue = [&](int j) {
                const int fl = bcast(c[FF_W(flags)], j);
                bq0n = bq_load(rs, bcast(c[FF_W(qb0)], j) + p);
                if (ff_naln(fl) == 2) bq1n = bq_load(rs, bcast(c[FF_W(qb1)], j) + p);
            };
            issue(0);
            for (int j = 0; j < n; j++) {
                const int bq0 = bq0n, bq1 = bq1n;
                if (j + 1 < n) issue(j + 1);
                const int fbeg = bcast(c[FF_W(beg)], j), fend = bcast(c[FF_W(end)], j), flags = bcast(c[FF_W(flags)], j);
                if (!(mine && p >= fbeg && p < fend)) continue;
                if ((flags & FF_NOT_REGISTER) != 0 || proton) { general = true; continue; }
                const int pos0 = bcast(c[FF_W(pos0)], j), rend0 = bcast(c[FF_W(rend0)], j), pos1 = bcast(c[FF_W(pos1)], j), rend1 = bcast(c[FF_W(rend1)], j);
                const int nogap0 = bcast(c[FF_W(nogap0)], j), nogap1 = bcast(c[FF_W(nogap1)], j);
                const bool has2 = (ff_naln(flags) == 2);
                const bool in0 = (p >= pos0 && p < rend0), in1 = (has2 && p >= pos1 && p < rend1);
                const int lv = link_better_mate(in0 && p > pos0, in1 && p > pos1, noindel80, nogap0, nogap1);
                if (lv > 0) { cL += 1; mL += lv; }
                if (in0 || in1) {
                    const PairCons pc = pair_consensus(in0, in1, bq0, bq1, P, padded_ignored); const int cs = pc.cs, cc = pc.cc, ct = pc.ct, cs4 = pc.cs4, cc4 = pc.cc4, ct4 = pc.ct4;
                    if (cs > UVC_BASE_N || cs4 > UVC_BASE_N) { general = true; continue; }   // cannot happen for packed base codes 0..4; kept as a guard
                    const int adj = imax(cc4 * 2, ct4) - ct4;
                    const int vote = ((adj >= P.fam_thres_highBQ_snv && adj > 0) ? 1 : 0);
                    c0 += (cs4 == 0 ? vote : 0); c1 += (cs4 == 1 ? vote : 0); c2 += (cs4 == 2 ? vote : 0); c3 += (cs4 == 3 ? vote : 0); c4 += (cs4 == 4 ? vote : 0);
                    const int adj5 = imax(imax(cc * 2, ct) - ct, 0);
                    m0 += (cs == 0 ? adj5 : 0); m1 += (cs == 1 ? adj5 : 0); m2 += (cs == 2 ? adj5 : 0); m3 += (cs == 3 ? adj5 : 0); m4 += (cs == 4 ? adj5 : 0);
                }
            }
        }
        if (!mine || general) return;   // a cell under a fragment of the general kind: k_fam_p4d_rest writes its digest and its increments
        // per symbol type: vote consensus (vcs, vcc, vct), BQ-sum consensus (m) with the votes of its symbol and of the type, duplex vote (dcs, dadj)
        int vcs[2], vcc[2], vct[2], dcs[2], dadj[2];
        P5Cons m[2];
        // LINK: only LINK_M can be non-zero; an empty type gives the last symbol of the type (fill_consensus starts from it)
        vcs[0] = (cL > 0 ? UVC_LINK_M : UVC_LINK_NN); vcc[0] = cL; vct[0] = cL;
        m[0] = { (mL > 0 ? UVC_LINK_M : UVC_LINK_NN), (mL > 0 ? cL : 0), cL, mL, mL };
        dcs[0] = vcs[0]; dadj[0] = cL;   // imax(2 * cc, ct) - ct with cc == ct
        // BASE: first maximum in symbol order A C G T N (NN is zero)
        int bs = UVC_BASE_NN, bc = 0;
        if (c0 > bc) { bs = 0; bc = c0; } if (c1 > bc) { bs = 1; bc = c1; } if (c2 > bc) { bs = 2; bc = c2; } if (c3 > bc) { bs = 3; bc = c3; } if (c4 > bc) { bs = 4; bc = c4; }
        vcs[1] = bs; vcc[1] = bc; vct[1] = c0 + c1 + c2 + c3 + c4;
        int qs = UVC_BASE_NN, qc = 0;
        if (m0 > qc) { qs = 0; qc = m0; } if (m1 > qc) { qs = 1; qc = m1; } if (m2 > qc) { qs = 2; qc = m2; } if (m3 > qc) { qs = 3; qc = m3; } if (m4 > qc) { qs = 4; qc = m4; }
        m[1] = { qs, (qs == 0 ? c0 : qs == 1 ? c1 : qs == 2 ? c2 : qs == 3 ? c3 : qs == 4 ? c4 : 0), vct[1], qc, m0 + m1 + m2 + m3 + m4 };
        // the duplex vote looks at A..T only when padded deletions are ignored (fill_consensus(..., ignore_padded_del)): then the start
        // symbol is T and N does not take part
        if (padded_ignored) {
            int ds = UVC_BASE_T, dc = 0;
            if (c0 > dc) { ds = 0; dc = c0; } if (c1 > dc) { ds = 1; dc = c1; } if (c2 > dc) { ds = 2; dc = c2; } if (c3 > dc) { ds = 3; dc = c3; }
            const int dt = c0 + c1 + c2 + c3;
            dcs[1] = ds; dadj[1] = imax(dc * 2, dt) - dt;
        } else { dcs[1] = bs; dadj[1] = imax(bc * 2, vct[1]) - vct[1]; }
        digest_store(R, digest_cell(u, p), m, dcs, dadj);
        P4Cell W;
        p4_cell(W, R, P, u, p, Q);
        if (vct[0]) { const int d = A.dense(vcs[0]); if (d >= 0) p4_apply_dense<true>(A, d, P, u, vcc[0], vct[0], Q, W); else p4_apply(A, R, P, u, p, x, UVC_LINK_SYMBOL, vcs[0], vcc[0], vct[0], &Q); }
        if (vct[1]) { const int d = A.dense(vcs[1]); if (d >= 0) p4_apply_dense<false>(A, d, P, u, vcc[1], vct[1], Q, W); else p4_apply(A, R, P, u, p, x, UVC_BASE_SYMBOL, vcs[1], vcc[1], vct[1], &Q); }
    });
    __syncthreads();
    fam_flush(R, x0, a32, a64, nullptr);
}

// The cells k_fam_p4d leaves out: positions of a unit under a fragment of the general kind (an InDel read, more than two alignments).
// One wave per generic unit that has such a fragment (FsRec::pad_, set by k_fam_stat), lanes over its positions; the consensus comes from
// the general walk (unit_counts<true>), the increments are global atomics.  A few per cent of the units on panel data.
__global__ void __launch_bounds__(64) k_fam_p4d_rest(RegionDev R, UvcParams P) {
    if ((int)blockIdx.x >= R.n_generic_fs) return;
    const FsRec u = R.fss[R.generic_fs[blockIdx.x]];
    if (!u.pad_) return;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const bool padded_ignored = (P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0;
    for (int p = u.beg + (int)threadIdx.x; p < u.end; p += 64) {
        const int64_t x = (int64_t)p - R.beg;
        if (x < 0 || x >= R.npos) continue;
        bool general = false;
        for (int f = u.frag_beg; f < u.frag_end && !general; f++) {
            const FragUnit &ff = R.ffast_u[f];
            general = (p >= ff.beg && p < ff.end && (((ff.flags & FF_NOT_REGISTER) != 0) || proton));
        }
        if (!general) continue;
        int vcs[2], vcc[2], vct[2], dcs[2], dadj[2];
        P5Cons m[2];
        general_unit(R, P, u, p, proton, padded_ignored, vcs, vcc, vct, m, dcs, dadj);
        digest_store(R, digest_cell(u, p), m, dcs, dadj);
        const FamAcc A = FamAcc::global(R, x);
        for (int vi = 0; vi < 2; vi++) {
            if (0 == vct[vi]) continue;
            p4_apply(A, R, P, u, p, x, (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL), vcs[vi], vcc[vi], vct[vi], nullptr);
        }
    }
}

// k_fam_p5d: P5 of the generic units on deep data, from the digest k_fam_p4d / k_fam_p4d_rest left
__global__ void __launch_bounds__(256) k_fam_p5d(RegionDev R, UvcParams P) {
    __shared__ int a32[2][FAMW_SLOTS][64];
    __shared__ int bk[2][2][NBUCKETS][64];
    __shared__ double p2p_s[128];   // phred2prob of every average quality a cell can have: one pow() per value and block, not one per cell
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t x0 = (int64_t)xcd_block() * 64;
    if (x0 >= R.npos) return;
    const int w0 = R.beg + (int)x0;
    const int lo = win_lo(R, 7, (int)(x0 >> 6)), hi = win_hi(R, 7, (int)(x0 >> 6));
    if (lo >= hi) return;   // block-uniform
    fam_lds_zero(a32, nullptr, bk);
    for (int i = threadIdx.x; i < 128; i += 256) p2p_s[i] = phred2prob(i);   // the fp64 expression of fam_qual
    __syncthreads();
    const int p = w0 + lane;
    const int64_t x = x0 + lane;
    const bool valid = x < R.npos;
    FamAcc A; A.a32 = a32; A.a64 = nullptr; A.bk = bk; A.R = &R; A.x = x; A.lane = lane; A.my_ref = (valid ? (int)R.refsym[x] : 0);
    for_window_units(R, w0, lo, hi, wv, lane, [&](const FsRec &u) {
        if (!(valid && p >= u.beg && p < u.end)) return;
        P5Cons m[2];
        digest_load(R, u, p, m);
        p5_apply(A, R, P, u, x, UVC_LINK_SYMBOL, m[0], p2p_s);
        p5_apply(A, R, P, u, x, UVC_BASE_SYMBOL, m[1], p2p_s);
    });
    __syncthreads();
    fam_flush(R, x0, a32, nullptr, bk);
}

// duplex consensus (main.hpp:3427-3433, 3523-3550): one thread per (strand-0 unit of a duplex family with both strands, position)
__global__ void __launch_bounds__(256) k_duplex(RegionDev R, UvcParams P, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_work) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_work) return;
    int lo = 0, hi = n_dup;
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (dup_off[mid] <= w) lo = mid; else hi = mid; }
    const FsRec u0 = R.fss[dup_units[lo]];
    const FsRec u1 = R.fss[u0.other_fs];
    const int dbeg = imin(u0.beg, u1.beg);
    const int p = dbeg + (int)(w - dup_off[lo]);
    const int64_t x = p - R.beg;
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const bool padded_ignored = (P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0;
    __shared__ int con_s[NSYM][256], dup_s[NSYM][256];
    const LdsCounts<256> con = { &con_s[0][threadIdx.x] }, dup = { &dup_s[0][threadIdx.x] };
    for (int s = 0; s < NSYM; s++) dup[s] = 0;
    for (int k = 0; k < 2; k++) {
        const FsRec &u = (k == 0 ? u0 : u1);
        if (p < u.beg || p >= u.end) continue;
        unit_counts<false>(R, P, u, p, proton, con, con);
        for (int st = 0; st < 2; st++) {   // updateByFiltering<true,false,false> with thresholds {1,1}
            int cs, cc, ct;
            fill_consensus(con, cs, cc, ct, st, false, st == UVC_BASE_SYMBOL && padded_ignored);
            const int adj = imax(cc * 2, ct) - ct;
            if (adj >= 1 && adj > 0) dup[cs] += 1;
        }
    }
    for (int st = 0; st < 2; st++) {
        int cs, cc, ct;
        fill_consensus(dup, cs, cc, ct, st, false, false);
        if (0 < ct) { mark_dup(R, cs, x); atomicAdd(&DUP(R, UVC_DUPLEX_dDP1, cs, x), 1); }
        if (1 < ct) atomicAdd(&DUP(R, UVC_DUPLEX_dDP2, cs, x), 1);
    }
}

// the duplex pass from the digest (k_fam_p4d / k_fam_p4d_rest): the votes of the two strand units of a duplex family at a position
__global__ void __launch_bounds__(64) k_duplex_d(RegionDev R, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_work) {
    // one wave per duplex family (its strand-0 unit), lanes over the positions of the two units' common span: no search for the family of a
    // (family, position) cell, the two unit records are read once
    if ((int)blockIdx.x >= n_dup) return;
    const FsRec u0 = R.fss[dup_units[blockIdx.x]];
    const FsRec u1 = R.fss[u0.other_fs];
    const int pbeg = imin(u0.beg, u1.beg);
    const int span = (int)(((int)blockIdx.x + 1 < n_dup ? dup_off[blockIdx.x + 1] : n_work) - dup_off[blockIdx.x]);   // the family's cells in the old (family, position) numbering
    for (int i = (int)threadIdx.x; i < span; i += 64) {
        const int p = pbeg + i;
        const int64_t x = p - R.beg;
        const uint32_t w0 = ((p >= u0.beg && p < u0.end) ? digest_dup_word(R, digest_cell(u0, p)) : 0u);
        const uint32_t w1 = ((p >= u1.beg && p < u1.end) ? digest_dup_word(R, digest_cell(u1, p)) : 0u);
        for (int vi = 0; vi < 2; vi++) {   // fill_consensus over at most two votes: the larger count wins, the smaller symbol on a tie
            int sa, sb;
            const bool va = digest_dup_vote(w0, vi, sa), vb = digest_dup_vote(w1, vi, sb);
            if (!va && !vb) continue;
            const int ct = (va ? 1 : 0) + (vb ? 1 : 0);
            const int cs = (va && vb) ? ((sa == sb) ? sa : imin(sa, sb)) : (va ? sa : sb);
            mark_dup(R, cs, x);
            atomicAdd(&DUP(R, UVC_DUPLEX_dDP1, cs, x), 1);
            if (1 < ct) atomicAdd(&DUP(R, UVC_DUPLEX_dDP2, cs, x), 1);   // tot_count of the two votes, as fill_consensus sums it (main.hpp:3540-3546)
        }
    }
}

// P5b (main.hpp:3552-3591): one thread per (position, strand)
__global__ void __launch_bounds__(256) k_p5b(RegionDev R, UvcParams P) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R.npos * 2) return;
    if (!R.p5flag[t]) return;   // no P5 bucket was filled at this (strand, position): every output is 0 (the flag index is strand * npos + x)
    const int strand = (int)(t / R.npos);
    const int64_t x = t % R.npos;
    const int qIAQ = (strand ? UVC_VQ_cIAQr : UVC_VQ_cIAQf), qIAD = (strand ? UVC_VQ_cIADr : UVC_VQ_cIADf), qIDQ = (strand ? UVC_VQ_cIDQr : UVC_VQ_cIDQf);
    const int ref_symbol = R.refsym[x];
    for (int st = 0; st < 2; st++) {
        const int sb = (st == 0 ? UVC_BASE_A : UVC_LINK_M), se = (st == 0 ? UVC_BASE_NN : UVC_LINK_NN);
        int totDP = 0;
        for (int s = sb; s <= se; s++) totDP += FAP(R, strand, UVC_FAM_cDP1, s, x);
        if (totDP == 0) continue;
        for (int s = sb; s <= se; s++) {
            if (0 == FAP(R, strand, UVC_FAM_cDP1, s, x)) continue;   // k_fam_p5 fills a bucket only next to a cDP1 increment of the same symbol: empty histogram, all outputs 0
            const int max_qual = sscs_phred(P, ref_symbol, s) + (!P.tumor_vcf_is_provided ? 0 : 4);
            int mv, ad, bq;
            infer_max_qual(mv, ad, bq, max_qual, 4, totDP, [&](int b) { return BKP(R, strand, s, b, x); });
            if (mv | ad | bq) { VQP(R, qIAQ, s, x) += mv; VQP(R, qIAD, s, x) += ad; VQP(R, qIDQ, s, x) += bq; }
            // the bucket planes are transient: leave them zero so that the next accumulate need not clear them
            for (int b = 0; b < NBUCKETS; b++) if (BKP(R, strand, s, b, x)) BKP(R, strand, s, b, x) = 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// InDel allele tables.  The reference keeps, beside FRAG_bDP / FAM_cDP12.. / FAM_cDP2 / FAM_cDPD + DUPLEX_dDP2, maps
// position -> inserted sequence (or deleted length) -> count (main.hpp:2710-2717, 3327-3336, 3196-3206, 3458-3469, 3535-3546), and
// scoring splits every InDel symbol into its alleles with them (fill_by_indel_info / indel_get_majority, main.hpp:5350-5455).
// Here: k_p2_slow<false> leaves one AlnGap event per I / D op; the events are sorted by (family, position); k_gap_alleles takes
// one (family, position) per thread, redoes the fragment / family / duplex consensus of the LINK symbol type at that position
// and emits one increment per map update; the increments are sorted by (position, symbol, allele) and k_gap_rows sums the runs.
// ------------------------------------------------------------------------------------------------
DEV int base_text_rank(int b) { return b == UVC_BASE_N ? 3 : (b == UVC_BASE_T ? 4 : b); }   // order of the characters "ACGTN": A < C < G < N < T
// order of two alleles of the same symbol: std::string resp. integer key order of the reference's maps
DEV int gap_cmp(const RegionDev &R, const AlnGap &a, const AlnGap &b) {
    if (is_del(a.sym)) return (a.len > b.len) - (a.len < b.len);
    const uint8_t *sa = R.bases + R.alns[a.aln].seq_off + a.qpos, *sb = R.bases + R.alns[b.aln].seq_off + b.qpos;
    const int n = imin(a.len, b.len);
    for (int i = 0; i < n; i++) { const int ra = base_text_rank(sa[i]), rb = base_text_rank(sb[i]); if (ra != rb) return ra < rb ? -1 : 1; }
    return (a.len > b.len) - (a.len < b.len);
}
// 35-bit allele code: exact for deletions and for insertions of up to 13 bases (base-5 digits behind a leading 1 < 5^14 < 2^33), a hash
// with bit 34 set for longer insertions
DEV unsigned long long gap_code(const RegionDev &R, const AlnGap &e) {
    if (is_del(e.sym)) return (unsigned long long)e.len & ((1ull << 33) - 1ull);
    const uint8_t *s = R.bases + R.alns[e.aln].seq_off + e.qpos;
    if (e.len <= 13) { unsigned long long c = 1; for (int i = 0; i < e.len; i++) c = c * 5ull + s[i]; return c; }
    unsigned long long h = 1469598103934665603ull ^ (unsigned long long)e.len;
    for (int i = 0; i < e.len; i++) { h ^= s[i]; h *= 1099511628211ull; }
    return (1ull << 34) | (h >> 30);
}

__global__ void __launch_bounds__(256) k_gap_keys(RegionDev R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.gap.n_ev) return;
    const AlnGap e = R.gap.ev[i];
    unsigned long long key = ~0ull;
    if (e.sym >= 0) key = ((unsigned long long)R.fss[R.alns[e.aln].fs].fam << 26) | (unsigned long long)(e.epos - R.beg);
    R.gap.ckey[i] = key; R.gap.cval[i] = (unsigned long long)i;
}

// The events of one (family, position) run as k_gap_alleles reads them.  GapEvGlobal: straight from the event array (any run).  GapEvLds: from
// the block's LDS copy, where every lane has loaded one event and worked out its allele code -- the consensus arithmetic below is O(n^2)
// in the events of the run and, read from global memory, a chain of thousands of dependent loads for one family of a 2000x panel (one
// thread's chain was the kernel's whole 2.6 ms).  Runs that leave the block's 128-event window, or hold an insertion longer than 13 bases
// (hashed code: equality needs the sequences), take the global form.
struct GapEvL { int32_t sym, aln, weight, mark, id, pad_; unsigned long long code; };
struct GapEvGlobal {
    const RegionDev &R; AlnGap *ev; const unsigned long long *order; int i0;
    DEV int id(int k) const { return (int)order[i0 + k]; }
    DEV int sym(int k) const { return ev[id(k)].sym; }
    DEV int aln(int k) const { return ev[id(k)].aln; }
    DEV int weight(int k) const { return ev[id(k)].weight; }
    DEV int mark(int k) const { return ev[id(k)].mark; }
    DEV void set_mark(int k, int v) const { ev[id(k)].mark = v; }
    DEV bool same(int a, int b) const { return 0 == gap_cmp(R, ev[id(a)], ev[id(b)]); }
    DEV int cmp(int a, int b) const { return gap_cmp(R, ev[id(a)], ev[id(b)]); }
    DEV unsigned long long code(int k) const { return gap_code(R, ev[id(k)]); }
};
struct GapEvLds {
    const RegionDev &R; AlnGap *ev; GapEvL *L;
    DEV int id(int k) const { return L[k].id; }
    DEV int sym(int k) const { return L[k].sym; }
    DEV int aln(int k) const { return L[k].aln; }
    DEV int weight(int k) const { return L[k].weight; }
    DEV int mark(int k) const { return L[k].mark; }
    DEV void set_mark(int k, int v) const { L[k].mark = v; }
    DEV bool same(int a, int b) const { return L[a].code == L[b].code; }   // (callers compare events of one symbol; exact codes only)
    DEV int cmp(int a, int b) const { return gap_cmp(R, ev[L[a].id], ev[L[b].id]); }   // ties between different alleles: rare
    DEV unsigned long long code(int k) const { return L[k].code; }
};

// one (family, position): events [0, nrun) of E, the first of them at sorted index i0
template <class EV>
DEV void gap_alleles_run(const RegionDev &R, const UvcParams &P, const EV &E, const int i0, const int nrun) {
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    AlnGap *ev = R.gap.ev;
    const int epos = ev[E.id(0)].epos;
    const long long x = epos - R.beg;
    for (int k = 0; k < nrun; k++) E.set_mark(k, 0);
    auto emit = [&](int strand, int level, int sym, int k) {
        const int q = atomicAdd(R.gap.n_inc, 1);
        if (q >= R.gap.inc_cap) { atomicExch(R.err, UVCGPU_EDEVICE); return; }   // cannot happen: the capacity is 7 per event + 8
        R.gap.ikey[q] = ((unsigned long long)x << 38) | ((unsigned long long)(sym - UVC_LINK_D3P) << 35) | E.code(k);
        R.gap.ival[q] = ((unsigned long long)E.id(k) << 8) | (unsigned long long)(strand * 4 + level);
    };
    // the event among `cand(k)` whose allele has the largest total weight; ties go to the larger allele (indelToData_getMajority, main.hpp:50-63)
    auto majority = [&](auto cand, auto weight) -> int {
        int best = -1; long long best_w = 0;
        for (int k = 0; k < nrun; k++) {
            if (!cand(k)) continue;
            long long w = 0;
            for (int j = 0; j < nrun; j++) if (cand(j) && E.same(k, j)) w += weight(j);
            // two steps on purpose: written as one expression `best < 0 || w > best_w || (w == best_w && gap_cmp(...) > 0)` the tie arm was
            // never taken in the code hipcc 7.2 generated at -O3 (found with device printf; tests/test_gpu_indel_alleles.py covers it)
            bool take = (best < 0 || w > best_w);
            if (!take && w == best_w) { const int c = E.cmp(k, best); take = (c > 0); }
            if (take) { best = k; best_w = w; }
        }
        return best;
    };
    const int fs_first = R.alns[E.aln(0)].fs;
    const FsRec u_first = R.fss[fs_first];
    int units[2] = { -1, -1 };
    units[u_first.strand] = fs_first; units[1 - u_first.strand] = u_first.other_fs;
    const bool is_duplex_fam = ((u_first.dflag & UVC_DFLAG_DUPLEX) != 0);
    const bool will_inc_dscs = is_duplex_fam && units[0] >= 0 && units[1] >= 0;
    const bool will_inc_sscs = is_duplex_fam && !will_inc_dscs;
    int con[2][NSYM], mmm[2][NSYM], cnt[NSYM];
    for (int s = 0; s < 2; s++) for (int k = 0; k < NSYM; k++) { con[s][k] = 0; mmm[s][k] = 0; }
    R.gap.maj[2 * i0] = 0; R.gap.maj[2 * i0 + 1] = 0;
    // fragments: P3 consensus (main.hpp:2650-2717) and their votes for the unit (updateByFiltering / updateByMajorMinusMinor, main.hpp:1659-1725)
    for (int s = 0; s < 2; s++) {
        if (units[s] < 0) continue;
        const FsRec u = R.fss[units[s]];
        for (int fi = u.frag_beg; fi < u.frag_end; fi++) {
            const FragRec f = R.frags[fi];
            if (epos < f.beg || epos >= f.end) continue;
            frag_counts(R, P, f, epos, proton, cnt);
            int cs, cc, ct;
            fill_consensus(cnt, cs, cc, ct, UVC_LINK_SYMBOL, true, false);
            if (0 == ct) continue;
            const int adj = imax(cc * 2, ct) - ct;
            if (adj > 0) { con[s][cs] += 1; mmm[s][cs] += adj; }
            if (!(is_ins(cs) || is_del(cs))) continue;
            const int e = majority([&](int q) { return E.sym(q) == cs && E.aln(q) >= f.aln_beg && E.aln(q) < f.aln_end; }, [&](int q) { return (long long)E.weight(q); });
            if (e < 0) { atomicExch(R.err, UVCGPU_EDEVICE); continue; }   // an InDel consensus without an InDel event cannot happen
            E.set_mark(e, 0x10000 | (s << 8) | cs);
            emit(s, 0, cs, e);
        }
    }
    // family x strand units: P4 (main.hpp:3180-3336) and P5 (main.hpp:3448-3469)
    int dup[NSYM], dup_allele[2] = { -1, -1 }, dup_sym[2] = { -1, -1 };
    for (int k = 0; k < NSYM; k++) dup[k] = 0;
    for (int s = 0; s < 2; s++) {
        if (units[s] < 0) continue;
        const FsRec u = R.fss[units[s]];
        auto unit_allele = [&](int sym) { return majority([&](int q) { return E.mark(q) == (0x10000 | (s << 8) | sym); }, [&](int q) { return 1LL; }); };
        {   // the count read_family_con_ampl_getMajority_ins returns: the inserted sequence most fragments of the unit agree on, over all three
            // insertion symbols (main.hpp:188-198); the FAM2 position-bias test of the family kernels reads it (main.hpp:3239-3246)
            // (the map is fed by every fragment whose consensus is an insertion symbol, main.hpp:1670-1676: the marked events of the unit)
            int m = 0;
            for (int k = 0; k < nrun; k++) {
                const int mk = E.mark(k);
                if ((mk >> 8) != (0x100 | s) || !is_ins(mk & 0xFF)) continue;
                int w = 0;
                for (int j = 0; j < nrun; j++) if (E.mark(j) == mk && E.same(k, j)) w++;
                m = imax(m, w);
            }
            R.gap.maj[2 * i0 + s] = m;
        }
        int cs, cc, ct;
        fill_consensus(con[s], cs, cc, ct, UVC_LINK_SYMBOL, false, false);
        if (ct > 0 && (is_ins(cs) || is_del(cs))) {
            const int e = unit_allele(cs);
            if (e < 0) atomicExch(R.err, UVCGPU_EDEVICE);
            else {
                const bool fam_good = is_fam_good(cc, ct, u.dflag, P);
                emit(s, 1, cs, e);
                if (fam_good) emit(s, 2, cs, e);
            }
        }
        if (will_inc_dscs) {   // updateByFiltering<true, false, false>(con, {1, 1}), main.hpp:3429-3432
            const int adj = imax(cc * 2, ct) - ct;
            if (adj >= 1) dup[cs] += 1;
            if (is_ins(cs) || is_del(cs)) { dup_allele[s] = unit_allele(cs); dup_sym[s] = cs; }
        }
        int c5, cc5, ct5;
        fill_consensus(mmm[s], c5, cc5, ct5, UVC_LINK_SYMBOL, false, false);
        if (ct5 > 0 && (is_ins(c5) || is_del(c5))) {
            const int con_nfrags = con[s][c5];
            int tot_nfrags = 0;
            for (int k = UVC_LINK_M; k <= UVC_LINK_NN; k++) tot_nfrags += con[s][k];
            if (will_inc_sscs && (!will_inc_dscs) && (tot_nfrags >= P.fam_thres_dup1add) && (con_nfrags * 100 >= tot_nfrags * P.fam_thres_dup1perc)) {
                const int e = unit_allele(c5);
                if (e < 0) atomicExch(R.err, UVCGPU_EDEVICE); else emit(s, 3, c5, e);
            }
        }
    }
    if (will_inc_dscs) {   // main.hpp:3523-3548
        int cs, cc, ct;
        fill_consensus(dup, cs, cc, ct, UVC_LINK_SYMBOL, false, false);
        if (1 < ct && (is_ins(cs) || is_del(cs))) {
            int e = -1;
            const bool h0 = (dup_sym[0] == cs && dup_allele[0] >= 0), h1 = (dup_sym[1] == cs && dup_allele[1] >= 0);
            if (h0 && h1) e = (E.cmp(dup_allele[0], dup_allele[1]) >= 0 ? dup_allele[0] : dup_allele[1]);
            else if (h0) e = dup_allele[0];
            else if (h1) e = dup_allele[1];
            if (e < 0) atomicExch(R.err, UVCGPU_EDEVICE);
            else { emit(0, 3, cs, e); emit(1, 3, cs, e); }
        }
    }
}

#define GAP_WIN 128
__global__ void __launch_bounds__(64) k_gap_alleles(RegionDev R, UvcParams P) {
    __shared__ GapEvL arena[GAP_WIN];
    const int n = R.gap.n_ev, b0 = blockIdx.x * 64, lane = threadIdx.x;
    const unsigned long long *order = R.gap.cval_s;
    AlnGap *ev = R.gap.ev;
    // every lane brings two events of the block's window into LDS, with their allele codes
    for (int h = 0; h < GAP_WIN / 64; h++) {
        const int i = b0 + h * 64 + lane;
        GapEvL g; g.sym = -1; g.aln = 0; g.weight = 0; g.mark = 0; g.id = 0; g.pad_ = 0; g.code = 0;
        if (i < n && R.gap.ckey_s[i] != ~0ull) {
            const int e = (int)order[i];
            const AlnGap a = ev[e];
            g.sym = a.sym; g.aln = a.aln; g.weight = a.weight; g.id = e; g.code = gap_code(R, a);
        }
        arena[h * 64 + lane] = g;
    }
    __syncthreads();
    const int i0 = b0 + lane;
    if (i0 >= n) return;
    const unsigned long long key = R.gap.ckey_s[i0];
    if (key == ~0ull || (i0 > 0 && R.gap.ckey_s[i0 - 1] == key)) return;   // one thread per (family, position): the head of the run
    int i1 = i0 + 1;
    while (i1 < n && R.gap.ckey_s[i1] == key) i1++;
    bool in_lds = (i1 - b0 <= GAP_WIN);
    for (int i = i0; in_lds && i < i1; i++) if ((arena[i - b0].code >> 34) & 1ull) in_lds = false;   // (an insertion of more than 13 bases)
    if (in_lds) { const GapEvLds E{ R, ev, arena + lane }; gap_alleles_run(R, P, E, i0, i1 - i0); }
    else { const GapEvGlobal E{ R, ev, order, i0 }; gap_alleles_run(R, P, E, i0, i1 - i0); }
}

// The sorted increments -> one GapRow per (position, symbol, allele).  At 2000x a site's allele has thousands of increments, so a run is
// not summed by one thread: k_gap_rows opens a row per run (the head of the run), k_gap_rows_add lets every increment find its run's head
// (binary search in the sorted keys) and add itself to the row's counters, k_gap_rows_fin fills in the allele of each row from its
// representative event (the smallest event index of the run).  `run_row` (the unsorted key array, free once the sort has run) holds the
// row of each run at the index of its head.
__global__ void __launch_bounds__(256) k_gap_rows(RegionDev R) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = imin(*R.gap.n_inc, R.gap.inc_cap);
    if (i0 >= n) return;
    const unsigned long long key = R.gap.ikey_s[i0];
    if (i0 > 0 && R.gap.ikey_s[i0 - 1] == key) return;
    int32_t *run_row = (int32_t *)R.gap.ikey;
    const bool hashed = ((key >> 34) & 1ull) != 0;
    if (!hashed) {   // exact codes: the whole run is one row
        const int r = atomicAdd(R.gap.n_rows, 1);
        GapRow row;
        for (int k = 0; k < 8; k++) row.cnt[k] = 0;
        row.x = (int)(key >> 38); row.sym = -1; row.len = 0; row.ev = INT32_MAX; row.seq_off = -1;
        R.gap.rows[r] = row;
        run_row[i0] = r;
        return;
    }
    // The allele code of an insertion longer than 13 bases is a hash: equal keys need not be equal sequences.  Such a run is split by
    // comparing the sequences themselves (one pass when they all agree, which is the case unless two long insertions of one site collide
    // in 34 bits); bit 63 of a value marks an increment that has found its row.  Long insertions are rare: this thread does the run alone.
    run_row[i0] = -1;
    int i1 = i0;
    while (i1 < n && R.gap.ikey_s[i1] == key) i1++;
    for (int ib = i0; ib < i1; ib++) {
        if (R.gap.ival_s[ib] >> 63) continue;
        const AlnGap first = R.gap.ev[(int)((R.gap.ival_s[ib] & ~(1ull << 63)) >> 8)];
        GapRow row;
        for (int k = 0; k < 8; k++) row.cnt[k] = 0;
        int rep = INT32_MAX;
        for (int i = ib; i < i1; i++) {
            const unsigned long long v = R.gap.ival_s[i];
            if (v >> 63) continue;
            if (i != ib && 0 != gap_cmp(R, first, R.gap.ev[(int)(v >> 8)])) continue;   // another sequence under the same hash: a later row
            row.cnt[v & 0xFF] += 1;
            rep = imin(rep, (int)(v >> 8));
            R.gap.ival_s[i] = v | (1ull << 63);
        }
        row.x = (int)(key >> 38); row.sym = -1; row.len = 0; row.ev = rep; row.seq_off = -1;
        R.gap.rows[atomicAdd(R.gap.n_rows, 1)] = row;
    }
}
__global__ void __launch_bounds__(256) k_gap_rows_add(RegionDev R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = imin(*R.gap.n_inc, R.gap.inc_cap);
    if (i >= n) return;
    const unsigned long long key = R.gap.ikey_s[i];
    if ((key >> 34) & 1ull) return;   // hashed alleles: done by the head of the run
    int lo = 0, hi = i;   // first index with this key
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (R.gap.ikey_s[mid] < key) lo = mid + 1; else hi = mid; }
    const int r = ((const int32_t *)R.gap.ikey)[lo];
    const unsigned long long v = R.gap.ival_s[i];
    atomicAdd(&R.gap.rows[r].cnt[v & 0xFF], 1);
    atomicMin(&R.gap.rows[r].ev, (int)(v >> 8));
}
__global__ void __launch_bounds__(256) k_gap_rows_fin(RegionDev R) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *R.gap.n_rows) return;
    GapRow &row = R.gap.rows[r];
    const AlnGap e = R.gap.ev[row.ev];
    row.sym = e.sym; row.len = e.len;
    if (is_ins(e.sym)) {
        const long long off = (long long)atomicAdd(R.gap.seq_len, (unsigned long long)e.len);
        if (off + e.len <= R.gap.seq_cap) {
            const uint8_t *src = R.bases + R.alns[e.aln].seq_off + e.qpos;
            for (int k = 0; k < e.len; k++) R.gap.seq[off + k] = src[k];
            row.seq_off = off;
        } else atomicExch(R.err, UVCGPU_EDEVICE);
    }
}

// ------------------------------------------------------------------------------------------------
// Haplotype links.  The reference strings together, per fragment (P3) and per family-strand unit (P5), the positions whose
// consensus symbol is a high-quality mutation (main.hpp:2720-2737, 3490-3521) and counts equal strings per strand
// (mutform2count4map_bq / _fq / _f2q); updateHapMap (main.hpp:3596-3663) turns the maps into the links FORMAT/bHap, cHap, c2Hap print.
// Only objects with at least two such positions matter, and an object cannot have more of them than its alignments have mismatching
// bases + InDel ops (AlnRec::n_mutc).  So: pick the candidates, reserve their slots, then one wave per candidate re-derives its consensus
// along its span (the generic per-position forms: this is O(candidates), off the accumulate path, run when the links are asked for).
// The maps, the sort and the link arithmetic are host work on a few thousand short lists (uvc_hap.cpp).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_hap_cand(RegionDev R, HapWork H, int units) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = units ? R.n_fs : R.n_frags;
    if (i >= n) return;
    int a0, a1;
    if (units) { const FsRec &u = R.fss[i]; a0 = R.frags[u.frag_beg].aln_beg; a1 = R.frags[u.frag_end - 1].aln_end; }
    else { a0 = R.frags[i].aln_beg; a1 = R.frags[i].aln_end; }
    int bound = 0;
    for (int k = a0; k < a1; k++) bound += R.alns[k].n_mutc;
    if (bound < 2) return;
    const int span = units ? (R.fss[i].end - R.fss[i].beg) : (R.frags[i].end - R.frags[i].beg);
    bound = imin(bound, 2 * span);
    const int slot = atomicAdd(H.n_cand, 1);
    H.cand[slot] = i; H.cand_cap[slot] = bound;
    H.cand_off[slot] = (int)atomicAdd(H.total, (unsigned long long)((units ? 2 : 1) * (bound + 2)));
}
// appends this lane's (up to two) events in lane order behind `count` events already written; LINK before BASE at one position
DEV int hap_append(int32_t *dst, int cap, int count, bool evL, int vL, bool evB, int vB, int lane, int32_t *err) {
    const unsigned long long mL = __ballot(evL), mB = __ballot(evB), below = (lane == 0 ? 0ull : (~0ull >> (64 - lane)));
    const int at = count + __popcll(mL & below) + __popcll(mB & below);
    if (evL) { if (at < cap) dst[2 + at] = vL; else atomicExch(err, UVCGPU_EDEVICE); }
    if (evB) { const int a2 = at + (evL ? 1 : 0); if (a2 < cap) dst[2 + a2] = vB; else atomicExch(err, UVCGPU_EDEVICE); }
    return count + __popcll(mL) + __popcll(mB);
}
__global__ void __launch_bounds__(64) k_hap_frags(RegionDev R, UvcParams P, HapWork H, int n_cand) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_cand) return;
    const int fi = H.cand[t];
    const FragRec &f = R.frags[fi];
    int32_t *dst = H.events + H.cand_off[t];
    const int cap = H.cand_cap[t];
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    int count = 0;
    int cnt[NSYM];
    for (int i0 = 0; i0 < f.end - f.beg; i0 += 64) {
        const int p = f.beg + i0 + lane;
        bool ev[2] = { false, false }; int val[2] = { 0, 0 };
        if (p < f.end) {
            frag_counts(R, P, f, p, proton, cnt);
            const int refsymbol = R.refsym[p - R.beg];
            for (int vi = 0; vi < 2; vi++) {   // SYMBOL_TYPES_IN_VCF_ORDER: LINK, then BASE
                const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
                int cs, cc, ct;
                fill_consensus(cnt, cs, cc, ct, st, st == UVC_LINK_SYMBOL, false);
                if (0 == ct) continue;
                const int con_qual = cc * 2 - ct;
                const bool highBQ = (proton ? (UVC_BASE_SYMBOL == st || con_qual + 3 >= P.bias_thres_highBQ) : (UVC_LINK_SYMBOL == st || con_qual >= P.bias_thres_highBQ));
                if (symbols_mutated(refsymbol, cs) && highBQ) { ev[vi] = true; val[vi] = ((p - R.beg) << 4) | cs; }
            }
        }
        count = hap_append(dst, cap, count, ev[0], val[0], ev[1], val[1], lane, R.err);
    }
    if (lane == 0) { dst[0] = f.strand | (cap << 8); dst[1] = imin(count, cap); }   // kind 0 (bq); the slot length lets the host walk the buffer
}
__global__ void __launch_bounds__(64) k_hap_units(RegionDev R, UvcParams P, HapWork H, int n_cand) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= n_cand) return;
    const FsRec u = R.fss[H.cand[t]];
    const int cap = H.cand_cap[t];
    int32_t *dst1 = H.events + H.cand_off[t], *dst2 = dst1 + cap + 2;   // fq, f2q
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const int strand = u.strand;
    __shared__ int con_s[NSYM][64], mmm_s[NSYM][64];
    const LdsCounts<64> con = { &con_s[0][lane] }, mmm = { &mmm_s[0][lane] };
    int count1 = 0, count2 = 0;
    for (int i0 = 0; i0 < u.end - u.beg; i0 += 64) {
        const int p = u.beg + i0 + lane;
        bool ev1[2] = { false, false }, ev2[2] = { false, false }; int val[2] = { 0, 0 };
        if (p < u.end) {
            const int64_t x = p - R.beg;
            unit_counts<true>(R, P, u, p, proton, con, mmm);
            for (int vi = 0; vi < 2; vi++) {
                const int st = (vi == 0 ? UVC_LINK_SYMBOL : UVC_BASE_SYMBOL);
                const P5Cons c = p5_cons(con, mmm, st);
                if (0 == c.tot_sumBQs) continue;
                const int cs = c.cs;
                int avgBQ;
                const int confam_qual = fam_qual(R, P, strand, x, st, c, nullptr, avgBQ);   // the empirical family quality of P5
                const bool highBQ = (proton ? (UVC_BASE_SYMBOL == st || imax(confam_qual + 3, avgBQ) >= P.bias_thres_highBQ) : (UVC_LINK_SYMBOL == st || confam_qual >= P.bias_thres_highBQ));
                if (symbols_mutated(R.refsym[x], cs) && highBQ) {
                    ev1[vi] = true; val[vi] = ((int)x << 4) | cs;
                    int cs1, cc1, ct1;
                    fill_consensus(con, cs1, cc1, ct1, st, false, false);
                    if (cs == cs1 && P.fam_thres_dup1add <= ct1 && (cc1 * 100 >= ct1 * P.fam_thres_dup1perc)) ev2[vi] = true;
                }
            }
        }
        count1 = hap_append(dst1, cap, count1, ev1[0], val[0], ev1[1], val[1], lane, R.err);
        count2 = hap_append(dst2, cap, count2, ev2[0], val[0], ev2[1], val[1], lane, R.err);
    }
    if (lane == 0) { dst1[0] = strand | (1 << 1) | (cap << 8); dst1[1] = imin(count1, cap); dst2[0] = strand | (2 << 1) | (cap << 8); dst2[1] = imin(count2, cap); }
}
extern "C" void uvc_launch_hap_cand(const RegionDev *R, const HapWork *H, int units, hipStream_t s) {
    const int n = units ? R->n_fs : R->n_frags;
    if (n > 0) hipLaunchKernelGGL(k_hap_cand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, *R, *H, units);
}
extern "C" void uvc_launch_hap_events(const RegionDev *R, const UvcParams *P, const HapWork *H, int units, int n_cand, hipStream_t s) {
    if (n_cand <= 0) return;
    if (units) hipLaunchKernelGGL(k_hap_units, dim3((unsigned)n_cand), dim3(64), 0, s, *R, *P, *H, n_cand);
    else hipLaunchKernelGGL(k_hap_frags, dim3((unsigned)n_cand), dim3(64), 0, s, *R, *P, *H, n_cand);
}

// ------------------------------------------------------------------------------------------------
// Family concordance (uvcgpu_region_family_concordance; the definitions are in uvcgpu.h).  The votes of a unit at a position
// are stored nowhere once P4 has taken their consensus, so the report evaluates them again with the generic per-position form
// (unit_counts), as the haplotype links above do: off the accumulate path, only for the positions inside the caller's ranges.
//   k_famconc_units: one wave per unit, a lane per position of a 64-position window of its span, the waves of the grid striding over ALL
//     units in unit order (neighbouring waves read neighbouring fragments).  Lone single-fragment units take the same grid: they too need
//     the fragment's consensus symbol at every position, so a kernel of their own would save no evaluation.
//   k_famconc_duplex: one lane per (duplex family, position) of the work list of k_duplex (dup_units, dup_off, the same binary search).
// Both tally into a block's LDS copy of the row (11 432 B beside 14 336 B of vote counters): +1 words through merge_add / count_lanes, the
// vote sums through famconc_add, which sums the lanes of equal cell first.  A block flushes its non-zero words into one of `shards` global
// copies, uvc_launch_sum_fold adds the copies: 64-bit integer adds only, the same bits from call to call.
// ------------------------------------------------------------------------------------------------
namespace {
enum {
#define UVC_FAMCONC(name, first, words) FCROW_##name,
#include "uvc_famconcord.def"
#undef UVC_FAMCONC
    FCROW_N
};
static_assert(FCROW_N == UVC_NFAMCONC, "include/uvc_famconcord.def and UvcFamConc of uvcgpu.h list the same sections");
#define UVC_FAMCONC(name, first, words) static_assert((int)FCROW_##name == (int)UVC_FAMCONC_##name, "uvc_famconcord.def order = UvcFamConc order");
#include "uvc_famconcord.def"
#undef UVC_FAMCONC
constexpr UvcSection FC_SECTIONS[UVC_NFAMCONC] = {
#define UVC_FAMCONC(name, first, words) { #name, first, words },
#include "uvc_famconcord.def"
#undef UVC_FAMCONC
};
static_assert(uvc_sections_tile(FC_SECTIONS, UVC_FAMCONC_ROW), "the sections of uvc_famconcord.def tile the row");
#define FC_BASE_VOTES (UVC_FAMCONC_NBASE + 1)   // a strand's BASE vote in the duplex pass: A..NN or none
#define FC_LINK_VOTES (UVC_FAMCONC_NLINK + 1)
static_assert(FC_SECTIONS[UVC_FAMCONC_base].first == UVC_FAMCONC_BASE && FC_SECTIONS[UVC_FAMCONC_base].words == 2 * UVC_FAMCONC_NBIN * UVC_FAMCONC_NBASE * UVC_FAMCONC_NBASE
              && FC_SECTIONS[UVC_FAMCONC_base_pos].first == UVC_FAMCONC_BASE_POS && FC_SECTIONS[UVC_FAMCONC_base_pos].words == 2 * UVC_FAMCONC_NBIN * 2
              && FC_SECTIONS[UVC_FAMCONC_link].first == UVC_FAMCONC_LINK && FC_SECTIONS[UVC_FAMCONC_link].words == UVC_FAMCONC_NBIN * UVC_FAMCONC_NLINK * UVC_FAMCONC_NLINK
              && FC_SECTIONS[UVC_FAMCONC_link_pos].first == UVC_FAMCONC_LINK_POS && FC_SECTIONS[UVC_FAMCONC_link_pos].words == UVC_FAMCONC_NBIN * 2
              && FC_SECTIONS[UVC_FAMCONC_dup_base].first == UVC_FAMCONC_DUP_BASE && FC_SECTIONS[UVC_FAMCONC_dup_base].words == 4 * FC_BASE_VOTES * FC_BASE_VOTES
              && FC_SECTIONS[UVC_FAMCONC_dup_link].first == UVC_FAMCONC_DUP_LINK && FC_SECTIONS[UVC_FAMCONC_dup_link].words == FC_LINK_VOTES * FC_LINK_VOTES
              && FC_SECTIONS[UVC_FAMCONC_counters].first == UVC_FAMCONC_COUNTERS && FC_SECTIONS[UVC_FAMCONC_counters].words == UVC_NFAMCONCC,
              "the offsets and sizes of uvcgpu.h are those of uvc_famconcord.def");
static_assert(UVC_BASE_NN - UVC_BASE_A + 1 == UVC_FAMCONC_NBASE && UVC_LINK_NN - UVC_LINK_M + 1 == UVC_FAMCONC_NLINK && UVC_BASE_A == 0, "the symbols of the two types are A..NN and LINK_M..LINK_NN");

#define FC_MAX_SHARDS 16
#define FC_MAX_BLOCKS 2048   // k_famconc_units: resident blocks of four waves that stride over the units (each flushes its row once)
#define FC_MAX_STEPS 16      // k_famconc_duplex: groups of 256 cells a block tallies before it flushes

// Is plane index x inside one of the caller's ranges?  g keeps the range of the last hit (its first plane index x0, its length next -
// first): a lane walks up its unit, so most questions end at the first line.  Any lane alone.
DEV bool famconc_in_range(UvcRangeCursor &g, const UvcRangeRow *tab, int n_ranges, int x) {
    if (g.rid >= 0 && x >= g.x0 && x < g.x0 + (g.next - g.first)) return true;
    int lo = 0, hi = n_ranges;   // the last range that begins at or in front of x (the ranges ascend)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tab[mid].x0 <= x) lo = mid; else hi = mid; }
    const int x0 = tab[lo].x0, first = tab[lo].first, next = tab[lo + 1].first;
    if (x < x0 || x >= x0 + (next - first)) return false;
    g.rid = lo; g.x0 = x0; g.first = first; g.next = next;
    return true;
}
DEV int famconc_bin(int ct) { return ct <= 4 ? ct - 1 : (ct < 8 ? 4 : (ct < 16 ? 5 : (ct < 32 ? 6 : 7))); }   // 1, 2, 3, 4, 5-7, 8-15, 16-31, 32+
// tab[key] += v for every lane with `on`, the lanes of equal key summed first (merge_add with a value): one round per distinct key among
// the lanes, its first lane adds the sum.  Called by the whole wave, tab wave-uniform.
DEV void famconc_add(unsigned long long *tab, int key, int v, bool on, int lane) {
    unsigned long long left = __ballot(on);
    while (left) {
        const int lead = __ffsll((long long)left) - 1;
        const int k = __shfl(key, lead);
        const bool mine = (on && key == k);
        const unsigned long long same = __ballot(mine);
        const int sum = wave_sum(mine ? v : 0);
        if (lane == lead) lds_add(tab + k, (unsigned long long)sum);
        left &= ~same;
    }
}
DEV void famconc_flush(const unsigned long long *row, int tid, int shards, unsigned long long *out) {
    unsigned long long *dst = out + (size_t)(blockIdx.x % (unsigned)shards) * UVC_FAMCONC_ROW;
    for (int j = tid; j < UVC_FAMCONC_ROW; j += 256) { const unsigned long long v = row[j]; if (v) atomicAdd(dst + j, v); }
}

__global__ void __launch_bounds__(256) k_famconc_units(RegionDev R, UvcParams P, const UvcRangeRow *tab, int n_ranges, int shards, unsigned long long *out) {
    __shared__ unsigned long long row[UVC_FAMCONC_ROW];
    __shared__ int con_s[NSYM][256];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int j = tid; j < UVC_FAMCONC_ROW; j += 256) row[j] = 0;
    __syncthreads();
    const LdsCounts<256> con = { &con_s[0][tid] };
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const int x_lo = tab[0].x0, x_hi = tab[n_ranges - 1].x0 + (tab[n_ranges].first - tab[n_ranges - 1].first);   // no range reaches outside [x_lo, x_hi)
    unsigned long long *ctr = row + UVC_FAMCONC_COUNTERS;
    UvcRangeCursor g;
    for (int ui = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(tid >> 6); ui < R.n_fs; ui += (int)gridDim.x * 4) {   // wave-uniform: the unit record is a scalar load
        const FsRec u = R.fss[ui];
        if (u.end <= u.beg || u.end - R.beg <= x_lo || u.beg - R.beg >= x_hi) continue;
        for (int i0 = 0; i0 < u.end - u.beg; i0 += 64) {
            const int p = u.beg + i0 + lane, x = p - R.beg;
            const bool act = (p < u.end && x >= 0 && (int64_t)x < R.npos && famconc_in_range(g, tab, n_ranges, x));
            if (__ballot(act) == 0) continue;
            if (act) unit_counts<false>(R, P, u, p, proton, con, con);
            count_lanes(ctr + UVC_FAMCONCC_unit_positions, act, lane);
            count_lanes(ctr + UVC_FAMCONCC_units_seen, act && p == u.beg, lane);
            // reference symbols exist for plane indices 0 .. npos - 2 (the region's last position, `end`, has no reference base)
            const int ref = ((act && (int64_t)x < R.npos - 1) ? (int)R.refsym[x] : UVC_BASE_N);
            {   // BASE
                int cs = 0, cc = 0, ct = 0;
                if (act) fill_consensus(con, cs, cc, ct, UVC_BASE_SYMBOL, false, false);
                count_lanes(ctr + UVC_FAMCONCC_base_no_vote, act && ct == 0, lane);
                const bool voted = (act && ct > 0), on = (voted && ref <= UVC_BASE_T);
                count_lanes(ctr + UVC_FAMCONCC_base_no_ref, voted && !on, lane);
                const int cell = (on ? ((cs == ref ? 0 : 1) * UVC_FAMCONC_NBIN + famconc_bin(ct)) : 0);
                for (int s = 0; s < UVC_FAMCONC_NBASE; s++) {
                    const int v = (on ? con[UVC_BASE_A + s] : 0);
                    famconc_add(row + UVC_FAMCONC_BASE, (cell * UVC_FAMCONC_NBASE + (on ? cs : 0)) * UVC_FAMCONC_NBASE + s, v, v != 0, lane);
                }
                merge_add(row + UVC_FAMCONC_BASE_POS, cell * 2, on, lane);
                merge_add(row + UVC_FAMCONC_BASE_POS, cell * 2 + 1, on && cc == ct, lane);
            }
            {   // LINK
                int cs = UVC_LINK_M, cc = 0, ct = 0;
                if (act) fill_consensus(con, cs, cc, ct, UVC_LINK_SYMBOL, false, false);
                count_lanes(ctr + UVC_FAMCONCC_link_no_vote, act && ct == 0, lane);
                const bool on = (act && ct > 0);
                const int cell = (on ? famconc_bin(ct) : 0);
                for (int s = 0; s < UVC_FAMCONC_NLINK; s++) {
                    const int v = (on ? con[UVC_LINK_M + s] : 0);
                    famconc_add(row + UVC_FAMCONC_LINK, (cell * UVC_FAMCONC_NLINK + (on ? cs - UVC_LINK_M : 0)) * UVC_FAMCONC_NLINK + s, v, v != 0, lane);
                }
                merge_add(row + UVC_FAMCONC_LINK_POS, cell * 2, on, lane);
                merge_add(row + UVC_FAMCONC_LINK_POS, cell * 2 + 1, on && cc == ct, lane);
            }
        }
    }
    __syncthreads();
    famconc_flush(row, tid, shards, out);
}

__global__ void __launch_bounds__(256) k_famconc_duplex(RegionDev R, UvcParams P, const UvcRangeRow *tab, int n_ranges, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_work,
                                                        int steps, int shards, unsigned long long *out) {
    __shared__ unsigned long long row[UVC_FAMCONC_ROW];
    __shared__ int con_s[NSYM][256];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int j = tid; j < UVC_FAMCONC_ROW; j += 256) row[j] = 0;
    __syncthreads();
    const LdsCounts<256> con = { &con_s[0][tid] };
    const bool proton = (UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform);
    const bool padded_ignored = (P.microadjust_padded_deletion_flag & (proton ? 0x2 : 0x1)) != 0;
    unsigned long long *ctr = row + UVC_FAMCONC_COUNTERS;
    UvcRangeCursor g;
    for (int c = 0; c < steps; c++) {
        const int64_t w0 = ((int64_t)blockIdx.x * steps + c) * 256 + (tid & ~63);   // the wave's first cell of this step: wave-uniform
        if (w0 >= n_work) break;
        const int64_t w = w0 + lane;
        bool act = (w < n_work);
        int vb[2] = { UVC_FAMCONC_NBASE, UVC_FAMCONC_NBASE }, vl[2] = { UVC_FAMCONC_NLINK, UVC_FAMCONC_NLINK };   // the two strands' votes: none
        int ref = 0;
        if (act) {
            int lo = 0, hi = n_dup;   // k_duplex's search: the last family whose first cell is <= w
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (dup_off[mid] <= w) lo = mid; else hi = mid; }
            const FsRec u0 = R.fss[dup_units[lo]];   // the strand-0 unit of the family
            const FsRec u1 = R.fss[u0.other_fs];
            const int p = imin(u0.beg, u1.beg) + (int)(w - dup_off[lo]), x = p - R.beg;
            act = (x >= 0 && (int64_t)x < R.npos && famconc_in_range(g, tab, n_ranges, x));
            if (act) {
                ref = ((int64_t)x < R.npos - 1 ? (int)R.refsym[x] : UVC_BASE_N);
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const FsRec &u = (k == 0 ? u0 : u1);
                    if (p < u.beg || p >= u.end) continue;
                    unit_counts<false>(R, P, u, p, proton, con, con);
                    int cs, cc, ct;
                    fill_consensus(con, cs, cc, ct, UVC_BASE_SYMBOL, false, padded_ignored);
                    if (imax(cc * 2, ct) - ct >= 1) vb[k] = cs - UVC_BASE_A;
                    fill_consensus(con, cs, cc, ct, UVC_LINK_SYMBOL, false, false);
                    if (imax(cc * 2, ct) - ct >= 1) vl[k] = cs - UVC_LINK_M;
                }
            }
        }
        const bool none_b = (vb[0] == UVC_FAMCONC_NBASE && vb[1] == UVC_FAMCONC_NBASE), none_l = (vl[0] == UVC_FAMCONC_NLINK && vl[1] == UVC_FAMCONC_NLINK);
        count_lanes(ctr + UVC_FAMCONCC_duplex_no_vote, act && none_b, lane);
        count_lanes(ctr + UVC_FAMCONCC_duplex_no_vote, act && none_l, lane);
        const bool on_b = (act && !none_b && ref <= UVC_BASE_T);
        count_lanes(ctr + UVC_FAMCONCC_duplex_base_no_ref, act && !none_b && !on_b, lane);
        merge_add(row + UVC_FAMCONC_DUP_BASE, on_b ? ((ref * FC_BASE_VOTES + vb[0]) * FC_BASE_VOTES + vb[1]) : 0, on_b, lane);
        merge_add(row + UVC_FAMCONC_DUP_LINK, vl[0] * FC_LINK_VOTES + vl[1], act && !none_l, lane);
    }
    __syncthreads();
    famconc_flush(row, tid, shards, out);
}
}   // namespace

extern "C" const char *uvc_famconcord_section_name(int id) { return (id >= 0 && id < UVC_NFAMCONC) ? FC_SECTIONS[id].name : nullptr; }
extern "C" int64_t uvc_famconcord_scratch_cells(void) { return (int64_t)FC_MAX_SHARDS * UVC_FAMCONC_ROW; }
extern "C" void uvc_launch_famconcord(const RegionDev *R, const UvcParams *P, const UvcRangeRow *d_tab, int n_ranges, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_dup_work,
                                      long long *d_out, long long *d_scratch, UvcProf *prof, hipStream_t s) {
    if (n_ranges <= 0) return;
    const long long blocks_u = (R->n_fs > 0 ? std::min<long long>(FC_MAX_BLOCKS, ((long long)R->n_fs + 3) / 4) : 0);
    // a block of the duplex kernel keeps its row over `steps` groups of 256 cells: fewer flushes, as long as 1 024 blocks stay to fill the machine
    const bool duplex = (n_dup > 0 && n_dup_work > 0);
    const int steps = (int)std::max<int64_t>(1, std::min<int64_t>(FC_MAX_STEPS, n_dup_work / (256 * 1024)));
    const long long blocks_d = (duplex ? (n_dup_work + 256LL * steps - 1) / (256LL * steps) : 0);
    // from 128 blocks on the row is sharded (the flushes meet on the same 1 429 words), at most 16 copies
    const int shards = (int)std::max<long long>(1, std::min<long long>(FC_MAX_SHARDS, std::max(blocks_u, blocks_d) / 64));
    unsigned long long *d_parts = (unsigned long long *)(shards > 1 ? d_scratch : d_out);
    hipMemsetAsync(d_parts, 0, sizeof(unsigned long long) * (size_t)shards * UVC_FAMCONC_ROW, s);
    {
        const int pi = uvc_prof_begin(prof, "k_famconc_units", s);
        if (blocks_u > 0) hipLaunchKernelGGL(k_famconc_units, dim3((unsigned)blocks_u), dim3(256), 0, s, *R, *P, d_tab, n_ranges, shards, d_parts);
        uvc_prof_end(prof, pi, s);
    }
    {
        const int pi = uvc_prof_begin(prof, "k_famconc_duplex", s);   // with the fold of the copies
        if (blocks_d > 0) hipLaunchKernelGGL(k_famconc_duplex, dim3((unsigned)blocks_d), dim3(256), 0, s, *R, *P, d_tab, n_ranges, dup_units, n_dup, dup_off, n_dup_work, steps, shards, d_parts);
        if (shards > 1) uvc_launch_sum_fold(d_scratch, shards, UVC_FAMCONC_ROW, d_out, s);
        uvc_prof_end(prof, pi, s);
    }
}

static inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }
static inline int imin_h(int a, int b) { return a < b ? a : b; }

// optional per-kernel HIP-event timing on the stream `s` of the place of use (uvc_prof_begin / uvc_prof_end of uvc_launch.h, bench.py roofline leg)
#define TIMED(prof, kname, ...) do { \
        UvcProf *p_ = (prof); const int i_ = uvc_prof_begin(p_, kname, s); \
        __VA_ARGS__; \
        uvc_prof_end(p_, i_, s); \
    } while (0)

// apply_bq_err_correction3 (grouping.cpp:459-543): quality increment and cap, tail penalty behind a long soft clip / homopolymer at
// the 3' end, and the poly-G penalty.  One thread per alignment; the base codes are mapped to the BAM 4-bit codes the reference
// compares (A=1, C=2, G=4, T=8, N=15; "no base yet" = 0).
__global__ void __launch_bounds__(256) k_correct_bq(RegionDev R, int bq_max, int bq_inc) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= R.n_alns) return;
    const AlnRec &a = R.alns[id];
    const int l = a.l_qseq;
    if (0 == l || (a.flag & 0x4)) return;
    uint8_t *q = (uint8_t *)R.quals + a.seq_off;
    const uint8_t *b = R.bases + a.seq_off;
    const uint32_t *cigar = R.cigars + a.cigar_off;
    auto code = [&](int i) -> int { const int v = b[i]; return v < 4 ? (1 << v) : 15; };
    for (int i = 0; i < l; i++) q[i] = (uint8_t)imin((int)q[i] + bq_inc, bq_max);
    const int isrc = ((a.flag & 0x10) ? 1 : 0);
    int inclu_beg_poss[2] = { 0, l - 1 };
    int exclu_end_poss[2] = { l, 0 - 1 };
    int end_clip_len = 0;
    if (a.n_cigar > 0) {
        uint32_t c1 = cigar[0];
        if (cig_op(c1) == C_SOFT_CLIP) {
            if (0 == isrc) inclu_beg_poss[0] += cig_len(c1);
            else { exclu_end_poss[1] += cig_len(c1); end_clip_len = cig_len(c1); }
        }
        c1 = cigar[a.n_cigar - 1];
        if (cig_op(c1) == C_SOFT_CLIP) {
            if (1 == isrc) inclu_beg_poss[1] -= cig_len(c1);
            else { exclu_end_poss[0] -= cig_len(c1); end_clip_len = cig_len(c1); }
        }
    }
    const int inc = (isrc ? -1 : 1), ibeg = inclu_beg_poss[isrc], eend = exclu_end_poss[isrc];
    // a read whose soft clips leave no aligned base would send the reference's loops out of the arrays (undefined there): skip it
    if ((isrc ? (ibeg <= eend) : (ibeg >= eend)) || ibeg < 0 || ibeg >= l || eend < -1 || eend > l) return;
    {
        int prev_b = 0, distinct_cnt = 0;
        int termpos = eend - inc;
        for (; termpos != ibeg - inc; termpos -= inc) {
            const int bb = code(termpos), qq = q[termpos];
            if (bb != prev_b && qq >= 20) { prev_b = bb; distinct_cnt += 1; if (2 == distinct_cnt) break; }
        }
        const int homopol_tracklen = abs(termpos - (eend - inc));
        const int tail_penal = (end_clip_len >= 20 ? 1 : 0) + (homopol_tracklen >= 15 ? 2 : (homopol_tracklen >= 10 ? 1 : 0));
        if (tail_penal > 0)
            for (int pos = eend - inc; pos != (ibeg - inc) && pos != termpos; pos -= inc) q[pos] = (uint8_t)(imax((int)q[pos], tail_penal + 1) - tail_penal);
    }
    {
        int homopol_len = 0, prev_b = 0;
        for (int pos = ibeg; pos != eend; pos += inc) {
            const int bb = code(pos);
            if (bb == prev_b) { homopol_len++; if (homopol_len >= 4 && bb == 4 /* G */) q[pos] = (uint8_t)(imax((int)q[pos], 1 + 1) - 1); }
            else { prev_b = bb; homopol_len = 1; }
        }
    }
}
extern "C" void uvc_launch_correct_bq(const RegionDev *R, int bq_max, int bq_inc, hipStream_t s) {
    if (R->n_alns) hipLaunchKernelGGL(k_correct_bq, dim3((unsigned)((R->n_alns + 255) / 256)), dim3(256), 0, s, *R, bq_max, bq_inc);
}

// (a base code above 4 is refused here, where the one-byte-per-base column enters: k_aln_bm compares eight bases per load and relies on every
// byte being below 0x80, the per-symbol tables index with the code)
__global__ void __launch_bounds__(256) k_pack_bq1(const uint8_t *bases, const uint8_t *quals, uint16_t *bq, int64_t n, int32_t *bad) {
    int any = 0, zero = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        bq[i] = (uint16_t)(bases[i] | (quals[i] << 8));
        any |= (bases[i] > 4); zero |= (quals[i] == 0);
    }
    if (bad && __any(any) && (threadIdx.x & 63) == 0) *bad = 2;
    if (bad && __any(zero) && (threadIdx.x & 63) == 0) bad[1] = 1;   // a quality byte of 0 (UvcPrepIn::zero_qual)
}
// eight read bases per thread: two 8-byte loads, one 16-byte store (a byte per thread ran at 1.7 TB/s of the 1.2 GB it moves)
__global__ void __launch_bounds__(256) k_pack_bq(const uint8_t *bases, const uint8_t *quals, uint16_t *bq, int64_t n, int32_t *bad) {
    const int64_t n8 = n >> 3;
    unsigned long long over = 0, zero = 0;   // bits 3..7 of any byte set <=> a code above 7; codes 5..7: bit 2 with bit 0 or 1
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long b = ((const unsigned long long *)bases)[i], q = ((const unsigned long long *)quals)[i];
        over |= (b & 0xF8F8F8F8F8F8F8F8ull) | (b & 0x0404040404040404ull & (((b | (b >> 1)) & 0x0101010101010101ull) << 2));
        zero |= (q - 0x0101010101010101ull) & ~q & 0x8080808080808080ull;   // bit 7 of a quality byte that is 0
        uint4 o;
        o.x = (uint32_t)((b & 0xFF) | ((q & 0xFF) << 8) | (((b >> 8) & 0xFF) << 16) | (((q >> 8) & 0xFF) << 24));
        o.y = (uint32_t)(((b >> 16) & 0xFF) | (((q >> 16) & 0xFF) << 8) | (((b >> 24) & 0xFF) << 16) | (((q >> 24) & 0xFF) << 24));
        o.z = (uint32_t)(((b >> 32) & 0xFF) | (((q >> 32) & 0xFF) << 8) | (((b >> 40) & 0xFF) << 16) | (((q >> 40) & 0xFF) << 24));
        o.w = (uint32_t)(((b >> 48) & 0xFF) | (((q >> 48) & 0xFF) << 8) | (((b >> 56) & 0xFF) << 16) | (((q >> 56) & 0xFF) << 24));
        ((uint4 *)bq)[i] = o;
    }
    if (blockIdx.x == 0) for (int64_t i = (n8 << 3) + threadIdx.x; i < n; i += blockDim.x) { bq[i] = (uint16_t)(bases[i] | (quals[i] << 8)); over |= (bases[i] > 4); zero |= (quals[i] == 0); }   // the last n % 8
    if (bad && __any(over != 0) && (threadIdx.x & 63) == 0) *bad = 2;
    if (bad && __any(zero != 0) && (threadIdx.x & 63) == 0) bad[1] = 1;   // (UvcPrepIn::zero_qual)
}
extern "C" void uvc_launch_pack_bq(const uint8_t *bases, const uint8_t *quals, uint16_t *bq, int64_t n, int32_t *bad, hipStream_t s) {
    if (n <= 0) return;
    // the wide form needs 8- / 16-byte aligned columns (device allocations are; a caller's sub-array of set_reads_device may not be)
    const bool aligned = !(((uintptr_t)bases | (uintptr_t)quals) & 7) && !((uintptr_t)bq & 15);
    if (getenv("UVCGPU_TIMING")) fprintf(stderr, "[uvcgpu pack_bq] %s\n", aligned ? "k_pack_bq" : "k_pack_bq1");
    if (aligned) hipLaunchKernelGGL(k_pack_bq, dim3((unsigned)std::min<int64_t>(((n >> 3) + 255) / 256 + 1, 16384)), dim3(256), 0, s, bases, quals, bq, n, bad);
    else hipLaunchKernelGGL(k_pack_bq1, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, s, bases, quals, bq, n, bad);
}
extern "C" void uvc_launch_build_p2list(const RegionDev *R, const int32_t *fast_rank, const int32_t *aln, const int32_t *cbeg, const int32_t *cend, const int32_t *qb, hipStream_t s) {
    if (R->n_fast2) hipLaunchKernelGGL(k_build_p2list, dim3(nblk(R->n_fast2, 256)), dim3(256), 0, s, *R, fast_rank, aln, cbeg, cend, qb);
}
extern "C" void uvc_launch_prelude(const RegionDev *R, const RawReads *W, const UvcParams *P, hipStream_t s) {
    if (R->n_alns && R->n_fast) hipLaunchKernelGGL(k_aln_bm, dim3(imin_h((int)nblk(R->n_alns, 256), 16384)), dim3(256), 0, s, *R, *W);
    if (R->n_alns) hipLaunchKernelGGL(k_aln_prelude, dim3(nblk(R->n_alns, 256)), dim3(256), 0, s, *R, *W, *P);
}
// The sequential, low-occupancy kernels of the InDel reads and the per-fragment statistics need P1 / P1b only, not P2: they run on
// a side stream underneath the two issue-bound P2 kernels and join before anything reads their outputs.
#define TIMED2(prof, kname, ...) do { hipStream_t s = s2; TIMED(prof, kname, __VA_ARGS__); } while (0)
#define TIMED3(prof, kname, ...) do { hipStream_t s = s3; TIMED(prof, kname, __VA_ARGS__); } while (0)
// Zero fill of the plane slab in front of an accumulate, without the parts the last accumulate did not write (RegionDev::dirty): a block
// per (plane, block of 4 096 positions).  A 1 Mb tile's slab is 5.6 KB per position; what every tile writes (the per-position planes, the
// planes of A C G T N and LINK_M) is 2.5 KB of it, the rest a few per cent.
__global__ void __launch_bounds__(256) k_zero_state(char *slab, const ZeroPlane *planes, const uint8_t *dirty, int ndblk, int64_t npos) {
    const ZeroPlane zp = planes[blockIdx.x];
    const int b = (int)blockIdx.y;
    if (zp.fam >= 0 && !dirty[((size_t)zp.fam * NSYM + zp.sym) * ndblk + b]) return;
    const int64_t x0 = (int64_t)b << UVC_DIRTY_SHIFT, x1 = (x0 + ((int64_t)1 << UVC_DIRTY_SHIFT) < npos ? x0 + ((int64_t)1 << UVC_DIRTY_SHIFT) : npos);
    char *p0 = slab + zp.off + x0 * zp.elem, *p1 = slab + zp.off + x1 * zp.elem;
    char *a0 = (char *)(((uintptr_t)p0 + 15) & ~(uintptr_t)15), *a1 = (char *)((uintptr_t)p1 & ~(uintptr_t)15);
    if (a0 >= a1) { for (char *q = p0 + threadIdx.x; q < p1; q += 256) *q = 0; return; }
    for (char *q = p0 + threadIdx.x; q < a0; q += 256) *q = 0;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (uint4 *q = (uint4 *)a0 + threadIdx.x; q < (uint4 *)a1; q += 256) *q = z;
    for (char *q = a1 + threadIdx.x; q < p1; q += 256) *q = 0;
}
extern "C" void uvc_launch_zero_state(char *slab, const ZeroPlane *planes, int n_planes, uint8_t *dirty, int ndblk, int64_t npos, hipStream_t s) {
    if (n_planes <= 0 || ndblk <= 0) return;
    hipLaunchKernelGGL(k_zero_state, dim3((unsigned)n_planes, (unsigned)ndblk), dim3(256), 0, s, slab, planes, dirty, ndblk, npos);
}
// uvcgpu_region_check_presence, second half: a (family, symbol, block) that is not marked holds only zeros
__global__ void __launch_bounds__(256) k_check_dirty(RegionDev R, unsigned long long *n_bad) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = (int)blockIdx.y;
    if (x >= R.npos) return;
    const int b = (int)(x >> UVC_DIRTY_SHIFT);
    long long any[UVC_N_DIRTY_FAMILIES] = { 0, 0, 0 };   // the cells of (s, x) in the groups of each plane family, OR-ed
#define X(g, m) { constexpr int fill = UVC_GROUPS[UVC_F_##g].fill; \
                  if (fill >= 0) for (int pl = 0; pl < uvc_group_sym_planes(UVC_F_##g); pl++) any[fill >= 0 ? fill : 0] |= R.m[((size_t)pl * NSYM + s) * R.npos + x]; }
    UVC_SLAB_MEMBERS(X)
#undef X
    int bad = 0;
    for (int fam = 0; fam < UVC_N_DIRTY_FAMILIES; fam++)
        if (any[fam] && !(fam == UVC_FILL_CORE && sym_always_filled(s)) && !R.dirty[((size_t)fam * NSYM + s) * R.ndblk + b]) bad++;
    if (bad) atomicAdd(n_bad, (unsigned long long)bad);
}
extern "C" void uvc_launch_check_dirty(const RegionDev *R, unsigned long long *d_n_bad, hipStream_t s) {
    hipLaunchKernelGGL(k_check_dirty, dim3((unsigned)((R->npos + 255) / 256), NSYM), dim3(256), 0, s, *R, d_n_bad);
}

// The form each pass of the accumulate takes: decided once from the tile's shape, the parameters and the families' flags, then printed
// (UVCGPU_TIMING) and launched from the same flags.
struct AccForms { bool vcf, proton, split_windows, p2_plain, misq_p1, frag_plain, h16, fam, digest, duplex; int n_gen; };
// UVCGPU_SPLIT is read on every accumulate; the handle remembers the answer for the completion passes that follow that accumulate
extern "C" int uvc_acc_split_windows(const RegionDev *R) {
    const char *sp_env = getenv("UVCGPU_SPLIT");
    const long long per_window = (long long)R->n_fast2 * (R->max_p2_span + 64) / (R->npos > 0 ? R->npos : 1);
    return (sp_env ? (atoi(sp_env) != 0) : (R->nwin < 4 * 1024 && per_window >= 1024)) ? 1 : 0;
}
// P2: no IonTorrent values, no amplicon-flagged family, no primer length, median read length at or above
// microadjust_median_readlen_thres: the specialisation without those arms
static bool p2_plain_form(const RegionDev *R, const UvcParams *P) {
    return UVC_PLATFORM_IONTORRENT != P->inferred_sequencing_platform && !R->any_amplicon && !(P->primerlen > 0 && !(0x2 & P->primer_flag)) && (P->central_readlen >= P->microadjust_median_readlen_thres);
}
// (the host forces UVCGPU_LINK=eager on the generic forms: their base pass does not carry the five cells of LINK_M)
extern "C" int uvc_acc_p2_plain(const RegionDev *R, const UvcParams *P) { return p2_plain_form(R, P) ? 1 : 0; }
static AccForms acc_forms(const RegionDev *R, const UvcParams *P, int n_dup) {
    AccForms F;
    F.vcf = (P->inferred_is_vcf_generated != 0);
    F.proton = (UVC_PLATFORM_IONTORRENT == P->inferred_sequencing_platform);
    // fewer windows than four per SIMD, and many reads on each (at least sixteen chunks of 64: at 300x a wave of the split form would get fewer
    // than two and pay its prologue for them -- twice as slow on the 1 Mb tile): a block per window in the kernels that can share a window's
    // reads among its waves (UVCGPU_SPLIT=0 / 1 forces)
    F.split_windows = (uvc_acc_split_windows(R) != 0);
    F.p2_plain = p2_plain_form(R, P);
    // The mismatch queue of k_p2_mism: P1 makes it for the plain P2 form, whose items are (read, position, base, quality + addend) -- all of it
    // in P1's registers; the generic forms need neighbouring qualities and the primer gate and keep the queue of their base pass.
    // UVCGPU_MISQ=p2 (read on every accumulate, like UVCGPU_SPLIT) keeps it in the plain base pass too; tests compare the two item by item.
    const char *mq_env = getenv("UVCGPU_MISQ");
    F.misq_p1 = F.vcf && F.p2_plain && !(mq_env && !strcmp(mq_env, "p2"));
    // P3: no IonTorrent values, no SSCS table cap, no padded deletions
    F.frag_plain = F.vcf && !F.proton && !(0x1 & P->fam_flag) && !(P->microadjust_padded_deletion_flag & 0x1);
    F.h16 = (R->max_frag_depth < 65536) && !R->frag32;   // two 16-bit bucket counters per LDS word
    F.fam = (R->n_generic_fs > 0);
    F.digest = (R->fam_digest != nullptr);              // set_reads chose the form of the family passes
    F.duplex = F.fam && F.vcf && n_dup;
    F.n_gen = F.proton ? R->n_frags : R->n_sweep;          // fragments of k_frag_generic: all of them on IonTorrent, else the sweep list
    return F;
}
// "none" where a pass is not launched (tests/test_gpu_kernel_forms.py parses this line)
static void print_forms(const AccForms &F) {
    fprintf(stderr, "[uvcgpu accumulate] forms prep=%s p2=%s%s frag=%s,%s,%s family=%s duplex=%s frag_generic=%s\n",
            !F.vcf ? "none" : F.split_windows ? "split" : "wave",
            !F.vcf ? "none" : F.split_windows ? "split" : "wave", !F.vcf ? "" : F.p2_plain ? ",plain" : ",generic",
            F.h16 ? "h16" : "b32", (F.split_windows && F.h16) ? "split" : "wave", F.frag_plain ? "plain" : "generic",
            !F.fam ? "none" : F.digest ? "digest" : "generic",
            !F.duplex ? "none" : F.digest ? "digest" : "generic",
            !F.n_gen ? "none" : F.proton ? "all" : "sweep");
    // who makes the mismatch queue (a line of its own: the keys of the forms line above are a closed set to its readers)
    fprintf(stderr, "[uvcgpu accumulate] misq=%s\n", !F.vcf ? "none" : F.misq_p1 ? "p1" : "p2");
}
// The P1 pass of the forms that are not split: k_prep_scan, or k_prep_fast<false> with UVCGPU_PREP=window (read on every accumulate, like
// UVCGPU_SPLIT; tests compare the two).
static bool prep_scan_wanted() {
    const char *e = getenv("UVCGPU_PREP");
    return !(e && !strcmp(e, "window"));
}
// k_prep_scan splits (int)(baq(p) - baq(apos) + 1) into two 32-bit differences against the BAQ value at the tile's first position; that is
// exact while no difference of two BAQ values at most one entry plus one tile apart reaches 2^30.  A position adds at most M / 10 to the
// prefix sums (k_rtr_tracks: the larger of the two increments, in its int arithmetic), so the bound holds for every read when
// (longest entry + PSCAN_TILE) * M / 10 + 2 < 2^30; indel_nonSTR_phred_per_base or indel_str_phred_per_region in the millions fail it and
// keep the window form.  (P is the handle's own parameter block, the one its BAQ prefix sums were made from: uvcgpu_region_accumulate and
// the region tracks of create / reset both pass &r->P.)
static bool prep_scan_exact(const RegionDev *R, const UvcParams *P) {
    const long long m_str = llabs((long long)(int32_t)((uint32_t)P->indel_str_phred_per_region * 10u)) + 1;
    const long long m_non = llabs((long long)(int32_t)((uint32_t)P->indel_nonSTR_phred_per_base * 10u));
    const long long m = (m_str > m_non ? m_str : m_non);
    return ((long long)R->max_p2_span + PSCAN_TILE) * m / 10 + 2 < (1LL << 30);
}
// one pass of k_p2_fast over the P2 work list: the base symbols with the five cells of LINK_M that P3 reads (DO_B), or the completion pass of
// LINK_M (DO_L), a block per window (split) or a wave per window
// (queue: the plain base pass that makes the mismatch queue itself, misq=p2; the generic base pass always does)
template <bool DO_L, bool DO_B>
static void launch_p2_fast(const char *kname, bool split, bool plain, const RegionDev *R, const UvcParams *P, UvcProf *prof, hipStream_t s, bool queue = false) {
    const unsigned nwin = nblk(R->npos, 256);   // 4 waves x 64 positions per block
    if (queue && plain && split) TIMED(prof, kname, hipLaunchKernelGGL(k_p2_fast_split_q, dim3(R->nwin), dim3(256), 0, s, *R, *P));
    else if (queue && plain) TIMED(prof, kname, hipLaunchKernelGGL(k_p2_fast_q, dim3(nwin), dim3(256), 0, s, *R, *P));
    else if (split && plain) TIMED(prof, kname, hipLaunchKernelGGL((k_p2_fast_split<DO_L, DO_B, true>), dim3(R->nwin), dim3(256), 0, s, *R, *P));
    else if (split) TIMED(prof, kname, hipLaunchKernelGGL((k_p2_fast_split<DO_L, DO_B, false>), dim3(R->nwin), dim3(256), 0, s, *R, *P));
    else if (plain) TIMED(prof, kname, hipLaunchKernelGGL((k_p2_fast<DO_L, DO_B, true>), dim3(nwin), dim3(256), 0, s, *R, *P));
    else TIMED(prof, kname, hipLaunchKernelGGL((k_p2_fast<DO_L, DO_B, false>), dim3(nwin), dim3(256), 0, s, *R, *P));
}
// The bias counters of LINK_M beyond the five cells of the base pass are made where somebody reads them.  RegionDev::link_need
// says which 64-position windows a reader wants, link_done which ones the completion pass has been to; both are zeroed with the planes.
//   UVC_LINK_INDEL      windows with an InDel (or LINK_NN) mark in RegionDev::occ: the only LINK groups the default gate opens (gate_count)
//   UVC_LINK_POSITIONS  windows of the n_xs plane indices d_xs (out-of-range entries are skipped)
//   UVC_LINK_ALL        every window
// The pass adds to cells that k_p2_items may have added to, in either order; a window is run once.
// The position list is read in place: entry t is xs[t * xs_stride] - xs_off (the int32 sites of a request, or UvcTumorKey::refpos, a row apart).
// Whoever is the first to set a window's need byte (an atomic OR on its word) also lists the window for the sparse form of the pass, unless
// the pass has been there: a window is listed at most once between two fills of the marks, so link_list holds at most nwin entries.
__global__ void __launch_bounds__(256) k_link_mark(RegionDev R, const int32_t *xs, int64_t n_xs, int xs_stride, int xs_off) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int w = -1;
    if (xs) { if (t < n_xs) { const int64_t x = (int64_t)xs[t * xs_stride] - xs_off; if (x >= 0 && x < R.npos) w = (int)(x >> 6); } }
    else {   // the 64 positions of a wave are one window: one lane speaks for it
        const bool m = (t < R.npos && uvc_link_occ_marks(R.occ[t]));
        if (BAL(m) && (threadIdx.x & 63) == 0) w = (int)(t >> 6);
    }
    if (w < 0 || R.link_need[w]) return;
    const unsigned byte = 0xFFu << (8 * (w & 3));
    const unsigned old = atomicOr((unsigned *)R.link_need + (w >> 2), 0x01010101u & byte);
    if (!(old & byte) && !R.link_done[w]) { const int i = atomicAdd(R.link_cnt, 1); if (i < R.nwin) R.link_list[i] = w; }
}
// UVCGPU_LINK_FORM=wave|sparse (read on every call, like UVCGPU_SPLIT) forces the form of an INDEL or POSITIONS pass of the plain forms; tests
// and A/B runs compare the two.  UVC_LINK_ALL, UVCGPU_LINK=eager and the generic forms are throughput-bound and keep the wave / split forms.
static bool link_form_sparse(const RegionDev *R, const UvcParams *P, int scope, int64_t n_xs) {
    if (scope == UVC_LINK_ALL || !p2_plain_form(R, P)) return false;
    const char *e = getenv("UVCGPU_LINK_FORM");
    if (e && !strcmp(e, "wave")) return false;
    if (e && !strcmp(e, "sparse")) return true;
    return !(scope == UVC_LINK_POSITIONS && uvc_link_positions_dense(n_xs, R->nwin));
}
#ifndef UVC_LINK_SPARSE_NSL
#define UVC_LINK_SPARSE_NSL 4   // slices per class list: 4 * 4 = 16 waves per window
#endif
extern "C" void uvc_launch_link_complete(const RegionDev *R, const UvcParams *P, int split, int scope, const int32_t *d_xs, int64_t n_xs, int xs_stride, int xs_off,
                                         const char *kname, UvcProf *prof, hipStream_t s) {
    if (!P->inferred_is_vcf_generated) { hipMemsetAsync(R->link_done, 1, (size_t)R->nwin, s); return; }   // no P2 on a FASTQ-only run: the planes are complete as they are
    if (scope == UVC_LINK_ALL) hipMemsetAsync(R->link_need, 1, (size_t)R->nwin, s);
    else if (scope == UVC_LINK_POSITIONS) { if (n_xs <= 0) return; hipLaunchKernelGGL(k_link_mark, dim3(nblk(n_xs, 256)), dim3(256), 0, s, *R, d_xs, n_xs, xs_stride, xs_off); }
    else hipLaunchKernelGGL(k_link_mark, dim3(nblk(R->npos, 256)), dim3(256), 0, s, *R, (const int32_t *)nullptr, (int64_t)0, 1, 0);
    const bool sparse = link_form_sparse(R, P, scope, n_xs);
    if (getenv("UVCGPU_TIMING")) fprintf(stderr, "[uvcgpu link_form] scope=%s form=%s\n", scope == UVC_LINK_ALL ? "all" : scope == UVC_LINK_POSITIONS ? "positions" : "indel", sparse ? "sparse" : split ? "split" : "wave");
    // the sparse form: a fixed grid that strides over the list; the blocks beyond the device-side count leave at once
    if (sparse) TIMED(prof, kname, hipLaunchKernelGGL(k_p2_link_sparse<UVC_LINK_SPARSE_NSL>, dim3(imin_h(R->nwin, 1024)), dim3(256 * UVC_LINK_SPARSE_NSL), 0, s, *R, *P));
    else launch_p2_fast<true, false>(kname, split != 0, p2_plain_form(R, P), R, P, prof, s);
}

// The launches of one accumulate and what orders them (the same table: DESIGN 6-r7).  "reads": what another kernel of the accumulate writes;
// the reads' columns, the lists of set_reads and the region tracks are complete before the first launch.  Streams: M = the handle's stream,
// S2 = side, S3 = side3; without side streams everything is on M and the order of the launches below is the order of the rows.  An edge is
// either stream order or the event named in brackets.
//  #  launch                          on  reads (writer)                                            writes
//  1  k_win_index lists 1-4, 7        M   --                                                        window index of the work list / the generic units
//  2  k_prep_sums                     M   index 1-4 (1)                                             PREP: plain stores into zeroed planes
//  3  k_prep_slow                     S2  -- ; its atomics must follow the plain stores of 2        PREP (atomics), fragment event lists, clip events
//                                         [e_fork recorded behind 2]
//  4  k_prep_scan / k_prep_fast       M   index 1-4 (1); atomics behind the stores of 2             PREP (atomics), fragment event lists, clip events; misq=p1: the mismatch queue
//                                                                                                   (mis_cnt was zeroed on M in front of the accumulate: uvcgpu_region_accumulate)
//  5  k_thres                         M   PREP (2, 3 [e_join], 4)                                   THRES, RTR.indelphred
//     -- fork [e_fork]: S2 and S3 behind 5 --
//  6  k_p2_slow<true>  (walk)         S2  RTR.indelphred, THRES (5)                                 P2 items of the InDel reads
//  7  k_p2_slow<false> (table)        S3  RTR.indelphred (5)                                        contribution table, gap events
//  8  k_fragstat_fast                 S3  fragment event lists (3, 4)                               ffast / ffast_u (whole records), n_cov / n_near, overflow list
//  9  k_win_index lists 5-6           S3  ffast.beg (8)                                             window index of the fragments
// 10  k_fragstat_sweep, sweep list    S3  table (7); behind the record stores of 8                  n_cov / n_near of frags and ffast
// 11  k_fragstat_sweep, overflow      S3  overflow list and count (8), table (7)                    n_cov / n_near of frags and ffast
// 12  k_frag_sums                     S3  ffast with n_cov / n_near (8, 10, 11), index 5-6 (9)      fsum
// 13  k_p2_fast, base symbols         M   THRES, RTR.indelphred (5), index 1-4 (1)                  SEG32 / SEG64 / BQSUM / VQ a*BQ* of the reference symbol and the five cells of LINK_M
//                                                                                                   that rows 19 and 20 read (SEG32 aDP**, BQSUM): plain stores; misq=p2: the mismatch queue
// 14  k_p2_mism                       S2  THRES (5), misq=p1: the mismatch queue (4 [e_fork]), in front of 6;   SEG32 / SEG64 / BQSUM / VQ a*BQ* of the symbols that differ from the
//                                         misq=p2: the queue (13 [e_fork2]), behind 6 and 13                   reference (atomics), occ marks
// 15  (UVCGPU_LINK=eager only: row 23 with every window, here)
//     -- join: M behind 6 and 14 [e_join] and 12 [e_join3]; S2 behind 12 [e_join3] --
// 16  k_gap_keys .. k_gap_rows_fin    S2  gap events (7 [e_join3])                                  InDel allele tables; fam2_ins_len complete at [e_alleles]
// 17  k_fam_stat                      S3  table (7), ffast_u (8)                                    unit records (fss) -> [e_stat]
// 18  k_p2_items                      M   items (6 [e_join]), THRES (5); atomics behind the stores of 13   SEG32 / SEG64 / BQSUM / VQ a*BQ* (atomics)
//     -- fork [e_link_fork]: S3, behind 17 and its e_stat record, waits for M behind 18 (behind the join when there are no InDel reads) --
// 18a k_link_mark, LINK_M early       S3  occ (6 [e_join, e_link_fork]; marks of 19-21 as far as they exist)   link_need, link_list / link_cnt
// 18b k_p2_link_sparse, LINK_M early  S3  link_list (18a), THRES, RTR.indelphred (5), index 1-4 (1)  the other 34 cells of LINK_M in the listed windows, added to what 18 left there;
//                                                                                                   link_done -> [e_link_join]
// 19  k_frag_generic                  M   SEG32 aDP*, BQSUM (13, 14 [e_join], 18), table (7 [e_join3]), ffast, n_cov / n_near (8, 10, 11 [e_join3])
//                                                                                                   FRAG, FAM, VQ bMQ (atomics), global buckets
// 20  k_frag16 / k_frag               M   SEG32 aDP*, BQSUM (as 19), fsum (12 [e_join3]), ffast, index 5-6, global buckets (19)   FRAG, FAM, VQ b*, buckets
// 21  k_fam_p4* / k_fam_p5* / k_duplex*  M  unit records (17 [e_stat]), fam2_ins_len (16 [e_alleles]), table, ffast_u, index 7 (1)   FAM, family info planes, buckets
// 22  k_p5b                           M   buckets, p5flag (20, 21)                                  VQ, buckets cleared
//     -- M behind 16 [e_fork2, recorded again on S2: gap_tables, the MSI call and set_reads wait for this last record] and behind 18b [e_link_join] --
// 23  k_link_mark, LINK_M final       M   occ (6, 18-21), link_need / link_done (18a, 18b)          link_need, link_list of the windows whose mark appeared after 18a
//     k_p2_link_sparse / k_p2_fast    M   link_list (18a, 23), THRES, RTR.indelphred (5), index 1-4 (1)   the other 34 cells of LINK_M in those windows, added to what 18 left
//                                                                                                   there (load, add, store: no other writer of these cells runs); link_done
// Rows 19 and 20 read, per position, the aDP* and BQSUM sums that row 18 adds to: k_p2_items cannot run beside the fragment kernels.
// Row 14 need not follow row 13 (misq=p1 runs them beside each other): an item has sym != the reference symbol of its position, mis_apply adds to
// the cells of that symbol alone (seg_flush) and ORs its occ bit, and seg_store of row 13 stores into the cells of the reference symbol and
// into five cells of LINK_M, which is no base symbol: no cell has both writers.  Rows 18, 18a, 19 and 20 read or add to cells of row 14 and
// stay behind the join; 18a sees the occ marks of mis_apply.
// Row 3 cannot be forked in front of rows 1 and 2: a store of row 2 would overwrite what row 3 has added.
// Rows 18a / 18b may run beside rows 19 to 22: they write the 34 cells of LINK_M beyond aDP** / BQSUM, link_need, link_done and the list, none of
// which 19 to 22 read (19 and 20 read the five cells of row 13), and 19 to 22 write none of the 34 cells.  occ is read while 19 to 21 may still add
// marks to it: a mark 18a misses is found by row 23, a window either of them lists is run once (link_done).  Without side streams 18a / 18b run
// in launch order behind 18.
// Row 23 runs again, for more windows, in front of any later call that reads the bias counters of LINK_M elsewhere (link_complete, uvc_host.cpp).
extern "C" void uvc_launch_accumulate(const RegionDev *R, const UvcParams *P, int half_ratio_phred, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_dup_work,
                                      const UvcAccStreams *st, int link_eager, UvcProf *prof) {
    const hipStream_t s = st->s, side = st->side, side3 = st->side3;
    const hipEvent_t e_fork = st->e_fork, e_join = st->e_join, e_fork2 = st->e_fork2, e_join3 = st->e_join3, e_stat = st->e_stat, e_alleles = st->e_alleles;
    const hipEvent_t e_link_fork = st->e_link_fork, e_link_join = st->e_link_join;
    const unsigned nwin = nblk(R->npos, 256);   // 4 waves x 64 positions per block
    const AccForms F = acc_forms(R, P, n_dup);
    if (getenv("UVCGPU_TIMING")) { print_forms(F); fprintf(stderr, "[uvcgpu accumulate] link %s\n", link_eager ? "eager" : "lazy"); }
    if (prof) prof->n = 0;
    hipStream_t s2 = (side ? side : s);
    hipStream_t s3 = ((side && side3) ? side3 : s2);   // the two CIGAR walks of the InDel reads are independent, one wave per 64 reads and long: a stream each
    {   // the window index of the alignment lists (the fragment list's follows k_fragstat_fast, which writes it)
        const int64_t n = 2 * (int64_t)R->nwin * 4;
        TIMED(prof, "k_win_index", hipLaunchKernelGGL(k_win_index, dim3(nblk(n, 256)), dim3(256), 0, s, *R, 1, 5));
        if (R->n_generic_fs) hipLaunchKernelGGL(k_win_index, dim3(nblk(2 * (int64_t)R->nwin, 256)), dim3(256), 0, s, *R, 7, 8);
    }
    if (P->inferred_is_vcf_generated && R->n_fast) TIMED(prof, "k_prep_sums", hipLaunchKernelGGL(k_prep_sums, dim3(nblk(R->npos, PSUM_TILE)), dim3(256), 0, s, *R, *P));
    if (P->inferred_is_vcf_generated) {
        // P1: the InDel reads (one wave per read) underneath the position-centric pass; behind k_prep_sums, whose plain stores go to planes
        // that k_prep_slow adds to (row 3 of the table)
        if (side && R->n_complex) { hipEventRecord(e_fork, s); hipStreamWaitEvent(s2, e_fork, 0); }
        if (R->n_complex) TIMED2(prof, "k_prep_slow", hipLaunchKernelGGL(k_prep_slow, dim3(R->n_complex), dim3(64), 0, s, *R, *P));
        if (side && R->n_complex) hipEventRecord(e_join, s2);
        const bool scan = !F.split_windows && prep_scan_wanted() && prep_scan_exact(R, P);
        if (getenv("UVCGPU_TIMING")) fprintf(stderr, "[uvcgpu accumulate] prep kernel %s\n", F.split_windows ? "k_prep_fast<true>" : scan ? "k_prep_scan" : "k_prep_fast<false>");
        const int emit = F.misq_p1 ? 1 : 0;   // (RegionDev::mis_cnt was zeroed on this stream in front of the accumulate)
        if (F.split_windows) TIMED(prof, "k_prep_fast", hipLaunchKernelGGL(k_prep_fast<true>, dim3(R->nwin), dim3(256), 0, s, *R, *P, emit));
        else if (scan) TIMED(prof, "k_prep_scan", hipLaunchKernelGGL(k_prep_scan, dim3(nblk(R->npos, PSCAN_TILE)), dim3(256), 0, s, *R, *P, emit));
        else TIMED(prof, "k_prep_fast", hipLaunchKernelGGL(k_prep_fast<false>, dim3(nwin), dim3(256), 0, s, *R, *P, emit));
        if (side && R->n_complex) hipStreamWaitEvent(s, e_join, 0);
    }
    // P1b is part of updateByAlns3UsingBQ too (main.hpp:3691-3702): on a FASTQ-only run the thresholds stay zero and rtr.indelphred unedited
    if (P->inferred_is_vcf_generated) TIMED(prof, "k_thres", hipLaunchKernelGGL(k_thres, dim3(nblk(R->npos, 256)), dim3(256), 0, s, *R, *P, half_ratio_phred));
    if (side) { hipEventRecord(e_fork, s); hipStreamWaitEvent(s2, e_fork, 0); if (s3 != s2) hipStreamWaitEvent(s3, e_fork, 0); }
    // ---- the P2 phase (rows 6-15 of the table).  Neither side chain may be longer than the two passes of k_p2_fast on the main stream, and
    // no more should run beside them than that takes: a side kernel costs the pass it runs beside part of its own time.
    // s2: the queued mismatches, then the walk that produces the P2 items (misq=p2: the walk, then, behind the base pass, the mismatches the
    // pass has queued).  s3: the walk that fills the contribution table, then the per-fragment statistics, the fragment window index and the
    // interval sums (they need P1 / P1b only).
    // misq=p1: the queue is complete behind row 4, so k_p2_mism needs THRES only and runs beside the base pass, not behind it: on s2 in front
    // of the walk, where it ends long before the join (behind the walk and on the main stream were measured and are no shorter: DESIGN 6-r11)
    if (F.misq_p1) TIMED2(prof, "k_p2_mism", hipLaunchKernelGGL(k_p2_mism, dim3(2048), dim3(256), 0, s, *R, *P));
    if (P->inferred_is_vcf_generated && R->n_complex) TIMED2(prof, "k_p2_slow_walk", hipLaunchKernelGGL(k_p2_slow<true>, dim3(nblk(R->n_complex, 64)), dim3(64), 0, s, *R, *P));
    if (R->n_complex) TIMED3(prof, "k_p2_slow_table", hipLaunchKernelGGL(k_p2_slow<false>, dim3(nblk(R->n_complex, 64)), dim3(64), 0, s, *R, *P));
    TIMED3(prof, "k_fragstat_fast", hipLaunchKernelGGL(k_fragstat_fast, dim3(nblk(R->n_frags, 256)), dim3(256), 0, s, *R, *P));
    TIMED3(prof, "k_win_index_frag", hipLaunchKernelGGL(k_win_index, dim3(nblk(2 * (int64_t)R->nwin * 2, 256)), dim3(256), 0, s, *R, 5, 7));
    if (R->n_sweep) TIMED3(prof, "k_fragstat_sweep", hipLaunchKernelGGL(k_fragstat_sweep, dim3(R->n_sweep), dim3(64), 0, s, *R, *P, R->sweep_frags, (const int32_t *)nullptr, R->n_sweep));
    // fragments whose event list overflowed (device-side list; the grid covers the worst case up to 65 535 blocks, surplus blocks exit and the
    // blocks stride over a longer list; a smaller fixed grid was measured and moved nothing: DESIGN 6-r7)
    TIMED3(prof, "k_fragstat_overflow", hipLaunchKernelGGL(k_fragstat_sweep, dim3(imin_h(R->n_frags, 65535)), dim3(64), 0, s, *R, *P, (const int32_t *)R->overflow_frags, (const int32_t *)R->n_overflow, 0));
    if (UVC_PLATFORM_IONTORRENT != P->inferred_sequencing_platform)   // (there every fragment takes k_frag_generic)
        TIMED3(prof, "k_frag_sums", hipLaunchKernelGGL(k_frag_sums, dim3(nblk(R->npos, FSUM_TILE), 2), dim3(256), 0, s, *R, *P));
    // main stream: the base symbols.  misq=p2: the mismatches the pass queues (other symbols, atomics: disjoint from the cells the pass
    // stores to) are applied on a side stream behind it
    if (P->inferred_is_vcf_generated) {
        launch_p2_fast<false, true>("k_p2_fast_base", F.split_windows, F.p2_plain, R, P, prof, s, !F.misq_p1);
        if (!F.misq_p1) {   // misq=p2: the base pass has made the queue
            if (side) { hipEventRecord(e_fork2, s); hipStreamWaitEvent(s2, e_fork2, 0); }
            TIMED2(prof, "k_p2_mism", hipLaunchKernelGGL(k_p2_mism, dim3(2048), dim3(256), 0, s, *R, *P));
        }
    }
    if (link_eager) uvc_launch_link_complete(R, P, F.split_windows, UVC_LINK_ALL, nullptr, 0, 1, 0, "k_p2_fast_link", prof, s);   // UVCGPU_LINK=eager and the generic forms: where the LINK pass ran before 6-r8
    if (side) {
        hipEventRecord(e_join, s2); hipStreamWaitEvent(s, e_join, 0);
        if (s3 != s2) { hipEventRecord(e_join3, s3); hipStreamWaitEvent(s, e_join3, 0); hipStreamWaitEvent(s2, e_join3, 0); }   // (the allele tables below read the gap events of the table walk)
    }
    // InDel allele tables: they read the contribution table (side stream) and the reads only, so the pipeline stays on the side stream
    // underneath the fragment / family kernels; the main stream picks it up at the end
    const GapWork &G = R->gap;
    hipMemsetAsync(G.n_inc, 0, 16, s2);   // n_inc, n_rows, seq_len
    if (P->inferred_is_vcf_generated && G.n_ev > 0) {
        TIMED2(prof, "k_gap", {
            hipLaunchKernelGGL(k_gap_keys, dim3(nblk(G.n_ev, 256)), dim3(256), 0, s, *R);
            uvc_gap_sort(G.sort_tmp, G.sort_tmp_bytes, G.ckey, G.ckey_s, G.cval, G.cval_s, (size_t)G.n_ev, 58, s);
            hipMemsetAsync(G.ikey, 0xFF, sizeof(unsigned long long) * (size_t)G.inc_cap, s);
            hipLaunchKernelGGL(k_gap_alleles, dim3(nblk(G.n_ev, 64)), dim3(64), 0, s, *R, *P);
            if (side) hipEventRecord(e_alleles, s);   // what the family kernels read of this chain (fam2_ins_len) is complete here
            uvc_gap_sort(G.sort_tmp, G.sort_tmp_bytes, G.ikey, G.ikey_s, G.ival, G.ival_s, (size_t)G.inc_cap, 64, s);
            hipLaunchKernelGGL(k_gap_rows, dim3(nblk(G.inc_cap, 256)), dim3(256), 0, s, *R);
            hipLaunchKernelGGL(k_gap_rows_add, dim3(nblk(G.inc_cap, 256)), dim3(256), 0, s, *R);
            hipLaunchKernelGGL(k_gap_rows_fin, dim3(nblk(G.n_ev, 256)), dim3(256), 0, s, *R);   // (rows <= events)
        });
    }
    if (side && !(P->inferred_is_vcf_generated && G.n_ev > 0)) hipEventRecord(e_alleles, s2);
    // per-unit statistics of the generic family units (medians, first / last consensus position, general-kind flag): they need the contribution
    // table and the fragment records only: on s3 behind the interval sums, beside the allele tables on s2, underneath k_frag
    if (R->n_generic_fs) TIMED3(prof, "k_fam_stat", hipLaunchKernelGGL(k_fam_stat, dim3(nblk(R->n_generic_fs, 64)), dim3(64), 0, s, *R, *P));
    if (side) { hipEventRecord(e_stat, s3); hipEventRecord(e_fork2, s2); }
    if (P->inferred_is_vcf_generated && R->n_complex) TIMED(prof, "k_p2_items", hipLaunchKernelGGL(k_p2_items, dim3(R->n_complex), dim3(64), 0, s, *R, *P));
    // The completion pass of LINK_M, early phase (row 18a): the InDel marks of the CIGAR walk exist, and no kernel below writes the 34 cells or
    // reads them, so the pass runs on s3 underneath the fragment kernels.  Marks that appear later (rows 19-21) are left to the final phase.
    if (!link_eager) {
        if (side) { hipEventRecord(e_link_fork, s); hipStreamWaitEvent(s3, e_link_fork, 0); }
        uvc_launch_link_complete(R, P, F.split_windows, UVC_LINK_INDEL, nullptr, 0, 1, 0, "k_p2_link_early", prof, s3);
        if (side) hipEventRecord(e_link_join, s3);
        if (getenv("UVCGPU_TIMING")) {   // (diagnosis, like link_report of uvc_host.cpp: it waits, so a UVCGPU_TIMING run is no timing of the step)
            int n_early = 0;
            if (hipStreamSynchronize(s3) == hipSuccess && hipMemcpy(&n_early, R->link_cnt, sizeof(n_early), hipMemcpyDeviceToHost) == hipSuccess)
                fprintf(stderr, "[uvcgpu link_early] %d windows listed for the early phase, the rest of the total below for the final one\n", n_early);
        }
    }
    {
        if (F.n_gen) TIMED(prof, "k_frag_generic", hipLaunchKernelGGL(k_frag_generic, dim3(imin_h(F.n_gen, 1 << 20), imin_h((R->max_frag_span + 63) / 64, 16)), dim3(64), 0, s, *R, *P, F.proton ? (const int32_t *)nullptr : R->sweep_frags, F.n_gen));
    }
    {
        const bool plain = F.frag_plain;
        if (F.split_windows && F.h16 && plain) TIMED(prof, "k_frag", hipLaunchKernelGGL(k_frag16_split<true>, dim3(R->nwin), dim3(256), 0, s, *R, *P));
        else if (F.split_windows && F.h16) TIMED(prof, "k_frag", hipLaunchKernelGGL(k_frag16_split<false>, dim3(R->nwin), dim3(256), 0, s, *R, *P));
        else if (plain && F.h16) TIMED(prof, "k_frag", hipLaunchKernelGGL(k_frag16<true>, dim3(nwin), dim3(256), 0, s, *R, *P));
        else if (plain) TIMED(prof, "k_frag", hipLaunchKernelGGL(k_frag<true>, dim3(nwin), dim3(256), 0, s, *R, *P));
        else if (F.h16) TIMED(prof, "k_frag", hipLaunchKernelGGL(k_frag16<false>, dim3(nwin), dim3(256), 0, s, *R, *P));
        else TIMED(prof, "k_frag", hipLaunchKernelGGL(k_frag<false>, dim3(nwin), dim3(256), 0, s, *R, *P));
    }
    if (R->n_generic_fs) {
        if (side) { hipStreamWaitEvent(s, e_stat, 0); hipStreamWaitEvent(s, e_alleles, 0); }   // k_fam_stat's unit records; fam2_ins_len reads what k_gap_alleles left (both ran under k_frag)
        // shallow data: the generic form, one thread per (unit, position); deep data (many units per position, e.g. UMI panels): the digest
        // form, window kernels whose LDS collection removes most of the atomics that bound the per-thread form, and one walk over the
        // fragments of a unit instead of three.  set_reads chose the form: the digest is allocated for the second.
        if (F.digest) TIMED(prof, "k_fam_p4", { hipLaunchKernelGGL(k_fam_p4d, dim3(nblk(R->npos, 64)), dim3(256), 0, s, *R, *P);
                                               hipLaunchKernelGGL(k_fam_p4d_rest, dim3(R->n_generic_fs), dim3(64), 0, s, *R, *P); });
        else TIMED(prof, "k_fam_p4", hipLaunchKernelGGL(k_fam_p4, dim3(nblk(R->n_generic_work, 256)), dim3(256), 0, s, *R, *P));
        if (P->inferred_is_vcf_generated) {
            if (F.digest) TIMED(prof, "k_fam_p5", hipLaunchKernelGGL(k_fam_p5d, dim3(nblk(R->npos, 64)), dim3(256), 0, s, *R, *P));
            else TIMED(prof, "k_fam_p5", hipLaunchKernelGGL(k_fam_p5, dim3(nblk(R->n_generic_work, 256)), dim3(256), 0, s, *R, *P));
            if (F.duplex && F.digest) TIMED(prof, "k_duplex", hipLaunchKernelGGL(k_duplex_d, dim3(n_dup), dim3(64), 0, s, *R, dup_units, n_dup, dup_off, n_dup_work));
            else if (F.duplex) TIMED(prof, "k_duplex", hipLaunchKernelGGL(k_duplex, dim3(nblk(n_dup_work, 256)), dim3(256), 0, s, *R, *P, dup_units, n_dup, dup_off, n_dup_work));
        }
    }
    if (P->inferred_is_vcf_generated) TIMED(prof, "k_p5b", hipLaunchKernelGGL(k_p5b, dim3(nblk(R->npos * 2, 256)), dim3(256), 0, s, *R, *P));
    if (side) hipStreamWaitEvent(s, e_fork2, 0);   // the allele tables
    // every InDel mark of the accumulate exists here (rows 6, 18-21): the windows the default gate can open a LINK group in
    // (final phase, row 23: behind the early one, for the windows whose mark appeared after the fork)
    if (!link_eager) {
        if (side) hipStreamWaitEvent(s, e_link_join, 0);
        uvc_launch_link_complete(R, P, F.split_windows, UVC_LINK_INDEL, nullptr, 0, 1, 0, "k_p2_fast_link", prof, s);
    }
}

// ------------------------------------------------------------------------------------------------
// The scalar functions of this file on their own, for tests (the second half of uvc_launch_math_probe, uvc_kernels_score.hip): one thread
// per row, the argument and the result as doubles.  with_table: phred2prob_tab reads the table a block of k_fam_p5d builds.
__global__ void __launch_bounds__(256) k_math_probe_acc(int op, long long n, const double *in, int n_in, double *out, int n_out) {
    __shared__ double p2p_s[128];
    const bool with_table = (op == UVC_PROBE_phred2prob_tab);
    if (with_table) { for (int i = threadIdx.x; i < 128; i += 256) p2p_s[i] = phred2prob(i); __syncthreads(); }
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = (int)in[i * n_in];
    out[i * n_out] = (op == UVC_PROBE_proton_cigarlen2phred) ? (double)proton_cigarlen2phred(cig_len((uint32_t)v << 4)) :   // (a CIGAR length: 28 bits, as at the call sites)
                     phred2prob_tab(with_table ? p2p_s : nullptr, v);
}
extern "C" int uvc_launch_math_probe_acc(int op, int64_t n, const double *in, int n_in, double *out, int n_out, hipStream_t s) {
    if (op < UVC_PROBE_proton_cigarlen2phred || op >= UVC_PROBE_END || n < 1 || n > (1LL << 32) || n_in < 1 || n_out < 1 || !in || !out) return -1;
    hipLaunchKernelGGL(k_math_probe_acc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, op, (long long)n, in, n_in, out, n_out);
    return 0;
}
