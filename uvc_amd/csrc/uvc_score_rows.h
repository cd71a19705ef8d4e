// uvc_score_rows.h -- the staged rows of the scoring path (uvc_kernels_score.hip), each fact once: the cells a row block holds (TOT_LIST,
// AL_LIST and the small enums), the blocks themselves (SCORE_ROW_LIST) and the two memory layouts built from them (the scratch of a one-call
// score, the row set of a streamed chunk).  No memory access and no HIP type in here, so the same text compiles for the host alone
// (tests/native/score_layout_host_main.cpp sweeps the layouts there) and into the kernels' translation unit.
// To add a cell: one entry of TOT_LIST / AL_LIST.  To add a row block: one entry of SCORE_ROW_LIST and the pointer of that name in Stage
// (bind_rows does not compile without it); layout, binding and the bytes per record follow.
#ifndef UVC_SCORE_ROWS_H
#define UVC_SCORE_ROWS_H

#include <stddef.h>
#include <stdint.h>
#include "uvcgpu.h"

// plane groups of RegionDev a staged cell is fetched from (stage_cell)
enum { SG_PREP32 = 0, SG_PREP64, SG_SEG32, SG_SEG64, SG_VQ, SG_FRAG, SG_FAM, SG_FI32, SG_FI64, SG_DUP };

// symbol-type totals (fill_symboltype_fmt, main.hpp:3745-3793): X(name, plane group, plane, the int32 FORMAT field truncates the sum).
// Every total is stored as a 64-bit sum and read as one (TT_), but for the names of TOT_INT_LIST below.
#define TOT_LIST(X) \
    X(APDP0, SG_PREP32, UVC_P_a_dp, 0) X(APDP1, SG_PREP32, UVC_P_a_near_ins_dp, 0) X(APDP2, SG_PREP32, UVC_P_a_near_del_dp, 0) X(APDP3, SG_PREP32, UVC_P_a_near_RTR_ins_dp, 0) \
    X(APDP4, SG_PREP32, UVC_P_a_near_RTR_del_dp, 0) X(APDP5, SG_PREP32, UVC_P_a_pcr_dp, 0) X(APDP6, SG_PREP32, UVC_P_a_snv_dp, 0) X(APDP7, SG_PREP32, UVC_P_a_dnv_dp, 0) \
    X(APDP8, SG_PREP32, UVC_P_a_highBQ_dp, 0) X(APDP9, SG_PREP32, UVC_P_a_near_pcr_clip_dp, 0) X(APDP10, SG_PREP32, UVC_P_a_near_long_clip_dp, 0) X(APDP11, SG_PREP32, UVC_P_a_umi_dp, 0) \
    X(APXM0, SG_PREP32, UVC_P_a_XM1500, 0) X(APXM1, SG_PREP32, UVC_P_a_GO1500, 0) X(APXM2, SG_PREP32, UVC_P_a_qlen, 0) X(APXM3, SG_PREP32, UVC_P_a_GAPLEN, 0) \
    X(APXM4, SG_PREP64, UVC_P_a_near_ins_pow2len, 0) X(APXM5, SG_PREP64, UVC_P_a_near_del_pow2len, 0) X(APXM6, SG_PREP32, UVC_P_a_near_ins_inv100len, 0) X(APXM7, SG_PREP32, UVC_P_a_near_del_inv100len, 0) \
    X(APLRI0, SG_PREP64, UVC_P_a_LI, 0) X(APLRI1, SG_PREP32, UVC_P_a_LIDP, 0) X(APLRI2, SG_PREP64, UVC_P_a_RI, 0) X(APLRI3, SG_PREP32, UVC_P_a_RIDP, 0) \
    X(A1BQf0, SG_VQ, UVC_VQ_a1BQf, 1) X(A1BQr0, SG_VQ, UVC_VQ_a1BQr, 1) X(AMQs0, SG_SEG32, UVC_S_aMQs, 1) X(AP10, SG_SEG32, UVC_S_aP1, 1) X(AP20, SG_SEG32, UVC_S_aP2, 1) \
    X(ADPff0, SG_SEG32, UVC_S_aDPff, 1) X(ADPfr0, SG_SEG32, UVC_S_aDPfr, 1) X(ADPrf0, SG_SEG32, UVC_S_aDPrf, 1) X(ADPrr0, SG_SEG32, UVC_S_aDPrr, 1) \
    X(ALP10, SG_SEG32, UVC_S_aLP1, 1) X(ALP20, SG_SEG32, UVC_S_aLP2, 1) X(ALPL0, SG_SEG32, UVC_S_aLPL, 0) X(ARP20, SG_SEG32, UVC_S_aRP2, 1) X(ARPL0, SG_SEG32, UVC_S_aRPL, 0) \
    X(ALB20, SG_SEG32, UVC_S_aLB2, 1) X(ALBL0, SG_SEG64, UVC_S64_aLBL, 0) X(ARB20, SG_SEG32, UVC_S_aRB2, 1) X(ARBL0, SG_SEG64, UVC_S64_aRBL, 0) \
    X(ABQ20, SG_SEG32, UVC_S_aBQ2, 1) X(APF20, SG_SEG32, UVC_S_aPF2, 1) X(ALI20, SG_SEG32, UVC_S_aLI2, 1) X(ARIf0, SG_SEG32, UVC_S_aRIf, 1) X(ARI20, SG_SEG32, UVC_S_aRI2, 1) X(ALIr0, SG_SEG32, UVC_S_aLIr, 1) \
    X(BDPb0, SG_FRAG, 0 * UVC_NFRAG + UVC_FRAG_bDP, 1) X(BDPb1, SG_FRAG, 1 * UVC_NFRAG + UVC_FRAG_bDP, 1) X(BTAb0, SG_FRAG, 0 * UVC_NFRAG + UVC_FRAG_bTA, 1) X(BTAb1, SG_FRAG, 1 * UVC_NFRAG + UVC_FRAG_bTA, 1) \
    X(BTBb0, SG_FRAG, 0 * UVC_NFRAG + UVC_FRAG_bTB, 1) X(BTBb1, SG_FRAG, 1 * UVC_NFRAG + UVC_FRAG_bTB, 1) \
    X(CDP1b0, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP1, 1) X(CDP1b1, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP1, 1) X(CDP12b0, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP12, 1) X(CDP12b1, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP12, 1) \
    X(CDP2b0, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP2, 1) X(CDP2b1, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP2, 1) X(CDP3b0, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP3, 1) X(CDP3b1, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP3, 1) \
    X(C2LP20, SG_FI32, UVC_FI_c2LP2, 1) X(C2LPL0, SG_FI32, UVC_FI_c2LPL, 0) X(C2RP20, SG_FI32, UVC_FI_c2RP2, 1) X(C2RPL0, SG_FI32, UVC_FI_c2RPL, 0) \
    X(C2LB20, SG_FI32, UVC_FI_c2LB2, 1) X(C2LBL0, SG_FI64, UVC_FI64_c2LBL, 0) X(C2RB20, SG_FI32, UVC_FI_c2RB2, 1) X(C2RBL0, SG_FI64, UVC_FI64_c2RBL, 0) \
    X(C2BQ20, SG_FI32, UVC_FI_c2BQ2, 1) X(C2LP00, SG_FI32, UVC_FI_c2LP0, 1) X(C2RP00, SG_FI32, UVC_FI_c2RP0, 1) X(DDP10, SG_DUP, UVC_DUPLEX_dDP1, 1)
// one allele's own cells (BcfFormat_symbol_init, main.hpp:4094-4251): X(name, plane group, plane); the 64-bit planes last.  A cell of a
// 32-bit plane is stored and read as int32_t (AL_), but for the names of AL_WIDE_LIST below; one of a 64-bit plane as long long (AL64_).
#define AL_LIST(X) \
    X(a1BQf, SG_VQ, UVC_VQ_a1BQf) X(a1BQr, SG_VQ, UVC_VQ_a1BQr) X(v2BQf, SG_VQ, UVC_VQ_a2BQf) X(v2BQr, SG_VQ, UVC_VQ_a2BQr) X(vbMQ, SG_VQ, UVC_VQ_bMQ) \
    X(bIAQb, SG_VQ, UVC_VQ_bIAQb) X(bIADb, SG_VQ, UVC_VQ_bIADb) X(cIAQf, SG_VQ, UVC_VQ_cIAQf) X(cIADf, SG_VQ, UVC_VQ_cIADf) X(cIDQf, SG_VQ, UVC_VQ_cIDQf) \
    X(cIAQr, SG_VQ, UVC_VQ_cIAQr) X(cIADr, SG_VQ, UVC_VQ_cIADr) X(cIDQr, SG_VQ, UVC_VQ_cIDQr) \
    X(aMQs, SG_SEG32, UVC_S_aMQs) X(aP1, SG_SEG32, UVC_S_aP1) X(aP2, SG_SEG32, UVC_S_aP2) X(aDPff, SG_SEG32, UVC_S_aDPff) X(aDPfr, SG_SEG32, UVC_S_aDPfr) X(aDPrf, SG_SEG32, UVC_S_aDPrf) X(aDPrr, SG_SEG32, UVC_S_aDPrr) \
    X(aLP1, SG_SEG32, UVC_S_aLP1) X(aLP2, SG_SEG32, UVC_S_aLP2) X(aLPL, SG_SEG32, UVC_S_aLPL) X(aRP1, SG_SEG32, UVC_S_aRP1) X(aRP2, SG_SEG32, UVC_S_aRP2) X(aRPL, SG_SEG32, UVC_S_aRPL) \
    X(aLB1, SG_SEG32, UVC_S_aLB1) X(aLB2, SG_SEG32, UVC_S_aLB2) X(aRB1, SG_SEG32, UVC_S_aRB1) X(aRB2, SG_SEG32, UVC_S_aRB2) X(a2XM2, SG_SEG32, UVC_S_a2XM2) X(a2BM2, SG_SEG32, UVC_S_a2BM2) X(aBQ2, SG_SEG32, UVC_S_aBQ2) \
    X(aPF1, SG_SEG32, UVC_S_aPF1) X(aPF2, SG_SEG32, UVC_S_aPF2) X(aLI1, SG_SEG32, UVC_S_aLI1) X(aLI2, SG_SEG32, UVC_S_aLI2) X(aLIr, SG_SEG32, UVC_S_aLIr) X(aRI1, SG_SEG32, UVC_S_aRI1) X(aRI2, SG_SEG32, UVC_S_aRI2) X(aRIf, SG_SEG32, UVC_S_aRIf) \
    X(aP3, SG_SEG32, UVC_S_aP3) X(aNC, SG_SEG32, UVC_S_aNC) \
    X(bDPf, SG_FRAG, 0 * UVC_NFRAG + UVC_FRAG_bDP) X(bTAf, SG_FRAG, 0 * UVC_NFRAG + UVC_FRAG_bTA) X(bTBf, SG_FRAG, 0 * UVC_NFRAG + UVC_FRAG_bTB) \
    X(bDPr, SG_FRAG, 1 * UVC_NFRAG + UVC_FRAG_bDP) X(bTAr, SG_FRAG, 1 * UVC_NFRAG + UVC_FRAG_bTA) X(bTBr, SG_FRAG, 1 * UVC_NFRAG + UVC_FRAG_bTB) \
    X(cDP1f, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP1) X(cDP12f, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP12) X(cDP2f, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP2) X(cDP3f, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDP3) \
    X(cDPMf, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDPM) X(cDPmf, SG_FAM, 0 * UVC_NFAM + UVC_FAM_cDPm) \
    X(cDP1r, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP1) X(cDP12r, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP12) X(cDP2r, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP2) X(cDP3r, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDP3) \
    X(cDPMr, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDPM) X(cDPmr, SG_FAM, 1 * UVC_NFAM + UVC_FAM_cDPm) \
    X(c2LP1, SG_FI32, UVC_FI_c2LP1) X(c2LP2, SG_FI32, UVC_FI_c2LP2) X(c2LPL, SG_FI32, UVC_FI_c2LPL) X(c2RP1, SG_FI32, UVC_FI_c2RP1) X(c2RP2, SG_FI32, UVC_FI_c2RP2) X(c2RPL, SG_FI32, UVC_FI_c2RPL) \
    X(c2LB1, SG_FI32, UVC_FI_c2LB1) X(c2LB2, SG_FI32, UVC_FI_c2LB2) X(c2RB1, SG_FI32, UVC_FI_c2RB1) X(c2RB2, SG_FI32, UVC_FI_c2RB2) X(c2BQ2, SG_FI32, UVC_FI_c2BQ2) X(c2LP0, SG_FI32, UVC_FI_c2LP0) X(c2RP0, SG_FI32, UVC_FI_c2RP0) \
    X(dDP1, SG_DUP, UVC_DUPLEX_dDP1) X(dDP2, SG_DUP, UVC_DUPLEX_dDP2) \
    X(aLBL, SG_SEG64, UVC_S64_aLBL) X(aRBL, SG_SEG64, UVC_S64_aRBL) X(aLIT, SG_SEG64, UVC_S64_aLIT) X(aRIT, SG_SEG64, UVC_S64_aRIT) X(c2LBL, SG_FI64, UVC_FI64_c2LBL) X(c2RBL, SG_FI64, UVC_FI64_c2RBL)
#define X(n, g, p, t) TOT_##n,
enum { TOT_LIST(X) NTOT };
#undef X
#define X(n, g, p) AL_##n,
enum { AL_LIST(X) NAL };
#undef X
// The C type a cell is read as where it is not the stored one: the reference keeps the fragment, family and duplex depths of a symbol type
// in int, and widens the four path lengths to 64 bits before it multiplies them; its int / 64-bit arithmetic order depends on both.
#define TOT_INT_LIST(X) X(BDPb0) X(BDPb1) X(BTAb0) X(BTAb1) X(BTBb0) X(BTBb1) X(CDP1b0) X(CDP1b1) X(CDP12b0) X(CDP12b1) X(CDP2b0) X(CDP2b1) X(CDP3b0) X(CDP3b1) X(DDP10)
#define AL_WIDE_LIST(X) X(aLPL) X(aRPL) X(c2LPL) X(c2RPL)
template <int tot> struct TotRead { typedef long long type; };
template <int al> struct AlRead { typedef int32_t type; };
#define X(n) template <> struct TotRead<TOT_##n> { typedef int type; };
TOT_INT_LIST(X)
#undef X
#define X(n) template <> struct AlRead<AL_##n> { typedef long long type; };
AL_WIDE_LIST(X)
#undef X
// the 64-bit allele cells: counted from the list, and they are its tail (the gather and AL64_ index them as AL_x - NAL32)
constexpr bool al_is64(int grp) { return grp == SG_SEG64 || grp == SG_FI64; }
constexpr int al64_count(bool tail_only) {
#define X(n, g, p) (g),
    const int grp[] = { AL_LIST(X) };
#undef X
    int n = 0;
    for (int i = NAL - 1; i >= 0 && (al_is64(grp[i]) || !tail_only); i--) n += al_is64(grp[i]) ? 1 : 0;
    return n;
}
constexpr int NAL64 = al64_count(false), NAL32 = NAL - NAL64;
static_assert(NAL64 == 6 && NAL64 == al64_count(true), "NAL64 is the count of 64-bit entries at the end of AL_LIST");

// per active group
enum { GR_x = 0, GR_zpos, GR_st, GR_refsym, GR_mask, GR_hp, GR_r1t, GR_r1u, GR_r1a, GR_r2t, GR_r2u, GR_r2a, GR_insc, GR_delc, GR_ins1c, GR_del1c, GR_rusize, GR_repnum, GR_rec0, GR_nrec, GR_refbdp, GR_vAC, GR_gemit, GR_kept, NGR };
// per record
enum { RH_gi = 0, RH_symbol, RH_src, RH_idx, RH_bdepth, RH_cdepth, NRH };
// what k_dpv_pre hands to k_dp4 / k_dpv_post
enum { MID_cbP = 0, MID_cbBQ, MID_dirdiv, MID_aDPFA, MID_cFA2L, MID_cFA2R, MID_dff, MID_pcread, MID_aPprior, MID_aBprior, MID_aIprior, MID_aSBprior, MID_oriall, NMID };
#define NDP4 14
enum { CNT_nvalid = 0, CNT_ticket1, CNT_ticket2, CNT_kept, NCNT = 8 };

#define GS_BLOCK 256
#define GS_ITEMS 8
#define GS_TILE (GS_BLOCK * GS_ITEMS)
// groups per thread of the gate (measured on the 1 Mb tile: 8 -> 58 us, 4 -> 69 us, 2 -> 84 us: more tiles cost more in tickets and look-back
// than the shorter chains of dependent loads per thread give back)
#ifndef GATE_ITEMS
#define GATE_ITEMS 8
#endif
#define GATE_TILE (GS_BLOCK * GATE_ITEMS)

// ---- the staged rows: X(name = the pointer in Stage, element type, rows, length: 0 = record capacity c, 1 = group capacity gc), in memory order ----
#define SCORE_ROW_LIST(X) \
    X(grp, int32_t, NGR, 1) X(tot, long long, NTOT, 1) X(rh, int32_t, NRH, 0) X(al, int32_t, NAL32, 0) X(al64, long long, NAL64, 0) \
    X(mid, double, NMID, 0) X(d4, double, NDP4 * 2, 0) X(keptoff, int32_t, 1, 1)
#define X(n, T, rows, by_group) SROW_##n,
enum { SCORE_ROW_LIST(X) NSROW };
#undef X
struct ScoreRowDesc { int rows, elem; bool by_group; };
#define X(n, T, rows, by_group) { (rows), (int)sizeof(T), (by_group) != 0 },
constexpr ScoreRowDesc SCORE_ROWS[NSROW] = { SCORE_ROW_LIST(X) };
#undef X
static_assert(SCORE_ROWS[SROW_grp].rows == NGR && SCORE_ROWS[SROW_tot].rows == NTOT && SCORE_ROWS[SROW_rh].rows == NRH && SCORE_ROWS[SROW_al].rows + SCORE_ROWS[SROW_al64].rows == NAL
              && SCORE_ROWS[SROW_mid].rows == NMID && SCORE_ROWS[SROW_d4].rows == NDP4 * 2 && SCORE_ROWS[SROW_keptoff].rows == 1, "the table's row counts are the enums' counts");
static_assert(SCORE_ROWS[SROW_grp].by_group && SCORE_ROWS[SROW_tot].by_group && SCORE_ROWS[SROW_keptoff].by_group && !SCORE_ROWS[SROW_rh].by_group, "grp, tot and keptoff are the rows per group");

inline size_t score_align16(size_t v) { return (v + 15) & ~(size_t)15; }
// The row block at byte `at` (16-aligned) for c records and gc groups: 16-aligned offsets in list order.  A window cannot have more active
// groups than records, nor than its request has groups: the rows per group are min(gc, c) long (and no row is empty).
struct ScoreRows { size_t off[NSROW], end; long long c, gc; };
inline long long score_group_cap(int64_t c, int64_t gc) { return gc > 0 ? (gc < c ? gc : (c > 0 ? c : 1)) : 1; }
inline ScoreRows score_rows_layout(size_t at, int64_t c_, int64_t gc_) {
    ScoreRows L;
    L.c = (c_ > 0 ? c_ : 1); L.gc = score_group_cap(c_, gc_);
    size_t o = at;
    for (int i = 0; i < NSROW; i++) { L.off[i] = o; o = score_align16(o + (size_t)SCORE_ROWS[i].rows * (size_t)(SCORE_ROWS[i].by_group ? L.gc : L.c) * (size_t)SCORE_ROWS[i].elem); }
    L.end = o;
    return L;
}
// bytes of the rows per record where the rows per group are as long as the others
constexpr size_t score_rows_bytes_per_record() { size_t b = 0; for (int i = 0; i < NSROW; i++) b += (size_t)SCORE_ROWS[i].rows * (size_t)SCORE_ROWS[i].elem; return b; }
// tile states of a chained scan over n items of `tile` each (one spare)
inline size_t score_scan_tiles(size_t n, size_t tile) { return (n + tile - 1) / tile + 1; }
inline size_t force_mask_words(int64_t npos_scored) { return (size_t)((npos_scored > 0 ? npos_scored : 0) + 31) / 32; }

// Scratch of one score call.  The head [record counts (2 x int64)] [counters] [tile states of the two scans] is zeroed in front of every
// call; then offsets and the active list (per group of the request), the row block, the force mask and the position table.
struct ScratchLayout { size_t zero_bytes, cnt, status1, status2, offsets, active; ScoreRows rows; size_t force_mask, zpos_tab, total; };
inline ScratchLayout scratch_layout(int64_t npos_scored, int64_t cap) {
    const size_t ngroups = (size_t)(2 * npos_scored), c = (size_t)(cap > 0 ? cap : 1);
    ScratchLayout L; size_t o = 16;
    L.cnt = o; o += NCNT * 4;
    L.status1 = o; o += score_scan_tiles(ngroups, GATE_TILE) * 8;
    L.status2 = o; o += score_scan_tiles(ngroups < c ? ngroups : c, GS_TILE) * 8;
    o = score_align16(o); L.zero_bytes = o;
    L.offsets = o; o = score_align16(o + (ngroups + 1) * 8);
    L.active = o; o = score_align16(o + ngroups * 4);
    L.rows = score_rows_layout(o, cap, (int64_t)ngroups); o = L.rows.end;
    L.force_mask = o; o = score_align16(o + force_mask_words(npos_scored) * 4);   // zeroed and filled only by a call with force-output sites
    L.zpos_tab = o; o = score_align16(o + (size_t)(npos_scored > 0 ? npos_scored : 0) * 4);   // written only by a ranges call (k_range_map)
    L.total = o;
    return L;
}
// Row set of one chunk of a streamed score (two per stream): [record counts 2 x int64][counters][tile states of the keep scan] -- zeroed in
// front of every chunk -- then the row block, the records and (kept_only) their compacted copy.  c = chunk_records, gc = groups of the request.
struct SetLayout { size_t zero_bytes, cnt, status2; ScoreRows rows; size_t fields, kept, total; };
inline SetLayout set_layout(int64_t c_, int64_t gc_, int with_kept) {
    SetLayout L; size_t o = 16;
    L.cnt = o; o += NCNT * 4;
    L.status2 = o; o += score_scan_tiles((size_t)score_group_cap(c_, gc_), GS_TILE) * 8;
    o = score_align16(o); L.zero_bytes = o;
    L.rows = score_rows_layout(o, c_, gc_); o = L.rows.end;
    const size_t rec_bytes = (size_t)UVC_NUM_SCORE_FIELDS * (size_t)L.rows.c * 4;
    L.fields = o; o = score_align16(o + rec_bytes);
    L.kept = o; if (with_kept) o = score_align16(o + rec_bytes);
    L.total = o;
    return L;
}
// device bytes of one row set per unit of chunk_records, at most: the rows per group as long as the others, the records and their kept
// copy, + 1 for the tile states
constexpr size_t score_set_bytes_per_record() { return score_rows_bytes_per_record() + 2 * (size_t)UVC_NUM_SCORE_FIELDS * 4 + 1; }
#endif
