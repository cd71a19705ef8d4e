/* uvcgpu.h -- C ABI of the MI355X-native UVC hot path (libuvcgpu.so).
 *
 * The reference (genetronhealth/uvc v0.15.1) has no FFI/plugin layer; the seam this library
 * replaces is the pair of C++ call groups inside `process_batch` (main.cpp:458-1193):
 *
 *   accumulate:  Symbol2CountCoverageSet S(tid, beg, end+1)                 main.cpp:569
 *                S.updateByRegion3Aln(fq3, hap_bq, hap_fq, hap_f2q, alns3,
 *                    refstring, region_repeatvec, baq, baq2, prev, cur, params)
 *                                                   main.cpp:575-591 -> main.hpp:3665-3742
 *   score:       BcfFormat_symboltype_init   main.cpp:648 -> main.hpp:3889
 *                BcfFormat_symbol_init       main.cpp:911 -> main.hpp:4094
 *                BcfFormat_symbol_calc_DPv   main.cpp:931 -> main.hpp:4274
 *                BcfFormat_symbol_sum_DPv    main.cpp:957 -> main.hpp:4888
 *                BcfFormat_symbol_calc_qual  main.cpp:967 -> main.hpp:4908
 *
 * Everything crosses the boundary as plain pointers + sizes (no C++/torch types).  All entry
 * points return 0 on success and a negative UVCGPU_E* code on failure; uvcgpu_last_error()
 * gives the text.  Library code never aborts (the reference abort()s / exit()s instead,
 * e.g. grouping.cpp:59-87).  A handle is confined to one host thread at a time, which is how
 * the reference calls process_batch from its OpenMP loop (main.cpp:1478-1520).
 *
 * Coordinates are 0-based reference positions, as in the reference (uvc1_refgpos_t).
 */
#ifndef UVCGPU_H_INCLUDED
#define UVCGPU_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- alphabet (a1) ------------ */
/* AlignmentSymbol, main_conversion.hpp:316-334.  Numeric values are part of the ABI. */
enum {
    UVC_BASE_A = 0, UVC_BASE_C = 1, UVC_BASE_G = 2, UVC_BASE_T = 3, UVC_BASE_N = 4, UVC_BASE_NN = 5,
    UVC_LINK_M = 6, UVC_LINK_D3P = 7, UVC_LINK_D2 = 8, UVC_LINK_D1 = 9,
    UVC_LINK_I3P = 10, UVC_LINK_I2 = 11, UVC_LINK_I1 = 12, UVC_LINK_NN = 13,
    UVC_NUM_SYMBOLS = 14
};
enum { UVC_BASE_SYMBOL = 0, UVC_LINK_SYMBOL = 1 };       /* SymbolType, main_conversion.hpp:375-379 */
enum { UVC_PLATFORM_AUTO = 0, UVC_PLATFORM_ILLUMINA = 1, UVC_PLATFORM_IONTORRENT = 2, UVC_PLATFORM_OTHER = 3 };

/* ---------------------------------------------------------------- errors ------------------- */
enum {
    UVCGPU_OK = 0,
    UVCGPU_ENOREADS = -1,      /* region has no reads: process_batch returns -1 (main.cpp:520-523) */
    UVCGPU_EINVAL = -2,        /* malformed argument (bad offsets, read outside region, ...) */
    UVCGPU_EUNSUPPORTED = -3,  /* CIGAR op the reference itself throws on (process_cigar, main_conversion.hpp:902-916) or a shape beyond the documented limits
                                  (2^29 positions, 2^31 read bases, 2^27 InDel ops per region; bias_thres_interfering_indel above 10000) */
    UVCGPU_EDEVICE = -4,       /* HIP runtime failure / no gfx950 device */
    UVCGPU_ESTATE = -5,        /* call order violated (e.g. score before accumulate) */
    UVCGPU_ENOMEM = -6,
    UVCGPU_STREAM_END = 1      /* uvcgpu_score_stream_next: every chunk has been returned (not an error) */
};

/* ---------------------------------------------------------------- parameters (C15) --------- */
/* POD mirror of the hot-path fields of `struct CommandLineArgs` (CmdLineArgs.hpp:20-438).
 * `struct_size` versions the struct (set by uvcgpu_params_default). */
typedef struct UvcParams {
    int32_t struct_size;
    int32_t reserved_;
#define UVC_PI(name, dflt) int32_t name;
#define UVC_PD(name, dflt)
#include "uvc_params.def"
#undef UVC_PI
#undef UVC_PD
    int32_t pad_to_8_;
#define UVC_PI(name, dflt)
#define UVC_PD(name, dflt) double name;
#include "uvc_params.def"
#undef UVC_PI
#undef UVC_PD
} UvcParams;

/* Fills *p with the reference defaults (CmdLineArgs.hpp:43-417). */
void uvcgpu_params_default(UvcParams *p);
/* Applies the platform deltas of CommandLineArgs::selfUpdateByPlatform (CmdLineArgs.cpp:113-134)
 * and sets inferred_sequencing_platform / central_readlen / inferred_maxMQ, which the reference
 * infers from the first 5000 BAM records (CmdLineArgs.cpp:50-92). */
void uvcgpu_params_apply_platform(UvcParams *p, int32_t platform, int32_t central_readlen, int32_t max_mapq);
/* The whole platform step of the reference for a requested --sequencing-platform (CmdLineArgs.cpp:37-134), on top of whatever values the
 * caller has set already (the deltas are added to them):
 *   UVC_PLATFORM_AUTO        = uvcgpu_params_apply_platform(p, inferred, central_readlen, max_mapq)
 *   UVC_PLATFORM_OTHER       records `inferred`, central_readlen (where 0) and max_mapq like AUTO, and applies no deltas
 *   UVC_PLATFORM_ILLUMINA / UVC_PLATFORM_IONTORRENT  taken as given: that platform's deltas; `inferred`, `central_readlen` and
 *                            `max_mapq` are not read (the reference does not look at the file then)
 * `inferred` (ILLUMINA or IONTORRENT), `central_readlen` and `max_mapq` are what the caller found in the first alignments.
 * UVCGPU_EINVAL for a requested platform outside 0..3. */
int uvcgpu_params_apply_platform_ex(UvcParams *p, int32_t sequencing_platform, int32_t inferred, int32_t central_readlen, int32_t max_mapq);
/* The value refusals of uvcgpu_region_create (which calls this): struct_size, repeat sizes, indel_BQ_max and bias_thres_interfering_indel
 * (UVCGPU_EINVAL / UVCGPU_EUNSUPPORTED with the same messages).  0 = a region handle accepts *p. */
int uvcgpu_params_check(const UvcParams *p);

/* ---------------------------------------------------------------- parameter names ---------- */
/* One table of every row of include/uvc_params.def (UvcParams, in .def order) followed by every row of include/uvc_group_params.def
 * (UvcGroupParams), generated from the two X-macro files.  A row's name is its field name; uvcgpu_param_set also takes the option form
 * of the reference's command line (REPLACE_UNDERSCORE_WITH_HYPHEN, CmdLineArgs.cpp:20: every '_' a '-', case kept). */
enum { UVC_PARAM_INT = 0, UVC_PARAM_DOUBLE = 1 };                 /* kind */
enum { UVC_PARAM_OF_PARAMS = 0, UVC_PARAM_OF_GROUP = 1 };         /* owning struct */
struct UvcGroupParams;
int32_t uvcgpu_param_count(void);
/* Row i (0 <= i < uvcgpu_param_count()): name, kind, owning struct, default (uvcgpu_params_default / uvcgpu_group_params_default) and
 * whether uvcgpu_param_set may set it (0 for the derived rows: inferred_*, tumor_vcf_*).  NULL outputs are skipped.  UVCGPU_EINVAL for i
 * out of range. */
int uvcgpu_param_info(int32_t i, const char **name, int32_t *kind, int32_t *owner, double *dflt, int32_t *settable);
/* The value of row i in *p (owner UVC_PARAM_OF_PARAMS) or *g (UVC_PARAM_OF_GROUP), as a double (exact for every int32). */
int uvcgpu_param_get(const UvcParams *p, const struct UvcGroupParams *g, int32_t i, double *value);
/* Sets the row called `name` (field or option form) from the text `value`, parsed strictly: the whole string; an int row takes a decimal
 * int32 or true / false (1 / 0), a double row a finite number.  `p` or `g` may be NULL when the row is not theirs.  UVCGPU_EINVAL for an
 * unknown or derived name or a bad value, nothing changed; uvcgpu_last_error() names the row. */
int uvcgpu_param_set(UvcParams *p, struct UvcGroupParams *g, const char *name, const char *value);

/* ---------------------------------------------------------------- reads (alns3) ------------ */
/* SoA image of `alns3` = vector<pair<array<vector<vector<bam1_t*>>,2>, MolecularBarcode>>
 * (main.hpp:3672): family -> strand(2) -> fragment (qname) -> alignment (R1, R2).
 * Reads must be grouped: all reads of one (fam_id, fam_strand, frag_id) contiguous, fragments
 * of one (fam_id, fam_strand) contiguous, both strands of one family contiguous.
 * Per read (htslib bam1_core_t fields, BAM spec):                                              */
typedef struct UvcReadSoA {
    int32_t struct_size;        /* sizeof(UvcReadSoA) of the header the caller was built with: the library refuses any other (fields were
                                   added to the end of this struct before, and will be again)                                         */
    int32_t reserved_;
    int64_t n_reads;
    const int32_t  *pos;        /* core.pos  (0-based leftmost)                                  */
    const int32_t  *mpos;       /* core.mpos                                                    */
    const int32_t  *isize;      /* core.isize, already NORM_INSERT_SIZE'd (common.hpp:73)       */
    const uint16_t *flag;       /* core.flag                                                    */
    const uint8_t  *mapq;       /* core.qual                                                    */
    const int32_t  *nm;         /* NM aux tag, -1 when absent (main.hpp:980-981)                */
    const int32_t  *l_qseq;     /* core.l_qseq                                                  */
    const int64_t  *seq_off;    /* offset of the read's first base in bases[] / quals[]; NULL = the reads lie back to back in read
                                   order (seq_off[i] = sum of l_qseq[0..i)): the library derives the offsets on the device            */
    const int64_t  *cigar_off;  /* offset of the read's first op in cigars[]; NULL = back to back in read order                     */
    const int32_t  *n_cigar;    /* core.n_cigar                                                 */
    const int32_t  *frag_id;    /* fragment (qname group) id, unique within (fam_id, strand)    */
    const int32_t  *fam_id;     /* family index, 0..n_fams-1                                    */
    const uint8_t  *fam_strand; /* 0/1 = bam_get_strand(aln) slot of alns3 (grouping.cpp:926)   */
    int64_t n_bases;
    const uint8_t  *bases;      /* 1 B/base = seq_nt16_int[bam_seqi()]: 0..3 = ACGT, 4 = other  */
    const uint8_t  *quals;      /* 1 B/base phred (bam_get_qual), after apply_bq_err_correction3 unless uvcgpu_region_correct_bq() is used */
    int64_t n_cigar_ops;
    const uint32_t *cigars;     /* BAM-packed ops: len<<4 | op                                  */
    int32_t n_fams;
    const uint8_t  *fam_dflag;  /* MolecularBarcode::duplexflag per family (grouping.cpp:931):
                                   0x1 UMI found, 0x2 duplex found, 0x4 amplicon, 0x8 borders preserved */
    /* Alternative to `bases` (then bases == NULL): the bases as the BAM record holds them (bam_get_seq: 4-bit codes "=ACMGRSVTWYHKDBN",
     * two per byte, high nibble first, every read starting on a byte boundary), the reads back to back in read order -- read i's bytes
     * start at sum of (l_qseq[j] + 1) / 2 over j < i.  The library applies seq_nt16_int[] on the device.  A quarter less to copy than
     * one byte per base + qual. */
    const uint8_t  *bases4;
    int64_t n_bases4_bytes;
} UvcReadSoA;

/* ---------------------------------------------------------------- per-position state (a2) -- */
/* Plane groups readable with uvcgpu_region_fetch().  Every group is a dense array
 * [n_planes][n_positions] (position fastest), position index = refpos - region begin.
 * "per symbol" groups are [field][symbol][pos].  The comments below are documentation: the table that the library and the Python mirror
 * read (element size, fields, strands, per symbol, zero fill) is uvc_field_groups.def. */
enum UvcField {
    UVC_F_PREP32 = 0,   /* int32 [UVC_NPREP32][npos]          SegFormatPrepSet i32 fields, main_conversion.hpp:541-605 */
    UVC_F_PREP64 = 1,   /* int64 [UVC_NPREP64][npos]          SegFormatPrepSet i64 fields                             */
    UVC_F_THRES  = 2,   /* int32 [UVC_NTHRES][npos]           SegFormatThresSet, main_conversion.hpp:614-643          */
    UVC_F_SEG32  = 3,   /* int32 [UVC_NSEG32][14][npos]       SegFormatInfoSet i32 fields, main_conversion.hpp:645-691 */
    UVC_F_SEG64  = 4,   /* int64 [UVC_NSEG64][14][npos]       SegFormatInfoSet i64 fields                             */
    UVC_F_VQ     = 5,   /* int32 [UVC_NVQ][14][npos]          VQFormatTagSet stored slots, main_conversion.hpp:743-763 */
    UVC_F_BQSUM  = 6,   /* int32 [14][npos]                   bg_seg_bqsum_conslogo, main.hpp:2566                    */
    UVC_F_FRAG   = 7,   /* int32 [2][UVC_NFRAG][14][npos]     FragFormatDepthSet x strand, main_conversion.hpp:693-699 */
    UVC_F_FAM    = 8,   /* int32 [2][UVC_NFAM][14][npos]      FamFormatDepthSet x strand, main_conversion.hpp:722-734 */
    UVC_F_FAMINFO32 = 9,/* int32 [UVC_NFAMINFO32][14][npos]   FamFormatInfoSet i32 fields, main_conversion.hpp:701-720 */
    UVC_F_FAMINFO64 = 10,/* int64 [UVC_NFAMINFO64][14][npos]  FamFormatInfoSet i64 fields                             */
    UVC_F_DUPLEX = 11,  /* int32 [UVC_NDUPLEX][14][npos]      DuplexFormatDepthSet, main_conversion.hpp:736-741       */
    UVC_F_RTR    = 12,  /* int32 [UVC_NRTR][npos]             RegionalTandemRepeat AFTER P1b edits indelphred, common.hpp:150-160 */
    UVC_F_BAQ    = 13,  /* int64 [2][npos]                    baq_offsetarr, baq_offsetarr2, main.cpp:400-429         */
    UVC_NUM_FIELD_GROUPS = 14
};

/* plane indices inside the groups (order = declaration order in the reference structs) */
enum { /* UVC_F_PREP32 */
    UVC_P_a_dp = 0, UVC_P_a_near_ins_dp, UVC_P_a_near_del_dp, UVC_P_a_near_RTR_ins_dp, UVC_P_a_near_RTR_del_dp,
    UVC_P_a_pcr_dp, UVC_P_a_umi_dp, UVC_P_a_snv_dp, UVC_P_a_dnv_dp, UVC_P_a_highBQ_dp,
    UVC_P_a_near_pcr_clip_dp, UVC_P_a_near_long_clip_dp, UVC_P_a_at_ins_dp, UVC_P_a_at_del_dp,
    UVC_P_a_XM1500, UVC_P_a_GO1500, UVC_P_a_GAPLEN, UVC_P_a_qlen,
    UVC_P_a_near_ins_inv100len, UVC_P_a_near_del_inv100len,
    UVC_P_a_LIDP, UVC_P_a_RIDP,
    UVC_P_a_l_dist_sum, UVC_P_a_r_dist_sum, UVC_P_a_inslen_sum, UVC_P_a_dellen_sum,
    UVC_NPREP32
};
enum { /* UVC_F_PREP64 */
    UVC_P_a_near_ins_pow2len = 0, UVC_P_a_near_del_pow2len,
    UVC_P_a_near_ins_l_pow2len, UVC_P_a_near_ins_r_pow2len, UVC_P_a_near_del_l_pow2len, UVC_P_a_near_del_r_pow2len,
    UVC_P_a_LI, UVC_P_a_RI,
    UVC_P_a_l_BAQ_sum, UVC_P_a_r_BAQ_sum, UVC_P_a_insBAQ_sum, UVC_P_a_delBAQ_sum,
    UVC_NPREP64
};
enum { /* UVC_F_THRES */
    UVC_T_aLPxT = 0, UVC_T_aRPxT,
    UVC_T_aLI1T, UVC_T_aLI2T, UVC_T_aRI1T, UVC_T_aRI2T, UVC_T_aLI1t, UVC_T_aLI2t, UVC_T_aRI1t, UVC_T_aRI2t,
    UVC_T_aLP1t, UVC_T_aLP2t, UVC_T_aRP1t, UVC_T_aRP2t,
    UVC_T_aLB1t, UVC_T_aLB2t, UVC_T_aRB1t, UVC_T_aRB2t,
    UVC_NTHRES
};
enum { /* UVC_F_SEG32 */
    UVC_S_a2XM2 = 0, UVC_S_a2BM2, UVC_S_aPF1, UVC_S_aPF2, UVC_S_aBQ2, UVC_S_aMQs,
    UVC_S_aP1, UVC_S_aP2, UVC_S_aP3, UVC_S_aNC,
    UVC_S_aDPff, UVC_S_aDPfr, UVC_S_aDPrf, UVC_S_aDPrr,
    UVC_S_aLP1, UVC_S_aLP2, UVC_S_aLPL, UVC_S_aRP1, UVC_S_aRP2, UVC_S_aRPL,
    UVC_S_aLB1, UVC_S_aLB2, UVC_S_aRB1, UVC_S_aRB2,
    UVC_S_aLI1, UVC_S_aLI2, UVC_S_aRI1, UVC_S_aRI2, UVC_S_aRIf, UVC_S_aLIr,
    UVC_NSEG32
};
enum { UVC_S64_aLBL = 0, UVC_S64_aRBL, UVC_S64_aLIT, UVC_S64_aRIT, UVC_NSEG64 };   /* UVC_F_SEG64 */
enum { /* UVC_F_VQ: the 14 stored VQFormatTagSet slots */
    UVC_VQ_a1BQf = 0, UVC_VQ_a1BQr, UVC_VQ_a2BQf, UVC_VQ_a2BQr, UVC_VQ_bMQ,
    UVC_VQ_bIAQb, UVC_VQ_bIADb, UVC_VQ_bIDQb,
    UVC_VQ_cIAQf, UVC_VQ_cIADf, UVC_VQ_cIDQf, UVC_VQ_cIAQr, UVC_VQ_cIADr, UVC_VQ_cIDQr,
    UVC_NVQ
};
enum { UVC_FRAG_bDP = 0, UVC_FRAG_bTA, UVC_FRAG_bTB, UVC_NFRAG };                  /* UVC_F_FRAG */
enum { UVC_FAM_cDP1 = 0, UVC_FAM_cDP12, UVC_FAM_cDP2, UVC_FAM_cDP3, UVC_FAM_cDPM, UVC_FAM_cDPm, UVC_FAM_cDP21, UVC_FAM_cDPD, UVC_NFAM };
enum { /* UVC_F_FAMINFO32 */
    UVC_FI_c2LP1 = 0, UVC_FI_c2LP2, UVC_FI_c2LPL, UVC_FI_c2RP1, UVC_FI_c2RP2, UVC_FI_c2RPL, UVC_FI_c2LP0, UVC_FI_c2RP0,
    UVC_FI_c2LB1, UVC_FI_c2LB2, UVC_FI_c2RB1, UVC_FI_c2RB2, UVC_FI_c2BQ2,
    UVC_NFAMINFO32
};
enum { UVC_FI64_c2LBL = 0, UVC_FI64_c2RBL, UVC_NFAMINFO64 };
enum { UVC_DUPLEX_dDP1 = 0, UVC_DUPLEX_dDP2, UVC_NDUPLEX };
enum { UVC_RTR_begpos = 0, UVC_RTR_tracklen, UVC_RTR_unitlen, UVC_RTR_indelphred, UVC_RTR_anyTR_begpos, UVC_RTR_anyTR_tracklen, UVC_RTR_anyTR_unitlen, UVC_NRTR };

/* ---------------------------------------------------------------- scoring (a13-a17) -------- */
/* One scored allele = one (refpos, symbol[, indel string]) the reference would carry as a
 * bcfrec::BcfFormat through symbol_init -> calc_DPv -> sum_DPv -> calc_qual.  Integer FORMAT
 * fields only (bcf_formats_generator1.cpp:135-527); string fields stay host side. */
enum UvcScoreField {
    /* identity + depths (bit-exact class) */
    UVC_O_refpos = 0, UVC_O_symbol, UVC_O_refsymbol,
    UVC_O_DP, UVC_O_AD, UVC_O_bDP, UVC_O_bAD, UVC_O_c2DP, UVC_O_c2AD, UVC_O_bDPa, UVC_O_cDP0a,
    /* fill_symbol_VQ_fmts, main.hpp:3820-3887 */
    UVC_O_a2BQf, UVC_O_a2BQr, UVC_O_aBQ, UVC_O_aBQQ, UVC_O_bMQ,
    /* calc_DPv, main.hpp:4274-4844 */
    UVC_O_nPF0, UVC_O_nPF1, UVC_O_bNMa, UVC_O_bNMb, UVC_O_bNMQ,
    UVC_O_nNFA0, UVC_O_nNFA1, UVC_O_nNFA2, UVC_O_nNFA3, UVC_O_nNFA4, UVC_O_nNFA5,
    UVC_O_nAFA0, UVC_O_nAFA1, UVC_O_nAFA2, UVC_O_nAFA3, UVC_O_nAFA4, UVC_O_nAFA5, UVC_O_nAFA6, UVC_O_nAFA7, UVC_O_nAFA8,
    UVC_O_nBCFA0, UVC_O_nBCFA1, UVC_O_nBCFA2, UVC_O_nBCFA3, UVC_O_nBCFA4, UVC_O_nBCFA5, UVC_O_nBCFA6, UVC_O_nBCFA7, UVC_O_nBCFA8, UVC_O_nBCFA9,
    UVC_O_FTS,          /* bit i set <=> i-th fmt_bias_push (main.hpp:4745-4769) fired; 0 <=> "PASS" */
    UVC_O_tier2,        /* enable_tier2_consensus_format_tags */
    UVC_O_cDP1v, UVC_O_cDP1w, UVC_O_cDP1x, UVC_O_cDP2v, UVC_O_cDP2w, UVC_O_cDP2x,
    /* sum_DPv, main.hpp:4888-4906: [0] = sum over alleles, [1] = the NN allele */
    UVC_O_CDP1v0, UVC_O_CDP1v1, UVC_O_CDP1w0, UVC_O_CDP1w1, UVC_O_CDP1x0, UVC_O_CDP1x1,
    UVC_O_CDP2v0, UVC_O_CDP2v1, UVC_O_CDP2w0, UVC_O_CDP2w1, UVC_O_CDP2x0, UVC_O_CDP2x1,
    /* calc_qual, main.hpp:4908-5343 */
    UVC_O_cMmQ, UVC_O_aAaMQ, UVC_O_bMQQ, UVC_O_bIAQ, UVC_O_cIAQ,
    UVC_O_cPCQ1, UVC_O_cPLQ1, UVC_O_cPCQ2, UVC_O_cPLQ2, UVC_O_bTINQ, UVC_O_cTINQ,
    UVC_O_gVQ1, UVC_O_cVQ1, UVC_O_dVQinc, UVC_O_cVQ2, UVC_O_CONTQ,
    /* InDel alleles: gapSa = index (into uvcgpu_region_indel_alleles' rows) of the first row that carries this record's InDel string,
     * or -1 (not an InDel, or the string came from the caller); gapSa_len = indelstring.size() (main.cpp:907) */
    UVC_O_gapSa, UVC_O_gapSa_len,
    UVC_O_tkey,                         /* index of the tumor record (UvcScoreRequest::tumor_keys) this allele was paired with, or -1 */
    /* ---- the calling step behind calc_qual (main.cpp:990-1168): same value in every record of a (position, symbol type) group ---- */
    /* the two best non-reference alleles of the group by (max(cVQ1, cVQ2), cVQ1, cVQ2, symbol, InDel string), main.cpp:996-1016:
     * cVQ1M / cVQ2M, cVQAM as the symbol (14 = none), cVQSM as a row of uvcgpu_region_indel_alleles (-1 = no string) */
    UVC_O_cVQ1M0, UVC_O_cVQ1M1, UVC_O_cVQ2M0, UVC_O_cVQ2M1, UVC_O_cVQAM0, UVC_O_cVQAM1, UVC_O_cVQSM0, UVC_O_cVQSM1,
    UVC_O_vAC0, UVC_O_vAC1,             /* alleles at or above germ_phred_het3al per symbol type at this zerobased_pos, main.cpp:994-997, 1088 */
    /* output_germline, main.hpp:5483-5775: vNLODQ[own symbol type] = GL4raw[0] - max(GL4raw[1..3]); GL4raw; GST = a0..a3 LODQ + the four
     * het LODQs; best genotype index (0 "0/0", 1 "0/1", 2 "1/1", 3 "1/2"), its GQ; whether a GERMLINE line is written (needs
     * OUTVAR_GERMLINE); the records chosen as ref / alt1 / alt2, as record indices (-1 = the padding allele) */
    UVC_O_vNLODQ, UVC_O_GL4_0, UVC_O_GL4_1, UVC_O_GL4_2, UVC_O_GL4_3,
    UVC_O_GST0, UVC_O_GST1, UVC_O_GST2, UVC_O_GST3, UVC_O_GST4, UVC_O_GST5, UVC_O_GST6, UVC_O_GST7,
    UVC_O_germ_GT, UVC_O_germ_GQ, UVC_O_germ_emit, UVC_O_germ_ref, UVC_O_germ_alt1, UVC_O_germ_alt2,
    /* ---- per record: main.cpp:1081-1147 and the arithmetic of append_vcf_record (main.hpp:6027-6272) ---- */
    UVC_O_out,                          /* will_generate_out && !is_out_blocked: append_vcf_record is called for this record */
    UVC_O_vHGQ, UVC_O_NLODQ, UVC_O_NLODV /* argmin_nlodq_symbol, 14 = none */, UVC_O_TLODQ, UVC_O_SomaticQ,
    UVC_O_TNBQF0, UVC_O_TNBQF1, UVC_O_TNBQF2, UVC_O_TNBQF3, UVC_O_TNCQF0, UVC_O_TNCQF1, UVC_O_TNCQF2, UVC_O_TNCQF3,
    UVC_O_QUAL,                         /* vcfqual: the bit pattern of the 32-bit float the reference prints with std::to_string */
    UVC_O_FILTER,                       /* 0..5 = Q10..Q60 (bcfrec::FILTER_IDS), 6 = PASS */
    UVC_O_keep,                         /* the record is written: keep_var && tki.bDP >= min_ad, main.hpp:6253-6262 */
    /* FORMAT/FTS prints "<bias name>-<round(100 * biasFA / refFA)>" for every bias that fired (fmt_bias_push, main.hpp:4266-4269): those
     * percentages, 8 bits each (bias i of UVC_O_FTS in byte i % 4 of field i / 4, 0 where the bias did not fire, capped at 255) */
    UVC_O_FTSpct0, UVC_O_FTSpct1, UVC_O_FTSpct2, UVC_O_FTSpct3, UVC_O_FTSpct4,
    UVC_NUM_SCORE_FIELDS
};

/* Caller-supplied InDel alleles (optional override).  By default the library derives the alleles of every scored InDel symbol
 * itself, the way fill_by_indel_info / indel_get_majority do (main.hpp:5350-5455, instcode.hpp, main.cpp:853-896): one record per
 * distinct inserted sequence / deleted length whose fragment support is at least a quarter of the best one, with
 * bDPa / cDP0a = that allele's fragment / family support summed over both strands.  If the request lists alleles for a
 * (refpos, symbol), those are scored instead. */
typedef struct UvcIndelAllele {
    int32_t refpos;
    int32_t symbol;
    int32_t bDPa;       /* std::get<0>(bcad0a_indelstring_tki), main.cpp:923 */
    int32_t cDP0a;      /* std::get<1>(...),                    main.cpp:924 */
    int32_t indel_len;  /* indelstring.size(),                  main.cpp:907 */
} UvcIndelAllele;

enum { UVC_MGVCF_SYMBOL = 15, UVC_ADDITIONAL_INDEL_CANDIDATE_SYMBOL = 16 };   /* main_conversion.hpp: the VTI of the two position-level line types */
/* One tumor-sample record of the T/N channel (TumorKeyInfo, main_conversion.hpp:490-529), reduced to what the scoring functions read:
 * tpfa of calc_DPv = (cDP1x + 1) / (CDP1x + 2) (main.cpp:935), tpfa of calc_qual = (bDP + 0.5) / (BDP + 1) (main.cpp:985-986),
 * enable_tier2_consensus_format_tags (main.hpp:4475), and for InDels the length of the tumor record's inserted / deleted string
 * (main.cpp:867-880).  Only read when UvcParams::tumor_vcf_is_provided. */
typedef struct UvcTumorKey {
    int32_t refpos, symbol;     /* key (the VTI of the tumor record) */
    int32_t cDP1x, CDP1x, bDP, BDP;
    int32_t tier2;
    int32_t indel_len;
    /* the rest of TumorKeyInfo that the somatic quality of the normal-sample record reads (main.cpp:1104-1147, main.hpp:6095-6206) */
    int32_t cVQ1, cPCQ1, cDP2x, CDP2x, cVQ2, cPCQ2, bNMQ, vHGQ, tDP;
    /* INFO values the record of the normal sample repeats from the tumor record (main.cpp:366-372, main.hpp:6214-6218): tADR, tDPC */
    int32_t tAD0, tAD1, t2DP;
} UvcTumorKey;

/* One row of the per-strand InDel allele tables that fill_by_indel_info pushes into gapSeq / gapbAD1 / gapcAD1 / gc2AD / gc2dAD
 * (instcode.hpp:44-83): the allele counters kept beside FRAG_bDP, FAM_cDP12-after-filtering, FAM_cDP2 and FAM_cDPD / DUPLEX_dDP2
 * (main.hpp:2710-2717, 3327-3336, 3196-3206, 3458-3469, 3535-3546).  Rows are ordered by (refpos, symbol, strand) and inside a
 * group as the reference sorts them (descending (cAD1, bAD1, c2AD, c2dAD, sequence)). */
typedef struct UvcGapRow {
    int32_t refpos, symbol, strand;
    int32_t len;                /* inserted / deleted length */
    int64_t seq_off;            /* insertions: offset of `len` base codes (0..4 = ACGTN) in the sequence buffer; deletions: -1 (the deleted
                                 * bases are refseq[refpos - beg, +len)) */
    int32_t bAD1, cAD1, c2AD, c2dAD;
} UvcGapRow;

typedef struct UvcScoreRequest {
    int32_t pos_beg;            /* first zerobased_pos scored (rpos_inclu_beg, main.cpp:527); -1 = whole region core */
    int32_t pos_end;            /* exclusive */
    int32_t all_out;            /* paramset.should_output_all (-A), main.cpp:835 */
    int32_t is_amplicon;        /* ASSAY_TYPE_AMPLICON == inferred_assay_type, main.cpp:510-525 */
    int64_t n_indel_alleles;
    const UvcIndelAllele *indel_alleles;
    int64_t n_tumor_keys;       /* normal sample of a T/N pair: the tumor records of this region, sorted by (refpos, symbol); a position is
                                 * scored iff it has a record (extended_posidx_to_is_rescued, main.cpp:532-538), every symbol of it */
    const UvcTumorKey *tumor_keys;
    int32_t release_state;      /* 1: the caller is done with the planes of this region after this call (no further score / fetch until the next
                                 * accumulate, which return UVCGPU_ESTATE): the library zeroes them for the next accumulate while the records
                                 * travel to the host, instead of in front of the next accumulate's kernels */
    int32_t base_at_pos_beg;    /* 0: as process_batch at the start of a region, the BASE sub-position of pos_beg (refpos pos_beg - 1) is not
                                 * scored (main.cpp:643).  1: it is -- for a region that continues an adjacent one whose last zerobased_pos was
                                 * pos_beg - 1 (fixed tiles of one covered stretch): a run of such tiles then yields each (position, symbol type)
                                 * exactly once, the records of one uncut region.  Needs pos_beg > region begin */
    int32_t region_beg;         /* incluBegPosition of the BED line this region belongs to (main.cpp:655-656): besides every refpos that is a
                                 * multiple of 1000 an MGVCF block also opens at refpos == region_beg.  0 = nothing beyond the multiples */
    int32_t kept_only;          /* 1: return only the (zerobased_pos, symbol type) groups the record writer reads -- those with a written record
                                 * (keep && out) or a GERMLINE line (germ_emit) -- all records of such a group, in the usual order, germ_ref /
                                 * germ_alt1 / germ_alt2 re-based to the returned array.  UvcScoreOut::capacity then only has to hold these (a
                                 * few thousand per Mb at the default gate instead of ~54 k): the D2H shrinks by an order of magnitude.
                                 * uvcgpu_region_vcf_records writes the same text from either form */
    const char *const *tumor_sample_columns;   /* [n_tumor_keys] or NULL: the sample column of each tumor record as text.  Only the record writer reads
                                 * it: with is_tumor_format_retrieved the normal-sample line ends with the tumor's column (bcf1_to_string,
                                 * main.hpp:5897-5910, 6269; MGVCF / ADDITIONAL_INDEL_CANDIDATE lines: main.cpp:739-757, 784-798) */
    const char *const *tumor_ref_alt;          /* [n_tumor_keys] or NULL: "REF\tALT" of each tumor record (TumorKeyInfo::ref_alt, main.cpp:380).  Record writer
                                 * only: the InDel string of a rescued InDel record is the tumor's (main.cpp:867-880); without it such a record
                                 * is written with its symbolic allele */
    int64_t n_force_sites;      /* force-output sites: zerobased_pos values, sorted ascending (repeats allowed); 0 / NULL = none.  A site selects
                                 * both (zerobased_pos, symbol type) groups of its position -- the BASE group of refpos site - 1 and the LINK group
                                 * of refpos site, whose records all print VCF POS = site -- and those are scored and written exactly as with
                                 * all_out = 1; every other group exactly as without it.  The two groups of a position go together because the
                                 * records of one read the other's gate (vAC0 / vAC1, and a GERMLINE line of either lets the REF record out).
                                 * Sites outside [pos_beg, pos_end) select nothing.  Not with tumor_vcf_is_provided (the rescue set is the gate
                                 * of a normal sample).  The planes, the MGVCF block and ADDITIONAL_INDEL_CANDIDATE lines do not depend on it */
    const int32_t *force_sites;
} UvcScoreRequest;

typedef struct UvcScoreOut {
    int64_t capacity;           /* in: records the planes can hold */
    int64_t n_records;          /* out: records produced (may exceed capacity => UVCGPU_ENOMEM, nothing written) */
    int32_t *fields;            /* [UVC_NUM_SCORE_FIELDS][capacity], record index fastest */
} UvcScoreOut;

/* ---------------------------------------------------------------- entry points ------------- */
typedef struct uvcgpu_region uvcgpu_region_t;

/* Once per host thread / process.  Fails with UVCGPU_EDEVICE when there is no gfx950 device:
 * there is no CPU fallback inside this library. */
int uvcgpu_init(int device_id);
/* Number of HIP devices visible to the process (0 when there is none); the region-shard dispatchers spread their workers over them. */
int uvcgpu_device_count(void);
/* hipMemGetInfo of the device the calling thread is bound to (uvcgpu_init): free and total bytes of device memory. */
int uvcgpu_device_memory(int64_t *free_bytes, int64_t *total_bytes);
const char *uvcgpu_last_error(void);
const char *uvcgpu_version(void);

/* Replaces `Symbol2CountCoverageSet(tid, ext_beg, ext_end+1)` (main.cpp:569) together with the
 * region side arrays built just before it (main.cpp:553-563): refstring -> refstring2repeatvec
 * (main.hpp:803-874) -> the two BAQ prefix-sum arrays (main.cpp:400-429).
 * refseq = ASCII reference of [beg, end) (the caller's load_refstring result, +-MAX_STR_N_BASES halo), beg/end =
 * extended_inclu_beg_pos / extended_exclu_end_pos of main.cpp:529-530.  The per-position state then covers
 * [beg, end + 1), i.e. npos = end - beg + 1 positions, exactly like Symbol2CountCoverageSet(tid, beg, end + 1). */
int uvcgpu_region_create(uvcgpu_region_t **out, const UvcParams *params,
                         int32_t tid, int32_t beg, int32_t end, const char *refseq);
/* Re-binds the handle to another region (the next tile of a stream of tiles): as destroy + create, but the streams and, when the new
 * region is not longer than the longest one the handle has held, the device buffers are kept -- no hipMalloc / hipFree per tile. */
int uvcgpu_region_reset(uvcgpu_region_t *r, int32_t tid, int32_t beg, int32_t end, const char *refseq);
/* Copies the reads to the device (the caller keeps ownership of its buffers). */
int uvcgpu_region_set_reads(uvcgpu_region_t *r, const UvcReadSoA *reads);
/* The same for columns that are already in HBM: every pointer of `reads` is a device pointer (on the handle's device), nothing is copied.
 * The arrays must stay valid and unchanged until the handle gets other reads, is reset or destroyed; uvcgpu_region_correct_bq then edits
 * `quals` in place, as the reference edits its bam1_t (grouping.cpp:459-543).  For callers whose decoder already writes to the device, and
 * for measuring the path without the PCIe copy. */
int uvcgpu_region_set_reads_device(uvcgpu_region_t *r, const UvcReadSoA *reads);
/* Optional: apply_bq_err_correction3 (grouping.cpp:459-543) on the device copy of quals. */
int uvcgpu_region_correct_bq(uvcgpu_region_t *r);
/* The base qualities as they are on the device now (after uvcgpu_region_correct_bq if it was called); n must equal
 * UvcReadSoA::n_bases of the last set_reads.  For callers that write the corrected qualities back (the reference edits the
 * bam1_t in place, grouping.cpp:459-543) and for tests. */
int uvcgpu_region_read_quals(uvcgpu_region_t *r, uint8_t *dst, int64_t n);
/* Replaces updateByRegion3Aln (main.hpp:3665-3742): passes P1..P5b. Asynchronous on the handle's stream. */
int uvcgpu_region_accumulate(uvcgpu_region_t *r);
/* Upper bound of records a request can produce (2 symbol types x <= 8 symbols x positions, + 16 per force-output site). */
int64_t uvcgpu_region_score_size(const uvcgpu_region_t *r, const UvcScoreRequest *req);
/* Replaces the BcfFormat_symbol* call group.  Synchronous: returns after D2H of the records. */
int uvcgpu_region_score(uvcgpu_region_t *r, const UvcScoreRequest *req, UvcScoreOut *out);
/* ---- many ranges of one accumulated region in one call (a BED panel whose lines were merged into one region) ----
 * The records of a ranges call are the records of uvcgpu_region_score called once per range on the same accumulated handle -- the same
 * `req` with that range's four values put in -- concatenated in range order: every field identical (the planes and the arithmetic are the
 * same), germ_ref / germ_alt1 / germ_alt2 re-based to the returned array as kept_only does.  One gate, one set of launches, one D2H.
 *   req->pos_beg must be -1, req->base_at_pos_beg and req->region_beg 0 (the ranges carry them); req = NULL is the default request.
 *   Ranges are sorted and disjoint (ranges[i + 1].pos_beg >= ranges[i].pos_end) and each obeys the bounds rule of uvcgpu_region_score;
 *   anything else is UVCGPU_EINVAL with a message that names the range, before any launch.  n_ranges >= 1.
 * all_out, kept_only, release_state, the caller's InDel alleles, tumor keys and force_sites work as the contract above defines them. */
typedef struct UvcScoreRange {
    int32_t pos_beg, pos_end;     /* zerobased_pos, half open, as UvcScoreRequest::pos_beg / pos_end */
    int32_t base_at_pos_beg;      /* as UvcScoreRequest::base_at_pos_beg, for this range */
    int32_t region_beg;           /* as UvcScoreRequest::region_beg, for this range */
} UvcScoreRange;
/* Upper bound of the records of a ranges call (as uvcgpu_region_score_size, over the ranges' total length); -1 for a NULL argument. */
int64_t uvcgpu_region_score_ranges_size(const uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges);
int uvcgpu_region_score_ranges(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, UvcScoreOut *out);
/* ---- a score in bounded memory: the records of one request, chunk by chunk ----
 * uvcgpu_region_score sizes its device rows, its records array and the caller's buffer by the records of the whole request (14 per
 * position under all_out).  A stream runs the gate once over the whole request, cuts the record list into chunks of at most
 * `chunk_records` records on the device, and runs the per-record kernels chunk by chunk over two row sets sized by chunk_records; chunk
 * k + 1 is computed and copied while the caller works on chunk k.
 *     uvcgpu_region_score_stream_begin(r, &req, ranges, n_ranges, chunk_records, &s);
 *     while ((rc = uvcgpu_score_stream_next(s, &chunk, covered, &n_covered)) == 0)
 *         uvcgpu_region_vcf_records_ranges(r, contig, &chunk, &req_text, covered, n_covered, dst, cap, &len);   // or anything else with the chunk
 *     uvcgpu_score_stream_end(s);                                             // rc == UVCGPU_STREAM_END: all chunks were returned
 *   Request: exactly that of uvcgpu_region_score (ranges = NULL, n_ranges = 0) or of uvcgpu_region_score_ranges; all_out, kept_only, the
 *     caller's InDel alleles, tumor keys and force_sites mean what they mean there.  The request's arrays are copied by begin.
 *   Chunks: a chunk is a run of whole zerobased_pos values (both symbol types of a position stay together); chunks come in order, are
 *     disjoint and together cover the request.  The records of a chunk are the records of uvcgpu_region_score_ranges on the ranges reported
 *     in `covered` (at most max(n_ranges, 1) entries: the caller's array must hold that many): the request's ranges cut to the chunk, with
 *     base_at_pos_beg = 1 where a piece continues the previous chunk inside a range, region_beg carried over.  Every field is the one call's;
 *     germ_ref / germ_alt1 / germ_alt2 are relative to the chunk, as they are to a kept_only result.  The texts of the chunks (covered and
 *     chunk handed to uvcgpu_region_vcf_records_ranges, with a request whose pos_beg is -1) concatenate to the one call's text.
 *   Size: every chunk has at most chunk_records records -- all records of its groups, with kept_only counted before the kept groups are
 *     picked.  There is no minimum.  When one position alone has more, begin returns UVCGPU_ENOMEM, the message names the position and
 *     the count, and no stream is opened.
 *   `chunk` is a view: fields points into the stream's own page-locked buffer ([UVC_NUM_SCORE_FIELDS][capacity = chunk_records]) and stays
 *     valid until the following next / end on the stream.  next returns UVCGPU_STREAM_END behind the last chunk.
 *   release_state: the planes are released behind the last chunk's kernels -- as soon as that chunk is queued, which is during the next call
 *     that returns the chunk before it (or begin, with one or two chunks); a stream that is ended earlier keeps them.
 *   While a stream is open, score, score_ranges, accumulate, reset, set_reads and a second begin on the handle return UVCGPU_ESTATE;
 *     end is legal at any point, also mid-way; afterwards the handle scores as before.  uvcgpu_region_destroy ends an open stream.
 *   Memory: uvcgpu_score_stream_bytes_per_record() = device + page-locked host bytes that one unit of chunk_records costs, both row sets
 *     and both host buffers counted.  uvcgpu_score_stream_footprint(r) = the bytes the handle holds for scoring right now (position-sized
 *     scratch, staged request arrays, row sets, records arrays, page-locked buffers).  With a stream open
 *         footprint <= chunk_records * bytes_per_record + 96 * (positions of the region) + staged request arrays * 3 / 2 + 256 KiB.
 *     begin frees the record-sized buffers of earlier one-call scores; the row sets and host buffers are kept across streams with the same
 *     chunk_records -- nothing is allocated per chunk. */
typedef struct uvcgpu_score_stream uvcgpu_score_stream_t;
int uvcgpu_region_score_stream_begin(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges,
                                     int64_t chunk_records, uvcgpu_score_stream_t **out);
int uvcgpu_score_stream_next(uvcgpu_score_stream_t *s, UvcScoreOut *chunk, UvcScoreRange *covered, int64_t *n_covered);
int uvcgpu_score_stream_end(uvcgpu_score_stream_t *s);
int64_t uvcgpu_score_stream_bytes_per_record(void);
int64_t uvcgpu_score_stream_footprint(const uvcgpu_region_t *r);
/* ---- depth statistics of ranges of the accumulated region (the per-target coverage report) ----
 * The measures (rows of include/uvc_coverage.def, in this order): per position the raw segment depth, the fragment depth, the de-duplicated
 * family depth, the BQ-filtered family depth, the families large enough for a single-strand consensus, the duplex families -- each of the
 * BASE symbol type, summed over both strands and the six BASE symbols where the plane has them. */
enum UvcCoverageMeasure { UVC_COV_aDP = 0, UVC_COV_bDP, UVC_COV_cDP1, UVC_COV_cDP12, UVC_COV_cDP2, UVC_COV_dDP1, UVC_NCOV };
enum { UVC_COV_SUM = 0, UVC_COV_MIN = 1, UVC_COV_MAX = 2, UVC_COV_GE = 3 /* .. + 7 */, UVC_COV_MAX_THRESHOLDS = 8, UVC_COV_ROW = 11 /* 3 + 8 */ };
typedef struct UvcCoverageRange { int32_t pos_beg, pos_end; } UvcCoverageRange;   /* zero-based, half open, inside the region [beg, end + 1) */
/* One row of UVC_NCOV x UVC_COV_ROW int64 per range: for every measure the sum, the minimum and the maximum of its per-position values over
 * the range and, for threshold k, the number of positions whose value is >= thresholds[k]; the slots of unused thresholds are 0.  The
 * planes are reduced on the device (one pass, every needed cell read once); nothing per position travels to the host.
 *   Legal after uvcgpu_region_accumulate and before the planes are released (a score with release_state comes after it); called before
 *   accumulate, after such a score or while a score stream is open it returns UVCGPU_EINVAL with a message and computes nothing.
 *   UVCGPU_EINVAL before any launch, the message naming the range: a range that is empty, outside the region, or begins in front of its
 *   predecessor's end (ranges are sorted and disjoint; neighbours may share an end point); n_ranges < 1; n_thresholds outside 0..8; a
 *   negative threshold or one that is not larger than the one before it.  `out` is written only by a call that returns 0. */
int uvcgpu_region_coverage(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges,
                           const int32_t *thresholds, int32_t n_thresholds /* 0..8, ascending */,
                           int64_t *out /* [n_ranges][UVC_NCOV][UVC_COV_ROW] */);
const char *uvcgpu_coverage_measure_name(int32_t id);   /* "aDP" .. "dDP1"; NULL for an id outside 0..UVC_NCOV - 1 */
/* ---- background error profile of ranges of the accumulated region (uvc1-mi355x --error-profile-out) ----
 * How often a non-reference base or an InDel symbol appears at positions that are not variant, per evidence level (rows of
 * include/uvc_errprofile.def, in this order: fragments, UMI families, BQ-filtered families, consensus-sized families, duplex families), split by
 * the reference trinucleotide.  c_L(s, p) is the level's cell of symbol s at position p, summed over both strands where the plane has them.
 *   Context of p: l, m, r = the handle's reference symbols at p - 1, p, p + 1; a position the handle holds no reference base for (in front of
 *   beg, at or behind end) counts as N.  Unless all three are A/C/G/T the position has no context: it adds 1 to no_context and nothing else.
 *   Otherwise ctx = 16 l + 4 m + r and, per level and for each of the two kinds
 *     BASE: symbols A C G T, reference symbol m;      LINK: symbols LINK_M D3P D2 D1 I3P I2 I1, reference symbol LINK_M
 *   with d = the sum of c_L over the kind's symbols and a = the largest c_L of a non-reference one: d < min_depth counts <kind>_low_depth; else
 *   a * 1000 > max_alt_permille * d counts <kind>_high_alt (the position looks variant); else <kind>_counted, and c_L(s, p) is added to the bin
 *   [ctx][s] of every symbol of the kind, the reference symbol included (the denominator's reference part).
 * A level's row: 256 BASE bins [ctx][4], 448 LINK bins [ctx][7], the 8 counters of UvcErrCounter (no_context is per position, the same in
 * every row).  Rows of disjoint position sets add. */
enum UvcErrLevel { UVC_ERRLEVEL_bDP = 0, UVC_ERRLEVEL_cDP1, UVC_ERRLEVEL_cDP12, UVC_ERRLEVEL_cDP2, UVC_ERRLEVEL_dDP1, UVC_NERRLEVEL };
enum { UVC_ERR_NCTX = 64, UVC_ERR_NBASE = 4, UVC_ERR_NLINK = 7, UVC_ERR_BASE_BINS = 0, UVC_ERR_LINK_BINS = 256 /* 64 * 4 */,
       UVC_ERR_COUNTERS = 704 /* 256 + 64 * 7 */, UVC_ERR_ROW = 712 /* + 8 */ };
enum UvcErrCounter { UVC_ERRC_BASE_counted = 0, UVC_ERRC_BASE_low_depth, UVC_ERRC_BASE_high_alt, UVC_ERRC_LINK_counted, UVC_ERRC_LINK_low_depth,
                     UVC_ERRC_LINK_high_alt, UVC_ERRC_no_context, UVC_ERRC_reserved /* 0 */, UVC_NERRC };
typedef struct UvcErrorProfileRequest { int32_t min_depth; int32_t max_alt_permille; } UvcErrorProfileRequest;
/* One profile of UVC_NERRLEVEL x UVC_ERR_ROW int64 per call, summed over all positions of all ranges; integers only, the same bits from call
 * to call.  The planes are reduced on the device in one pass (396 B per position); nothing per position travels to the host.
 *   Ranges and the legality window are those of uvcgpu_region_coverage (zero-based, half open, sorted, disjoint, inside [beg, end + 1); after
 *   accumulate, before the planes are released, no score stream open), with the same refusals.  min_depth < 1 or max_alt_permille outside
 *   0..1000 is UVCGPU_EINVAL before any launch.  `out` is written only by a call that returns 0. */
int uvcgpu_region_error_profile(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges,
                                const UvcErrorProfileRequest *req, int64_t *out /* [UVC_NERRLEVEL][UVC_ERR_ROW] */);
const char *uvcgpu_error_level_name(int32_t id);   /* "bDP" .. "dDP1"; NULL for an id outside 0..UVC_NERRLEVEL - 1 */
/* ---- UMI family statistics of ranges, from the family units of the region's reads (uvc1-mi355x --family-stats-out) ----
 * A family is one fam_id of the reads the handle holds (UvcReadSoA), as uvcgpu_group_families formed it and as the family passes of
 * accumulate consume it.  Family f has a_f / b_f = the fragments (distinct frag_id) of its strand-0 / strand-1 unit (a missing unit: 0),
 * n_f = its alignments, lo_f = its smallest pos, hi_f = its largest reference end (pos + the reference length of the CIGAR, exclusive; both
 * unclamped, from the alignments) and dflag_f = fam_dflag[f].  f overlaps range i iff lo_f < pos_end_i and hi_f > pos_beg_i.
 * One row of UVC_FAMSTAT_ROW int64 per range (sections: include/uvc_famstats.def), two blocks:
 *   TARGET (words 0..3: families, fragments = sum of a + b, alignments = sum of n, families with a >= 1 and b >= 1) over every family that
 *     overlaps the range -- with UVC_FAMRANGE_CONTINUES only over those with lo_f >= pos_beg: the range is a later piece of the target its
 *     predecessor belongs to, which counted the others.  A family may count in several targets.
 *   FIRST (words 4..): over every family that overlaps the range and has prev_end <= lo_f: the same four counters, the families with dflag
 *     bit 0 (UMI), bit 1 (duplex tag), bit 2 (amplicon), a reserved 0, size[64] (bin k - 1: a + b == k; the last: a + b >= 64) and
 *     strands[17][17] (bin [min(a, 16)][min(b, 16)]).  With prev_end = the end of the previous range of a run of sorted, disjoint ranges
 *     every family that overlaps any range is counted exactly once in the run.
 * A family is seen as the region it was grouped in sees it: next to a tile cut it may lack fragments that the fetch of the neighbouring
 * tile holds, so sums over tiles depend on the cuts. */
enum UvcFamStat { UVC_FAMSTAT_target_families = 0, UVC_FAMSTAT_target_fragments, UVC_FAMSTAT_target_alignments, UVC_FAMSTAT_target_families_both_strands,
                  UVC_FAMSTAT_families, UVC_FAMSTAT_fragments, UVC_FAMSTAT_alignments, UVC_FAMSTAT_families_both_strands,
                  UVC_FAMSTAT_families_umi, UVC_FAMSTAT_families_duplex_tag, UVC_FAMSTAT_families_amplicon, UVC_FAMSTAT_reserved,
                  UVC_FAMSTAT_size, UVC_FAMSTAT_strands, UVC_NFAMSTAT };
enum { UVC_FAMSTAT_TARGET = 0, UVC_FAMSTAT_FIRST = 4, UVC_FAMSTAT_SIZE = 12, UVC_FAMSTAT_NSIZE = 64, UVC_FAMSTAT_STRANDS = 76 /* 12 + 64 */,
       UVC_FAMSTAT_STRAND_CAP = 16, UVC_FAMSTAT_ROW = 365 /* 76 + 17 * 17 */, UVC_FAMRANGE_CONTINUES = 1 };
typedef struct UvcFamilyRange { int32_t pos_beg, pos_end, prev_end, flags; } UvcFamilyRange;   /* zero-based, half open; flags: UVC_FAMRANGE_CONTINUES */
/* Reduced on the device from the unit records of set_reads (two passes over the alignments and the units); integers only, the same bits
 * from call to call.  Legal after uvcgpu_region_set_reads / _set_reads_device of the current region (zero reads: rows of zeros), with or
 * without accumulate, after any score -- a releasing one too: it gives up the planes, not the reads -- and while a score stream is open.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason (a range by its index): called before set_reads or after a reset;
 *   NULL ranges or out; n_ranges < 1; a range that is empty or reversed, outside the region [beg, end + 1), or begins in front of its
 *   predecessor's end; prev_end > pos_beg; prev_end smaller than the predecessor's prev_end or pos_end; a flag bit other than
 *   UVC_FAMRANGE_CONTINUES.  `out` is written only by a call that returns 0. */
int uvcgpu_region_family_stats(uvcgpu_region_t *r, const UvcFamilyRange *ranges, int64_t n_ranges, int64_t *out /* [n_ranges][UVC_FAMSTAT_ROW] */);
const char *uvcgpu_family_stat_name(int32_t id);   /* "target_families" .. "strands"; NULL for an id outside 0..UVC_NFAMSTAT - 1 */
/* ---- fragment length and end-motif profile of ranges, from the fragments and family units of the region's reads (uvc1-mi355x
 * --fragment-profile-out) ----
 * All values are integers.
 *   An alignment is counted iff mapq >= min_mapq and (flag & 0x904) == 0 (not unmapped, secondary or supplementary).  Its reference span is
 *   [pos, rend), rend = pos + the reference length of the CIGAR (a CIGAR that consumes no reference counts one position, as for the family
 *   statistics); it is forward iff !(flag & 0x10).  Nothing is clamped to the region.
 *   A fragment g is one distinct (fam_id, fam_strand, frag_id) of the reads the handle holds.  Over its counted alignments nF / nR are the
 *   numbers of forward / reverse ones, loF / hiF the smallest pos and the largest rend of the forward ones, loR / hiR those of the reverse
 *   ones; lo_g = min(loF, loR), hi_g = max(hiF, hiR), L_g = hi_g - lo_g.  A fragment without a counted alignment adds nothing anywhere.
 *   Every other fragment has one kind:
 *     pair:   nF >= 1, nR >= 1, loF <= loR and hiF <= hiR (the forward end is leftmost, the reverse end rightmost: the span is the template);
 *     other:  nF >= 1 and nR >= 1 otherwise (everted, or one mate reaching past the other);
 *     single: one orientation only (the span is not a template length).
 *   A family f is one fam_id, both strand units joined.  It is sized iff it has at least one pair fragment; its template is
 *   [tlo_f, thi_f) = the smallest lo_g and the largest hi_g over its pair fragments, TL_f = thi_f - tlo_f.
 *   Ranges are UvcFamilyRange rows with the rules and refusals of uvcgpu_region_family_stats; overlap, UVC_FAMRANGE_CONTINUES and prev_end
 *   mean what they mean there, applied to [lo_g, hi_g) for the fragment counters and to [tlo_f, thi_f) for the family counters.
 * out_ranges: UVC_FRAGPROF_TARGET_ROW int64 per range, the TARGET rule (every overlapping object; with UVC_FAMRANGE_CONTINUES only those
 *   that begin at or behind pos_beg): pairs, others, singles, len_sum (the sum of L_g over the pairs), short (pairs with
 *   short_lo <= L_g <= short_hi), long (the same with the long bounds), families (sized families), a reserved 0.
 * out_profile: one row of UVC_FRAGPROF_ROW int64 per call (sections: include/uvc_fragprofile.def), the FIRST rule (an object counts iff
 *   there is a range that it overlaps and whose prev_end is at most its begin: once per call however many ranges it spans): the eight
 *   words above, families_both_strands (sized families with a pair fragment in each strand unit), ends, ends_off_region, ends_no_ref,
 *   reserved zeros up to 16 words; LEN[1024] (pairs, bin min(L_g, 1023)); FAMLEN[1024] (sized families, bin min(TL_f, 1023)); MOTIF[256].
 *   End motifs come from the reference, so soft clips and base errors do not enter.  Each pair fragment counted in the profile has two 5'
 *   ends.  With x = lo_g - beg, y = hi_g - beg and n = the positions of the region that hold a reference base (its last position holds
 *   none): the left end is usable iff x >= 0 and x + 4 <= n, its symbols are s_k = ref[x + k]; the right end is usable iff y - 4 >= 0 and
 *   y <= n, its symbols are s_k = 3 - ref[y - 1 - k] (the reverse complement; A C G T are 0..3), k = 0..3.  An end that is not usable adds
 *   to ends_off_region; a usable end with a symbol above UVC_BASE_T to ends_no_ref; any other end to ends and to
 *   MOTIF[s_0 * 64 + s_1 * 16 + s_2 * 4 + s_3].
 * A fragment and a family are seen as the region they were grouped in sees them: next to a tile cut a fragment may lack the mate that the
 * fetch of the neighbouring tile holds, so sums over tiles depend on the cuts. */
enum UvcFragProfSection { UVC_FRAGPROF_pairs = 0, UVC_FRAGPROF_others, UVC_FRAGPROF_singles, UVC_FRAGPROF_len_sum, UVC_FRAGPROF_short,
                          UVC_FRAGPROF_long, UVC_FRAGPROF_families, UVC_FRAGPROF_reserved, UVC_FRAGPROF_families_both_strands,
                          UVC_FRAGPROF_ends, UVC_FRAGPROF_ends_off_region, UVC_FRAGPROF_ends_no_ref, UVC_FRAGPROF_reserved2,
                          UVC_FRAGPROF_LEN, UVC_FRAGPROF_FAMLEN, UVC_FRAGPROF_MOTIF, UVC_NFRAGPROF };
enum { UVC_FRAGPROF_TARGET_ROW = 8, UVC_FRAGPROF_NCOUNTER = 16, UVC_FRAGPROF_NLEN = 1024, UVC_FRAGPROF_NMOTIF = 256,
       UVC_FRAGPROF_LEN_BINS = 16, UVC_FRAGPROF_FAMLEN_BINS = 1040 /* 16 + 1024 */, UVC_FRAGPROF_MOTIF_BINS = 2064 /* + 1024 */,
       UVC_FRAGPROF_ROW = 2320 /* + 256 */ };
typedef struct UvcFragmentProfileRequest { int32_t min_mapq, short_lo, short_hi, long_lo, long_hi; } UvcFragmentProfileRequest;
/* Reduced on the device from the per-alignment columns, the fragments and the unit records of set_reads; integers only, the same bits from
 * call to call.  Legal where uvcgpu_region_family_stats is: from uvcgpu_region_set_reads / _set_reads_device of the current region on (zero
 * reads: zeros), with or without accumulate, after any score and while a score stream is open.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason: what uvcgpu_region_family_stats refuses; NULL req, out_ranges or
 *   out_profile; min_mapq outside 0..255; a bound below 0; short_lo > short_hi or long_lo > long_hi.  The outputs are written only by a
 *   call that returns 0. */
int uvcgpu_region_fragment_profile(uvcgpu_region_t *r, const UvcFamilyRange *ranges, int64_t n_ranges, const UvcFragmentProfileRequest *req,
                                   int64_t *out_ranges /* [n_ranges][UVC_FRAGPROF_TARGET_ROW] */, int64_t *out_profile /* [UVC_FRAGPROF_ROW] */);
const char *uvcgpu_fragment_profile_name(int32_t id);   /* "pairs" .. "MOTIF"; NULL for an id outside 0..UVC_NFRAGPROF - 1 */
/* ---- base-quality and cycle profile of the region's reads (uvc1-mi355x --read-profile-out) ----
 * One pass over the read bases the handle holds (UvcReadSoA): what the reported qualities are worth, where along the read mismatches,
 * InDels and clips fall, and which substitutions each read class makes.  All integers.
 *   An alignment is counted iff mapq >= min_mapq.  Its class c = 2 * ((flag & 0x80) != 0) + ((flag & 0x10) != 0): R1 forward, R1 reverse,
 *   R2 forward, R2 reverse.  An alignment with l_qseq 0 adds nothing.
 *   CIGAR walk: query index q from 0, reference coordinate p from pos; M = X consume both, I S the query, D N the reference, H P nothing.
 *   Cycle of q in a read of l_qseq L: (flag & 0x10) ? L - 1 - q : q (hard clips do not count), bin cb = min(cycle, 255).  Quality bin
 *   qb = min(quality, 63), the quality being the handle's present one: after uvcgpu_region_correct_bq the corrected one.
 *   Status of every position p of the region, over ALL counted alignments and independent of the ranges: D(p) = the aligned bases (M = X)
 *   at p whose read base is A/C/G/T, X(p) = those that differ from the reference symbol; no_ref when the reference symbol is not A/C/G/T
 *   (the region's last position, which has no reference base, included); else low_depth when D < min_depth; else high_alt when
 *   X * 1000 > max_alt_permille * D; else clean.
 *   An aligned base at p inside a range adds to exactly one counter, tested in this order: bases_low_mapq (alignment not counted),
 *   bases_no_ref, bases_n (read base not A/C/G/T), bases_low_depth, bases_high_alt, else bases_clean together with Q[c][qb][k],
 *   CYC[c][cb][k] (k = 0 match, 1 mismatch against the reference symbol) and SUB[c][reference base][read base] (forward-strand codes 0..3).
 *   Unaligned events of counted alignments are gated by an anchor position alone: max(pos, p - 1) for I and S and p for D, p being the
 *   walk's reference coordinate at the op.  An anchor in no range or outside the region adds nothing; else every inserted base adds
 *   CYC[c][cb][2] and every soft-clipped base CYC[c][cb][4] at its own cycle, every D op one CYC[c][cb][3] at the cycle of query index
 *   max(0, q - 1).  N moves p and adds nothing.
 *   Every position inside a range adds 1 to the positions_* counter of its status.
 * One row of UVC_READPROF_ROW int64 per call (sections: include/uvc_readprofile.def).  Rows of disjoint position sets add. */
enum UvcReadProfSection { UVC_READPROF_Q = 0, UVC_READPROF_CYC, UVC_READPROF_SUB, UVC_READPROF_bases_low_mapq, UVC_READPROF_bases_no_ref,
                          UVC_READPROF_bases_n, UVC_READPROF_bases_low_depth, UVC_READPROF_bases_high_alt, UVC_READPROF_bases_clean,
                          UVC_READPROF_positions_no_ref, UVC_READPROF_positions_low_depth, UVC_READPROF_positions_high_alt,
                          UVC_READPROF_positions_clean, UVC_READPROF_reserved, UVC_NREADPROF };
enum { UVC_READPROF_NCLASS = 4, UVC_READPROF_NQUAL = 64, UVC_READPROF_NCYCLE = 256, UVC_READPROF_NKIND = 5 /* match mismatch ins del clip */,
       UVC_READPROF_Q_BINS = 0, UVC_READPROF_CYC_BINS = 512 /* 4 * 64 * 2 */, UVC_READPROF_SUB_BINS = 5632 /* + 4 * 256 * 5 */,
       UVC_READPROF_COUNTERS = 5696 /* + 4 * 4 * 4 */, UVC_READPROF_NCOUNTER = 16, UVC_READPROF_ROW = 5712 /* + 16 */ };
typedef struct UvcReadProfileRequest { int32_t min_mapq, min_depth, max_alt_permille; } UvcReadProfileRequest;
/* Reduced on the device in two passes over the read bases; integers only, the same bits from call to call.  Ranges: those of
 * uvcgpu_region_coverage (zero-based, half open, sorted, disjoint, inside [beg, end + 1)).  Legal where uvcgpu_region_family_stats is:
 * from uvcgpu_region_set_reads / _set_reads_device of the current region on (zero reads: only the positions_* words are non-zero), with or
 * without accumulate, after any score and while a score stream is open.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason: called before set_reads or after a reset; NULL ranges, req or
 *   out; a range list that uvcgpu_region_coverage refuses; min_mapq outside 0..255; min_depth < 1; max_alt_permille outside 0..1000.  `out`
 *   is written only by a call that returns 0. */
int uvcgpu_region_read_profile(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcReadProfileRequest *req,
                               int64_t *out /* [UVC_READPROF_ROW] */);
const char *uvcgpu_read_class_name(int32_t c);   /* "R1_fwd" "R1_rev" "R2_fwd" "R2_rev"; NULL for a class outside 0..3 */
/* ---- the alignments behind listed sites (uvc1-mi355x --site-reads-out) ----
 * Which alignments of the handle (UvcReadSoA; `read` is an alignment's index in that struct as given) show what at a short list of
 * positions.  sites[n_sites]: zero-based positions, strictly ascending, every one inside [beg, end + 1).  All integers.
 *   An alignment is counted iff mapq >= min_mapq and l_qseq > 0; others add nothing anywhere.
 *   CIGAR walk (that of uvcgpu_region_read_profile): query index q from 0, reference coordinate p from pos; M = X consume both, I S the
 *   query, D N the reference, H P nothing.
 *   Observation: a counted alignment has one observation at site s iff an M = X or D op holds s (a site inside an N op or outside the
 *   aligned span has none).  kind = 0..3 for the read base A C G T at s, 4 for any other base, 5 when s lies inside a D op.  q = the query
 *   index of that base; for kind 5 max(0, q_at_op - 1), the base in front of the op.  qual = the handle's present quality at q: after
 *   uvcgpu_region_correct_bq the corrected one.
 *   Events: an I op of length n at walk coordinate p has anchor p - 1 and adds ins_len += n, ins_q being the query index of the first
 *   inserted base of the first such op of that anchor; a D op of length n whose first deleted coordinate is p has anchor p - 1 and adds
 *   del_len += n.  An event attaches to the same alignment's observation at its anchor iff that observation exists: an event whose anchor
 *   lies in front of pos, inside an N op or is not a listed site is dropped.  Several events of one anchor add their lengths (I P I, 2I3D).
 *   counts[n_sites][8], over all observations of counted alignments and independent of alt_only: columns 0..5 the observations of each
 *   kind, column 6 those with ins_len > 0, column 7 those with del_len > 0.
 *   alt_only = 0: every observation is a row.  alt_only = 1: a row is kept iff kind == 5, ins_len > 0, del_len > 0, or kind <= 3 and the
 *   reference symbol at the site is A/C/G/T and differs from kind (the region's last position has no reference base).
 *   Rows ascend by (read, site). */
typedef struct UvcSiteReadsRequest { int32_t min_mapq; int32_t alt_only; } UvcSiteReadsRequest;
typedef struct UvcSiteRead {
    int32_t site;      /* index into `sites` */
    int32_t read;      /* index of the alignment in the UvcReadSoA */
    int32_t q;         /* query index of the observation */
    int32_t obs;       /* kind | qual << 8 */
    int32_t ins_q;     /* query index of the first inserted base; -1 without an insertion */
    int32_t ins_len;   /* summed inserted length at this anchor */
    int32_t del_len;   /* summed deleted length at this anchor */
    int32_t reserved;  /* 0 */
} UvcSiteRead;
enum { UVC_SITEREAD_A = 0, UVC_SITEREAD_C, UVC_SITEREAD_G, UVC_SITEREAD_T, UVC_SITEREAD_N, UVC_SITEREAD_DEL, UVC_SITEREAD_NKIND,
       UVC_SITEREAD_COL_INS = 6, UVC_SITEREAD_COL_DEL_AFTER = 7, UVC_SITEREAD_NCOL = 8 };
/* Found, counted and compacted on the device from the read columns, CIGARs and packed base | quality of the handle: the work is split by
 * (alignment, site) item, the kept rows are ranked by count / scan / write (no atomic decides an order), the counts are integer adds: two
 * calls return the same bytes.
 *   Sizes first, as for uvcgpu_region_callable: *n_rows and counts are always written by a call that is not refused; when row_capacity is
 *   smaller than *n_rows the call returns UVCGPU_ENOMEM and writes nothing to `rows`; a second call with enough room returns the data.
 *   Legal where uvcgpu_region_family_stats is: from uvcgpu_region_set_reads / _set_reads_device of the current region on, with or without
 *   accumulate, after any score and while a score stream is open.  Zero reads: zero rows and zero counts.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason (a site by its index): called before set_reads or after a reset;
 *   NULL sites, req, counts or n_rows; n_sites < 1; a site not strictly above its predecessor; a site outside [beg, end + 1); min_mapq
 *   outside 0..255; alt_only outside 0..1; row_capacity < 0; NULL rows with row_capacity > 0.
 *   UVCGPU_EUNSUPPORTED, the one refusal that comes behind a launch (the number is known only on the device): the (alignment, site)
 *   candidates -- the listed sites inside [pos, endpos) of the counted alignments, summed -- number 2^31 or more; pass the sites in
 *   several calls.  A refused call, this one included, writes nothing: neither *n_rows nor counts nor rows. */
int uvcgpu_region_site_reads(uvcgpu_region_t *r, const int32_t *sites, int64_t n_sites, const UvcSiteReadsRequest *req,
                             int32_t *counts /* [n_sites][8] */, UvcSiteRead *rows, int64_t row_capacity, int64_t *n_rows);
const char *uvcgpu_site_read_kind_name(int32_t kind);   /* "A" "C" "G" "T" "N" "DEL"; NULL for a kind outside 0..5 */
/* ---- clipped-read breakpoint sites (uvc1-mi355x --clip-sites-out) ----
 * Where the soft and hard clips of the handle's alignments (UvcReadSoA) pile up inside a list of ranges: the sites are found, not given.
 * All integers.
 *   An alignment is counted iff mapq >= min_mapq, (flag & 0x4) == 0 and l_qseq > 0; secondary and supplementary alignments count (split
 *   reads are the point).  rend = pos + the reference length of the CIGAR.
 *   CIGAR walk (that of uvcgpu_region_read_profile): reference coordinate p from pos; M = X D N move p.  An aligned op is M, = or X; a CIGAR
 *   without one adds nothing but the counted alignment.
 *   LEFT event (side 0): all S and H ops in front of the first aligned op; its boundary p is the walk's coordinate at that op.  RIGHT event
 *   (side 1): all S and H ops behind the last aligned op; its boundary p is the walk's coordinate behind that op.  S / H ops between aligned
 *   ops add nothing.  soft_len / hard_len: the summed S / H lengths of the event, len = soft_len + hard_len.  An event exists iff len >= 1
 *   and qualifies iff len >= min_clip; an alignment has at most one event per side.
 *   Vote bases: the query bases of the event's S ops in query order, c[0 .. soft_len).  Vote index k counts outward from the junction:
 *   c[soft_len - 1 - k] for LEFT, c[k] for RIGHT, k < min(soft_len, UVC_CLIPSITE_NCONS).  Codes 0..3 = A C G T, 4 = anything else;
 *   qualities are not read.
 *   A qualifying event is in range iff p lies inside one of `ranges` (those of uvcgpu_region_coverage).  Every other qualifying event --
 *   one whose p - beg falls outside [0, npos) included -- adds to its total alone.
 *   A site is a (p, side) whose qualifying in-range events number at least min_reads.  Sites come sorted by (p, side).
 *   spanning(p): the counted alignments with pos < p < rend (aligned on both sides of the junction, D and N included); independent of the
 *   ranges and of min_clip.
 * sites: one row of UVC_CLIPSITE_ROW int64 per site (sections: include/uvc_clipsites.def): range (index into `ranges`), pos (absolute p),
 *   side, reads (its events), reads_fwd (!(flag & 0x10)), reads_supp (flag & 0x800), reads_secondary (flag & 0x100), reads_hard (events
 *   with hard_len > 0), len_sum, len_max, mapq_sum, spanning, reserved zeros up to word 16, VOTE[32][5] (k, code).
 * totals[UVC_CLIPSITE_NTOTAL]: counted alignments; qualifying events in range; qualifying events not in range; events with
 *   1 <= len < min_clip (any p); qualifying events at kept sites; three zeros.
 * reads (written only with want_reads = 1): one UvcClipRead per qualifying in-range event at a kept site, ascending by (read, side);
 *   `site` indexes the returned rows, `read` the UvcReadSoA as given.  *n_reads is written either way. */
enum UvcClipSiteSection { UVC_CLIPSITE_range = 0, UVC_CLIPSITE_pos, UVC_CLIPSITE_side, UVC_CLIPSITE_reads, UVC_CLIPSITE_reads_fwd, UVC_CLIPSITE_reads_supp,
                          UVC_CLIPSITE_reads_secondary, UVC_CLIPSITE_reads_hard, UVC_CLIPSITE_len_sum, UVC_CLIPSITE_len_max, UVC_CLIPSITE_mapq_sum,
                          UVC_CLIPSITE_spanning, UVC_CLIPSITE_reserved, UVC_CLIPSITE_VOTE, UVC_NCLIPSITE };
enum { UVC_CLIPSITE_NTOTAL = 8, UVC_CLIPSITE_NCOUNTER = 16, UVC_CLIPSITE_NCONS = 32, UVC_CLIPSITE_NCODE = 5, UVC_CLIPSITE_VOTE_BINS = 16,
       UVC_CLIPSITE_ROW = 176 /* 16 + 32 * 5 */, UVC_CLIPSITE_LEFT = 0, UVC_CLIPSITE_RIGHT = 1 };
enum UvcClipSiteTotal { UVC_CLIPTOTAL_alignments = 0, UVC_CLIPTOTAL_events_in_range, UVC_CLIPTOTAL_events_off_range, UVC_CLIPTOTAL_events_short,
                        UVC_CLIPTOTAL_events_at_sites };
typedef struct UvcClipSitesRequest { int32_t min_mapq, min_clip, min_reads, want_reads; } UvcClipSitesRequest;
typedef struct UvcClipRead { int32_t site, read, soft_len, hard_len; } UvcClipRead;
/* Found, counted, ranked and filled on the device from the read columns, CIGARs and bases of the handle: two passes over the alignments,
 * the sites and the event rows ranked by count / scan / write (no atomic decides an order), the row words integer adds: two calls return
 * the same bytes.
 *   Sizes first: a call that is not refused always writes totals, *n_sites and *n_reads.  It returns UVCGPU_ENOMEM when site_capacity <
 *   *n_sites, or when want_reads is set and read_capacity < *n_reads, and then writes nothing to `sites` or `reads`.
 *   Legal where uvcgpu_region_read_profile is: from uvcgpu_region_set_reads / _set_reads_device of the current region on, with or without
 *   accumulate, after any score and while a score stream is open.  Zero reads: zero sites.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason: called before set_reads or after a reset; a range list that
 *   uvcgpu_region_coverage refuses; NULL req, totals, n_sites or n_reads; min_mapq outside 0..255; min_clip < 1; min_reads < 1; want_reads
 *   outside 0..1; a negative capacity; a NULL array with a positive capacity.  A refused call writes nothing. */
int uvcgpu_region_clip_sites(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcClipSitesRequest *req,
                             int64_t *totals /* [UVC_CLIPSITE_NTOTAL] */,
                             int64_t *sites /* [site_capacity][UVC_CLIPSITE_ROW] */, int64_t site_capacity, int64_t *n_sites,
                             UvcClipRead *reads, int64_t read_capacity, int64_t *n_reads);
const char *uvcgpu_clip_site_section_name(int32_t id);   /* "range" .. "VOTE"; NULL for an id outside 0..UVC_NCLIPSITE - 1 */
/* ---- clip-site junctions: where the clipped consensus of a site lies on the region's reference (uvc1-mi355x --clip-sites-junctions 1,
 * DESIGN.md 4r) ----
 * Per row of uvcgpu_region_clip_sites the call searches the consensus of the site's votes in the reference of the region, on both strands,
 * and names the other end of the event.  All integers; of a site row only the words pos, side and VOTE are read.
 *   Reference: the n = npos - 1 positions x in [0, n) with the code refsym[x] of the region's reference character; plane index npos - 1 has
 *   no reference base and is never part of a placement.  A position is a base iff its code is <= UVC_BASE_T; any other code (N, a gap
 *   character, ..) mismatches everything.
 *   Query of a site: for k in 0 .. UVC_CLIPSITE_NCONS - 1, total_k = the sum of the five vote cells of k and winner_k = the code with the
 *   most votes, ties to the smaller code.  query_len = 1 + the largest k with total_k >= 1, 0 when there is none.  Index k is compared iff
 *   total_k >= min_votes, winner_k is 0..3 and winner_k's votes * 3 >= total_k * 2 (the upper-case rule of the S line's consensus);
 *   cmp_len = the number of compared k.  The site is searched iff cmp_len >= min_len.
 *   Placements: d = +1 for a RIGHT site, -1 for a LEFT site.  The forward placement at t has q[k] facing ref[t + d k]; the reverse placement
 *   at t has q[k] facing the complement of ref[t - d k].  A placement exists iff all query_len faced positions lie in [0, n); its
 *   mismatches are the compared k whose faced position is not a base or differs from winner_k.
 *   Partner junction of a placement, in the convention of a site's pos (plane index; reported absolute, + beg), and the side of the mate:
 *       RIGHT forward: t, LEFT       LEFT forward: t + 1, RIGHT       RIGHT reverse: t + 1, RIGHT       LEFT reverse: t, LEFT
 *   A placement counts iff its mismatches are <= max_mismatch and, with max_dist > 0, |partner - pos| <= max_dist.
 *   hist[m] = the counted placements with exactly m mismatches, m in 0..7 (0 above max_mismatch).  The best placement is the smallest by
 *   (mismatches, strand with forward first, t); n_best = hist[best_mm]; second_mm = best_mm when n_best >= 2, else the next non-empty bin,
 *   else -1.
 *   klass: UVC_CLIPCLASS_INV for a reverse best placement; forward: ADJACENT when partner == pos; RIGHT site: DEL when partner > pos, DUP when
 *   partner < pos; LEFT site: DEL when partner < pos, DUP when partner > pos.  len = |partner - pos|.
 *   mate: among the given rows (the site itself included) the one of the expected side whose pos is nearest to partner, at most mate_slop
 *   away; of two at the same distance the one with the smaller pos; its index in `sites`, -1 when there is none.  The slop absorbs
 *   microhomology, which moves the two ends of one event apart.
 *   status: UVC_CLIPJUNC_NOT_SEARCHED (0), UVC_CLIPJUNC_NOT_PLACED (1: searched, no placement counted), UVC_CLIPJUNC_PLACED (2).
 * junctions: one row of UVC_CLIPJUNC_ROW int64 per site (sections: include/uvc_clipjunc.def): site (the row's index), query_len, cmp_len,
 *   status, best_mm, n_best, second_mm, partner, strand (0 forward, 1 reverse), klass, len, mate, hist[8], reserved zeros.  Without a
 *   placement best_mm, second_mm, partner, strand, len and mate are -1, n_best is 0 and klass is UVC_CLIPCLASS_NONE.
 * totals[UVC_CLIPJUNC_NTOTAL]: sites; sites searched; sites placed; sites placed uniquely (n_best == 1); sites with a mate; three zeros. */
enum UvcClipJuncSection { UVC_CLIPJUNC_site = 0, UVC_CLIPJUNC_query_len, UVC_CLIPJUNC_cmp_len, UVC_CLIPJUNC_status, UVC_CLIPJUNC_best_mm, UVC_CLIPJUNC_n_best,
                          UVC_CLIPJUNC_second_mm, UVC_CLIPJUNC_partner, UVC_CLIPJUNC_strand, UVC_CLIPJUNC_klass, UVC_CLIPJUNC_len, UVC_CLIPJUNC_mate,
                          UVC_CLIPJUNC_hist, UVC_CLIPJUNC_reserved, UVC_NCLIPJUNC };
enum { UVC_CLIPJUNC_ROW = 24, UVC_CLIPJUNC_NTOTAL = 8, UVC_CLIPJUNC_NHIST = 8, UVC_CLIPJUNC_NOT_SEARCHED = 0, UVC_CLIPJUNC_NOT_PLACED = 1, UVC_CLIPJUNC_PLACED = 2 };
enum UvcClipJuncTotal { UVC_CLIPJTOTAL_sites = 0, UVC_CLIPJTOTAL_searched, UVC_CLIPJTOTAL_placed, UVC_CLIPJTOTAL_unique, UVC_CLIPJTOTAL_mated };
enum UvcClipClass { UVC_CLIPCLASS_NONE = 0, UVC_CLIPCLASS_DEL, UVC_CLIPCLASS_DUP, UVC_CLIPCLASS_INV, UVC_CLIPCLASS_ADJACENT, UVC_NCLIPCLASS };
typedef struct UvcClipJunctionsRequest { int32_t min_votes, min_len, max_mismatch, max_dist, mate_slop; } UvcClipJunctionsRequest;
/* Searched on the device: the reference packed once per call into 2-bit codes, a 64-bit query word and compare mask per site and strand,
 * one XOR / popcount per (window, site, strand); the best placement is a 64-bit atomicMin over the packed (mismatches, strand, t), hist is
 * integer adds: no atomic decides an order, two calls return the same bytes.
 *   `sites` are n_sites rows as uvcgpu_region_clip_sites returns them, re-uploaded; `junctions` has room for n_sites rows (no sizes-first
 *   step).  n_sites == 0 gives zero totals and success (sites and junctions may then be NULL).
 *   Legal from uvcgpu_region_create / _reset on, in every later state of that region: it reads the reference and the caller's rows, no reads
 *   and no planes; a score stream may be open.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason: a NULL argument; n_sites < 0; min_votes < 1; min_len outside
 *   1..32; max_mismatch outside 0..7; max_dist < 0; mate_slop < 0; a row whose pos - beg is outside [0, npos) or whose side is not 0 or 1;
 *   rows not strictly ascending by (pos, side).  A refused call writes nothing. */
int uvcgpu_region_clip_junctions(uvcgpu_region_t *r, const int64_t *sites /* [n_sites][UVC_CLIPSITE_ROW] */, int64_t n_sites, const UvcClipJunctionsRequest *req,
                                 int64_t *junctions /* [n_sites][UVC_CLIPJUNC_ROW] */, int64_t *totals /* [UVC_CLIPJUNC_NTOTAL] */);
const char *uvcgpu_clip_junction_section_name(int32_t id);   /* "site" .. "reserved"; NULL for an id outside 0..UVC_NCLIPJUNC - 1 */
const char *uvcgpu_clip_class_name(int32_t klass);           /* "NONE" "DEL" "DUP" "INV" "ADJACENT"; NULL for a class outside 0..4 */
/* ---- clip-site mates: where the mates of the discordant pairs that face a site cluster (uvc1-mi355x --clip-sites-mates 1) ----
 * Per row of uvcgpu_region_clip_sites the call gathers the read pairs of the handle that face the breakpoint, classes each of them and
 * clusters the mates of the discordant ones: the partner of a fusion or translocation lies on another contig or beyond the region, where
 * uvcgpu_region_clip_junctions cannot place it.  All integers; of a site row only the words pos and side are read.  mt(i) = mtid ? mtid[i]
 * : req->tid is the contig of alignment i's mate; mtid is a host column of its own, one entry per alignment of the handle in the order of
 * the UvcReadSoA as given (UvcReadSoA has no such column), uploaded per call.
 *   Pair read: alignment i is a pair read iff it is counted as in uvcgpu_region_clip_sites (mapq >= min_mapq, !(flag & 0x4), l_qseq > 0),
 *   flag & 0x1, !(flag & 0x8), !(flag & 0x900) (a supplementary line repeats its primary's mate fields) and mt(i) >= 0.  rend = the handle's
 *   end of the alignment (bam_endpos: pos + the reference length of the CIGAR, pos + 1 without one).
 *   Facing: i faces a RIGHT site p iff !(flag & 0x10), pos < p and p - window < rend <= p + overhang; i faces a LEFT site p iff flag & 0x10,
 *   rend > p and p - overhang <= pos < p + window.  One alignment may face several sites: the unit of work is the (alignment, site) item.
 *   Class of an item, the first rule that applies: UVC_CLIPMATE_OTHER_CONTIG: mt != tid; UVC_CLIPMATE_SAME_STRAND: ((flag >> 5) & 1) ==
 *   ((flag >> 4) & 1); UVC_CLIPMATE_FAR: |mpos - pos| >= min_dist; else UVC_CLIPMATE_CONCORDANT.  The three other classes are discordant;
 *   their items are the witnesses.
 *   Witness order: ascending by (site, mt, mate strand = (flag >> 5) & 1, mpos, read), mpos the mate's leftmost coordinate as the BAM gives
 *   it (signed); total, since two items of one site never share a read.
 *   Clusters: along that order a new cluster begins at the first witness of a site, at a change of mt or of mate strand, and where mpos -
 *   the previous mpos > max_gap (single linkage in one dimension).  A cluster is kept iff its pairs >= min_pairs.
 * site_rows: one row of UVC_CLIPMATE_SITE_ROW int64 per given site (include/uvc_clipmates.def): site (the row's index), facing (its items),
 *   concordant, other_contig, same_strand, far (its items by class), clusters (all of them), clusters_kept.
 * clusters: one row of UVC_CLIPMATE_ROW int64 per kept cluster, in witness order (so sorted by site): site, mtid, mate_strand, mpos_min,
 *   mpos_max (the smallest and largest mpos, 0-based leftmost coordinates, not ends), pairs (its witnesses), other_contig, same_strand, far
 *   (its witnesses by class), mapq_sum, first (the index of its first witness in the witness order, with or without want_reads), reserved 0.
 * reads (written only with want_reads = 1): one UvcClipMate per witness in witness order; `site` indexes the given rows, `read` the
 *   UvcReadSoA as given, `cluster` the returned cluster rows (-1: the witness's cluster is not kept), klass is the item's class.
 * totals[UVC_CLIPMATE_NTOTAL]: pair reads (each alignment once); facing items; concordant items; discordant items; clusters; kept clusters;
 *   sites with a kept cluster; 0. */
enum UvcClipMateSiteWord { UVC_CLIPMSITE_site = 0, UVC_CLIPMSITE_facing, UVC_CLIPMSITE_concordant, UVC_CLIPMSITE_other_contig, UVC_CLIPMSITE_same_strand,
                           UVC_CLIPMSITE_far, UVC_CLIPMSITE_clusters, UVC_CLIPMSITE_clusters_kept, UVC_NCLIPMSITE };
enum UvcClipMateClusterWord { UVC_CLIPMCLUS_site = 0, UVC_CLIPMCLUS_mtid, UVC_CLIPMCLUS_mate_strand, UVC_CLIPMCLUS_mpos_min, UVC_CLIPMCLUS_mpos_max, UVC_CLIPMCLUS_pairs,
                              UVC_CLIPMCLUS_other_contig, UVC_CLIPMCLUS_same_strand, UVC_CLIPMCLUS_far, UVC_CLIPMCLUS_mapq_sum, UVC_CLIPMCLUS_first,
                              UVC_CLIPMCLUS_reserved, UVC_NCLIPMCLUS };
enum { UVC_CLIPMATE_SITE_ROW = 8, UVC_CLIPMATE_ROW = 12, UVC_CLIPMATE_NTOTAL = 8 };
enum UvcClipMateClass { UVC_CLIPMATE_CONCORDANT = 0, UVC_CLIPMATE_OTHER_CONTIG, UVC_CLIPMATE_SAME_STRAND, UVC_CLIPMATE_FAR, UVC_NCLIPMATECLASS };
enum UvcClipMateTotal { UVC_CLIPMTOTAL_pair_reads = 0, UVC_CLIPMTOTAL_facing, UVC_CLIPMTOTAL_concordant, UVC_CLIPMTOTAL_discordant, UVC_CLIPMTOTAL_clusters,
                        UVC_CLIPMTOTAL_clusters_kept, UVC_CLIPMTOTAL_sites_kept };
typedef struct UvcClipMatesRequest { int32_t tid, min_mapq, window, overhang, min_dist, max_gap, min_pairs, want_reads; } UvcClipMatesRequest;
typedef struct UvcClipMate { int32_t site, read, cluster, klass; } UvcClipMate;
/* Gathered, ordered and clustered on the device from the read columns of the handle: a count pass and a scatter pass over the alignments
 * (the sites an alignment faces are a stretch of the ascending LEFT or RIGHT list), the witnesses of a site ranked by their keys (the slot
 * of a witness is the number of witnesses of its site with a smaller (mt, strand, mpos, read); no vendor sort, and no atomic decides an
 * order), clusters numbered by a scan over "begins a cluster", their counters integer adds, the kept ones compacted by count / scan /
 * write: two calls return the same bytes.
 *   Sizes first: a call that is not refused always writes totals, site_rows, *n_clusters (the kept clusters) and *n_reads (the witnesses).
 *   It returns UVCGPU_ENOMEM when cluster_capacity < *n_clusters, or when want_reads is set and read_capacity < *n_reads, and then writes
 *   nothing to `clusters` or `reads`.  n_sites == 0 gives zero totals and success.
 *   Legal where uvcgpu_region_clip_sites is.  Zero reads: zero counts in every row.
 *   UVCGPU_EINVAL before any launch, with a message that names the reason: called before set_reads or after a reset; NULL req, totals,
 *   n_clusters or n_reads; NULL sites or site_rows with n_sites > 0; n_sites < 0; tid < 0; min_mapq outside 0..255; window < 1; overhang <
 *   0; min_dist < 1; max_gap < 0; min_pairs < 1; want_reads outside 0..1; a negative capacity; a NULL array with a positive capacity; a
 *   row whose pos - beg is outside [0, npos) or whose side is not 0 or 1; rows not strictly ascending by (pos, side).  A refused call
 *   writes nothing.  UVCGPU_EUNSUPPORTED behind the count pass, the one refusal behind a launch: 2^31 or more facing items (pass the sites
 *   in several calls); nothing is written then either. */
int uvcgpu_region_clip_mates(uvcgpu_region_t *r, const int64_t *sites /* [n_sites][UVC_CLIPSITE_ROW] */, int64_t n_sites,
                             const int32_t *mtid /* [alignments of the handle], host; NULL: every mate on req->tid */,
                             const UvcClipMatesRequest *req, int64_t *totals /* [UVC_CLIPMATE_NTOTAL] */, int64_t *site_rows /* [n_sites][UVC_CLIPMATE_SITE_ROW] */,
                             int64_t *clusters /* [cluster_capacity][UVC_CLIPMATE_ROW] */, int64_t cluster_capacity, int64_t *n_clusters,
                             UvcClipMate *reads, int64_t read_capacity, int64_t *n_reads);
const char *uvcgpu_clip_mate_site_name(int32_t id);      /* "site" .. "clusters_kept"; NULL for an id outside 0..UVC_NCLIPMSITE - 1 */
const char *uvcgpu_clip_mate_cluster_name(int32_t id);   /* "site" .. "reserved"; NULL for an id outside 0..UVC_NCLIPMCLUS - 1 */
const char *uvcgpu_clip_mate_class_name(int32_t klass);  /* "CONCORDANT" "OTHER_CONTIG" "SAME_STRAND" "FAR"; NULL for a class outside 0..3 */
/* ---- family concordance of ranges: what the family consensus out-voted, and where the two strands of a duplex family disagree
 * (uvc1-mi355x --family-concordance-out) ----
 * Units and votes.  A unit u is one family-strand unit of the reads the handle holds (one fam_id and one strand: what the family passes of
 *   accumulate walk), with the span [u.beg, u.end) those passes give it: u.beg the smallest pos of its alignments, u.end grown over its
 *   alignments in read order as max(u.end, reference end of the alignment) + 1 (one more per alignment, as the reference's
 *   fillTidBegEndFromAlns2 has it) and clamped to the region's end + 1.  con_u(p)[s] is the number of fragments of u that vote symbol s at
 *   position p, as the family pass counts them: every fragment's own consensus of its alignments (BASE_QUALITY_MAX merge) votes once per
 *   symbol type when 2 cc - ct of that consensus (cc: the value of its symbol, ct: of the whole type) is at least 1 and, for BASE, at least
 *   fam_thres_highBQ_snv (updateByFiltering with thresholds (fam_thres_highBQ_snv, 0); the fragment's LINK consensus counts the reference
 *   symbol once, its BASE consensus leaves N and the padded deletion out where microadjust_padded_deletion_flag says so for the platform).
 *   The IonTorrent rules apply where the inferred platform is IonTorrent.
 * Per unit and position p of [u.beg, u.end) inside a range: unit_positions += 1, and units_seen += 1 where p == u.beg.  Then per symbol
 *   type (BASE: A..NN, 6 symbols; LINK: LINK_M..LINK_NN, 8 symbols) (cs, cc, ct) = the consensus of con_u(p) over the type: cs the first
 *   symbol with the most votes, cc its votes, ct all votes of the type (fill_consensus without the reference-once and the padded rule: the
 *   call in front of cDP12).  ct == 0 adds 1 to base_no_vote / link_no_vote and nothing else.  Otherwise k is the bin of ct among
 *   1, 2, 3, 4, 5-7, 8-15, 16-31, 32+ (UVC_FAMCONC_NBIN = 8) and
 *     BASE: the reference symbol of p is that of the handle; a position without one (the region's last position, `end`) or with one that
 *       is not A/C/G/T adds 1 to base_no_ref and nothing else.  Otherwise refclass = 0 when cs is the reference symbol, else 1, and
 *       base[refclass][k][cs][s] += con_u(p)[s] for the six symbols s (the diagonal: the agreeing votes), base_pos[refclass][k][0] += 1 and
 *       base_pos[refclass][k][1] += 1 when cc == ct (unanimous).
 *     LINK: link[k][cs][s] += con_u(p)[s] for the eight symbols and link_pos[k][0..1] the same way; no reference gate.
 * Duplex families: those the duplex pass of accumulate walks -- fam_dflag bit 1 set and both strand units present.  Per family and position
 *   p of [min(beg0, beg1), max(end0, end1)) inside a range, and per symbol type, v_j is the vote unit j (j = its strand) casts in the
 *   duplex pass: the cs of the consensus of con_j(p) over the type (BASE: over A..T only where the padded-deletion rule applies) when
 *   max(2 cc, ct) - ct >= 1, else "none"; a unit that does not cover p: "none".  (none, none) adds 1 to duplex_no_vote (once per type) and
 *   nothing else.  Otherwise LINK: dup_link[v0][v1] += 1 (9 x 9, vote 8 = none); BASE: a position without an A/C/G/T reference symbol adds
 *   1 to duplex_base_no_ref, every other one dup_base[ref][v0][v1] += 1 (4 x 7 x 7, vote 6 = none).  The cells off the diagonal with two
 *   votes are the strand conflicts the duplex pass settles silently (the smaller symbol wins).
 * One row of UVC_FAMCONC_ROW int64 per call (sections: include/uvc_famconcord.def), every word a sum over the (unit, position) pairs whose
 * position lies in a range: rows of disjoint position sets add.  Integers only, the same bits from call to call.
 * A family is seen as the region it was grouped in sees it: next to a tile cut it may lack fragments that the fetch of the neighbouring
 * tile holds, so its votes -- and sums over tiles -- depend on the cuts. */
enum UvcFamConc { UVC_FAMCONC_base = 0, UVC_FAMCONC_base_pos, UVC_FAMCONC_link, UVC_FAMCONC_link_pos, UVC_FAMCONC_dup_base, UVC_FAMCONC_dup_link,
                  UVC_FAMCONC_counters, UVC_NFAMCONC };
enum { UVC_FAMCONC_NBIN = 8, UVC_FAMCONC_NBASE = 6, UVC_FAMCONC_NLINK = 8, UVC_FAMCONC_BASE = 0, UVC_FAMCONC_BASE_POS = 576 /* 2 * 8 * 6 * 6 */,
       UVC_FAMCONC_LINK = 608 /* + 2 * 8 * 2 */, UVC_FAMCONC_LINK_POS = 1120 /* + 8 * 8 * 8 */, UVC_FAMCONC_DUP_BASE = 1136 /* + 8 * 2 */,
       UVC_FAMCONC_DUP_LINK = 1332 /* + 4 * 7 * 7 */, UVC_FAMCONC_COUNTERS = 1413 /* + 9 * 9 */, UVC_FAMCONC_ROW = 1429 /* + 16 */ };
enum UvcFamConcCounter { UVC_FAMCONCC_units_seen = 0, UVC_FAMCONCC_unit_positions, UVC_FAMCONCC_base_no_vote, UVC_FAMCONCC_link_no_vote,
                         UVC_FAMCONCC_base_no_ref, UVC_FAMCONCC_duplex_no_vote, UVC_FAMCONCC_duplex_base_no_ref,
                         UVC_FAMCONCC_reserved /* 7..15: 0 */, UVC_NFAMCONCC = 16 };
/* The votes are evaluated again on the device, once per (unit, position) of the ranges, from what accumulate leaves beside the planes: the
 * fragment records in position order, the contribution table of the InDel reads and the InDel-phred track as P1 edited it.  So the call
 * is legal after uvcgpu_region_accumulate of the current reads, until uvcgpu_region_set_reads / _set_reads_device, _reset or
 * _correct_bq end that accumulate -- after any score, a releasing one too (it gives up the planes, which the call does not read), and
 * while a score stream is open.  A handle whose set_reads brought zero reads has nothing to accumulate: there the call gives a row of zeros.
 *   Ranges: the rules and refusals of uvcgpu_region_coverage (zero-based, half open, sorted, disjoint, inside [beg, end + 1)).
 *   UVCGPU_EINVAL before any launch, with a message that names the reason (a range by its index): a NULL handle; called before set_reads,
 *   after a reset, or before the accumulate of the current reads; NULL ranges or out; n_ranges < 1; a range that is empty or reversed,
 *   outside the region, or begins in front of its predecessor's end.  `out` is written only by a call that returns 0. */
int uvcgpu_region_family_concordance(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, int64_t *out /* [UVC_FAMCONC_ROW] */);
const char *uvcgpu_family_concordance_section_name(int32_t id);   /* "base" .. "counters"; NULL for an id outside 0..UVC_NFAMCONC - 1 */
/* ---- callable-region intervals of ranges of the accumulated region (uvc1-mi355x --callable-out) ----
 * m_k(p) is measure k of uvcgpu_region_coverage at position p (UvcCoverageMeasure).  The mask of p has bit k = UVC_CALL_LOW_<measure k> set
 * when min_depth[k] > 0 and m_k(p) < min_depth[k], UVC_CALL_EXCESS_aDP when max_aDP > 0 and m_0(p) > max_aDP, UVC_CALL_NO_COVERAGE when
 * m_0(p) == 0 (the bits and their order: include/uvc_callable.def); a criterion of 0 is not tested, and an untested measure is not read.
 * p is callable iff its mask is 0.  A run is a maximal stretch of consecutive positions of ONE range with equal masks: runs never cross
 * a range border, even where two ranges touch and the masks on both sides are equal. */
enum UvcCallableBit { UVC_CALL_LOW_aDP = 0, UVC_CALL_LOW_bDP, UVC_CALL_LOW_cDP1, UVC_CALL_LOW_cDP12, UVC_CALL_LOW_cDP2, UVC_CALL_LOW_dDP1,
                      UVC_CALL_EXCESS_aDP, UVC_CALL_NO_COVERAGE, UVC_NCALLBIT };
typedef struct UvcCallableRequest { int32_t min_depth[UVC_NCOV]; int32_t max_aDP; } UvcCallableRequest;   /* 0 = not tested */
typedef struct UvcCallableRun { int32_t range, pos_beg, pos_end, mask; } UvcCallableRun;   /* range: index into `ranges`; zero-based, half open */
/* The runs of every range, sorted by (range, pos_beg); the runs of a range tile it exactly.  Classified, counted and compacted on the
 * device (integers only: the same bytes from call to call); nothing per position travels to the host, only 16 bytes per run.
 *   Sizes first, as for uvcgpu_region_indel_alleles: *n_runs always receives the number of runs; when run_capacity is smaller the call
 *   returns UVCGPU_ENOMEM and writes nothing to `runs`; a second call with enough room returns the data.
 *   Ranges and the window in which the call is legal: as for uvcgpu_region_coverage (sorted, disjoint, inside [beg, end + 1); after
 *   accumulate, before the planes are released, while no score stream is open).  UVCGPU_EINVAL before any launch, with a message that names
 *   the reason (a range by its index): every refusal of uvcgpu_region_coverage; a negative min_depth[k] or max_aDP; a NULL req or n_runs;
 *   run_capacity < 0; a NULL runs with run_capacity > 0.  A refused call writes neither *n_runs nor runs.  An all-zero request is legal:
 *   only UVC_CALL_NO_COVERAGE can then be set. */
int uvcgpu_region_callable(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcCallableRequest *req,
                           UvcCallableRun *runs, int64_t run_capacity, int64_t *n_runs);
const char *uvcgpu_callable_bit_name(int32_t bit);   /* "LOW_aDP" .. "NO_COVERAGE"; NULL for a bit outside 0..UVC_NCALLBIT - 1 */
/* ---- microsatellite length-shift tallies of ranges of the accumulated region (uvc1-mi355x --msi-out) ----
 * Positions in these rules are region-relative (x = position - beg); the rows carry absolute positions.  RTR_* are the STR planes of
 * UVC_F_RTR as accumulate leaves them: the microsatellites as the caller itself sees them (indelphred, the BAQ sums, INFO/RU;RC).
 *   Locus: a position h inside some range is a locus head iff RTR_begpos[h] == h, 1 <= RTR_unitlen[h] <= max_unitlen,
 *     RTR_tracklen[h] >= min_tracklen and RTR_tracklen[h] / RTR_unitlen[h] >= min_units (integer division).  Its tract is
 *     [h, h + RTR_tracklen[h]); it belongs to the range that holds h, and its tract may leave that range.  A track whose own head position
 *     was given to a longer neighbouring track (RTR_begpos[h] != h) is no locus.  Loci come sorted by head, so by (range, position).
 *   UVC_MSI_EDGE in flags: h == 0 or h + tracklen >= npos - 1 -- the tract holds the first or the last reference base of the region (the
 *     region's last position npos - 1 has no base of its own), so the region cut may have truncated it.  Its depths and histograms are 0.
 *   depth[4]: the minimum over the tract of the measures bDP, cDP12, cDP2, dDP1 of uvcgpu_region_coverage (UVC_COV_*), the measures kept
 *     beside the four allele counters below (the duplex allele counter is kept beside cDPD / dDP2: depth[3] is a measure of the same
 *     families, not its denominator).  The row holds counts and depths, no ratios.
 *   Allele rows: every device row (x, symbol, len, inserted bases, cnt[strand * 4 + level]) of the InDel allele tables; a strand
 *     contributes its four counters only where its fragment counter cnt[strand * 4] is positive, the two strands are summed: the sums of
 *     the rows of uvcgpu_region_indel_alleles (bAD1, cAD1, c2AD, c2dAD = levels 0..3) over (refpos, symbol, len, sequence).
 *   A deletion sits on its first deleted base x.  It goes to the locus h = RTR_begpos[x] if h is a reported locus without EDGE: a unit
 *     shift of -len / unit iff len % unit == 0 and x + len <= h + tracklen, else OTHER.
 *   An insertion sits on q = x, the position of the base right of the inserted bases (the CIGAR walk's reference coordinate at the I op:
 *     the position LINK_I* is counted at).  It goes to the locus h = RTR_begpos[q] if that is a reported locus (q lies in its tract);
 *     failing that, for q > 0, to h = RTR_begpos[q - 1] if that is a reported locus whose tract ends at q (an insertion behind the last
 *     unit).  Without EDGE: a unit shift of +len / unit iff len % unit == 0 and inserted base i == ref[h + ((q - h + i) mod unit)] for
 *     every i, else OTHER.  A row that reaches no reported locus adds nothing.
 *   hist[level][13]: bins 0..5 = shifts -6..-1, bins 6..11 = +1..+6, longer shifts clamped into the -6 / +6 bins, bin 12 = OTHER.
 * One row of UVC_MSI_ROW int32 per locus (sections: include/uvc_msi.def): range, pos_beg (absolute, zero-based), tracklen, unitlen, flags,
 * depth[4], hist[4][13], zeros. */
enum UvcMsiSection { UVC_MSI_range = 0, UVC_MSI_pos_beg, UVC_MSI_tracklen, UVC_MSI_unitlen, UVC_MSI_flags, UVC_MSI_depth, UVC_MSI_hist, UVC_MSI_reserved, UVC_NMSI };
enum { UVC_MSI_NLEVEL = 4, UVC_MSI_MAXSHIFT = 6, UVC_MSI_NBIN = 13 /* 2 * 6 + OTHER */, UVC_MSI_OTHER = 12, UVC_MSI_DEPTH = 5, UVC_MSI_HIST = 9,
       UVC_MSI_ROW = 64 /* 9 + 4 * 13 + 3 */, UVC_MSI_EDGE = 1 };
typedef struct UvcMsiRequest { int32_t min_tracklen, min_units, max_unitlen; } UvcMsiRequest;   /* each at least 1 */
/* Found, compacted, measured and binned on the device (integers only: the same bytes from call to call); 256 bytes per locus travel home.
 *   Sizes first, as for uvcgpu_region_callable: *n_loci always receives the number of loci; when locus_capacity is smaller the call returns
 *   UVCGPU_ENOMEM and writes nothing to `loci`.  Zero loci is legal.
 *   Ranges and the window in which the call is legal: as for uvcgpu_region_callable.  UVCGPU_EINVAL before any launch, with a message that
 *   names the reason (a range by its index): every refusal of uvcgpu_region_coverage; a request field below 1; a NULL req or n_loci;
 *   locus_capacity < 0; a NULL loci with locus_capacity > 0.  A refused call writes neither *n_loci nor loci. */
int uvcgpu_region_msi(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcMsiRequest *req,
                      int32_t *loci /* [locus_capacity][UVC_MSI_ROW] */, int64_t locus_capacity, int64_t *n_loci);
const char *uvcgpu_msi_section_name(int32_t id);   /* "range" .. "reserved"; NULL for an id outside 0..UVC_NMSI - 1 */
/* Raw state access (the reference reads members directly, main.cpp:682-688, 759-760, 801-816). */
int64_t uvcgpu_region_field_bytes(const uvcgpu_region_t *r, int32_t field_group);
int uvcgpu_region_fetch(uvcgpu_region_t *r, int32_t field_group, void *dst, int64_t dst_bytes);
/* The InDel allele tables of the accumulated region (see UvcGapRow).  *n_rows / *seq_bytes receive the sizes needed; rows / seq are
 * filled when the capacities suffice, else UVCGPU_ENOMEM is returned and nothing is written.  Replaces the direct reads of
 * getPosToIseqToData / getPosToDlenToData / pos2iseq2data_cDP2 / pos2iseq2data_c2dDP in main.hpp:5350-5376. */
int uvcgpu_region_indel_alleles(uvcgpu_region_t *r, UvcGapRow *rows, int64_t row_capacity, int64_t *n_rows,
                                uint8_t *seq, int64_t seq_capacity, int64_t *seq_bytes);
/* The haplotype links of the accumulated region: the three std::vector<HapLink> that updateByRegion3Aln hands back (hap_bq, hap_fq,
 * hap_f2q, main.hpp:3665-3670) -- per link the mutated (refpos, symbol) pairs that one fragment (bq) / one UMI family (fq; f2q: confirmed by
 * the family vote) carried together, how many fragments / families on each strand carried exactly this set, and, for the three most
 * frequent sets, how many carried a superset (updateHapMap, main.hpp:3596-3663).  Links come grouped by `which` in the reference's order;
 * FORMAT/bHap, cHap, c2Hap of a record list the links that contain its (refpos, symbol) (main.cpp:82-97, main.hpp:5380-5404).
 * Sizes first (UVCGPU_ENOMEM with *n_links / *n_mut_ints set), then the data, as for uvcgpu_region_indel_alleles.  Needs the planes. */
typedef struct UvcHapLink {
    int32_t which;              /* 0 bq (fragments, duplicates kept), 1 fq (families), 2 f2q (families, tier-2 consensus) */
    int32_t n_muts;             /* pairs of this link */
    int64_t mut_off;            /* index of its first int in `muts`: refpos, symbol, refpos, symbol, ... */
    int32_t fr_cnt[2];          /* HapLink::fr_cnts */
    int32_t other_cnt[2];       /* HapLink::other_hap_cnts, -1 -1 beyond the phasing_haplotype_max_detail_cnt most frequent links */
} UvcHapLink;
int uvcgpu_region_hap_links(uvcgpu_region_t *r, UvcHapLink *links, int64_t link_capacity, int64_t *n_links,
                            int32_t *muts, int64_t mut_capacity, int64_t *n_mut_ints);
/* Every plane value of chosen positions, one row of uvcgpu_region_n_columns() int64 values per position: the groups in UvcField order
 * (PREP32 .. DUPLEX; RTR and BAQ are not part of a row), the planes of a group in the group's array order, i.e. column =
 * uvcgpu_region_column_base(group) + plane.  Positions outside the region give a row of zeros.  Replaces the getByPos() reads of
 * BcfFormat_symboltype_init / BcfFormat_symbol_init for the few positions whose records are written (main.hpp:3889-4251). */
int32_t uvcgpu_region_n_columns(void);
int32_t uvcgpu_region_column_base(int32_t field_group);   /* -1 for RTR / BAQ / out of range */
int uvcgpu_region_fetch_columns(uvcgpu_region_t *r, const int32_t *refpos, int64_t n, int64_t *dst /* [n][n_columns] */);

/* ---------------------------------------------------------------- VCF text ------ */
/* The header and the record lines of the reference's output for the scored records of a region: generate_vcf_header (the ##FILTER /
 * ##FORMAT / ##INFO / ##contig lines and the #CHROM line) and append_vcf_record + bcfrec::streamAppendBcfFormat (main.hpp:6027-6272,
 * bcf_formats_generator1.cpp:135-527, 643-690): CHROM POS ID REF ALT QUAL FILTER INFO FORMAT and the sample column with every FORMAT tag
 * of FORMAT_STRING_PER_REC(_WITHOUT_SSCS), in the reference's order and separators, bHap / cHap / c2Hap from uvcgpu_region_hap_links.
 * Not produced here: FORMAT/note (should_add_note) and the GERMLINE lines of output_germline.
 * Both return UVCGPU_ENOMEM with *len = the size needed when `capacity` is too small. */
const char *uvcgpu_vcf_format_keys(int32_t with_tier2_consensus_tags);
/* tumor_sample_name: NULL, or -- for the normal sample of a T/N pair with is_tumor_format_retrieved -- the name of the tumor VCF's sample,
 * which becomes a second sample column of the #CHROM line (generate_vcf_header, main.hpp:5785, 5881) */
int uvcgpu_vcf_header(const UvcParams *params, const char *sample_name, const char *tumor_sample_name, const char *const *contig_names,
                      const int64_t *contig_lens, int32_t n_contigs, char *dst, int64_t capacity, int64_t *len);
/* The same with the three lines that state facts about the caller's run, in the reference's places (main.hpp:5792-5794, 5870-5874):
 * ##fileDate=<file_date> (the reference prints strftime("%F %T")), ##reference=<reference_fname>, ##variantCallerCommand=<command_line>
 * (the reference joins argv with two blanks behind each word).  NULL leaves a line out.  Every other line -- ##ALT, ##FILTER, ##INFO,
 * ##FORMAT with their Description texts, ##phasing, ##variantCallerInferredParameters, #CHROM -- is the reference's, byte for byte;
 * ##variantCallerVersion names this library. */
int uvcgpu_vcf_header_ex(const UvcParams *params, const char *sample_name, const char *tumor_sample_name, const char *const *contig_names,
                         const int64_t *contig_lens, int32_t n_contigs, const char *file_date, const char *reference_fname,
                         const char *command_line, char *dst, int64_t capacity, int64_t *len);
/* `scored` is what uvcgpu_region_score filled for this region (all records, in order: the REF record of a position supplies the first
 * value of every Number=R tag); the lines of the records with out != 0 and keep != 0 are written.  The planes must not have been
 * released (UvcScoreRequest::release_state = 0).  `req` is the request of that score call (NULL = its defaults): its tumor_keys (normal
 * sample of a T/N pair), and its zerobased_pos range [pos_beg, pos_end), base_at_pos_beg and region_beg for the MGVCF block lines
 * (OUTVAR_MGVCF, main.cpp:655-735) and the ADDITIONAL_INDEL_CANDIDATE lines (main.cpp:759-799), which are written in front of the
 * records of their position. */
int uvcgpu_region_vcf_records(uvcgpu_region_t *r, const char *contig_name, const UvcScoreOut *scored, const UvcScoreRequest *req,
                              char *dst, int64_t capacity, int64_t *len);
/* The text of a ranges call: `scored` is what uvcgpu_region_score_ranges filled for (req, ranges); the result is the concatenation of the
 * texts uvcgpu_region_vcf_records gives for the single-range calls, MGVCF block and ADDITIONAL_INDEL_CANDIDATE lines included (a block looks
 * up to 1001 positions past its range's end into the region).  The block statistics of all ranges come in one device round trip. */
int uvcgpu_region_vcf_records_ranges(uvcgpu_region_t *r, const char *contig_name, const UvcScoreOut *scored, const UvcScoreRequest *req,
                                     const UvcScoreRange *ranges, int64_t n_ranges, char *dst, int64_t capacity, int64_t *len);
/* Optional: page-lock a caller buffer that is handed to the library again and again (the records buffer of uvcgpu_region_score, read
 * arrays of uvcgpu_region_set_reads): copies then run at PCIe speed.  Unpin before freeing the buffer. */
int uvcgpu_pin_host_buffer(void *p, int64_t bytes);
int uvcgpu_unpin_host_buffer(void *p);
/* Page-locked host memory owned by the library (hipHostMalloc): the safe home of a records buffer that lives as long as a handle.  Pinning
 * a heap buffer in place works, but heap pages change roles -- memory that once was the (read-only mapped) source of a pageable upload and
 * was freed can come back as the buffer the records are written to, and the copy then faults ("write access to a read-only page"). */
int uvcgpu_host_alloc(void **p, int64_t bytes);
int uvcgpu_host_free(void *p);
int uvcgpu_region_sync(uvcgpu_region_t *r);
/* Record counts of the last uvcgpu_region_score on this handle: scored in all, and returned (fewer with UvcScoreRequest::kept_only). */
int uvcgpu_region_last_score_counts(const uvcgpu_region_t *r, int64_t *scored, int64_t *returned);
/* Self-check (a TEST entry point) of the three statements about ALL planes that scoring and the zero fill of a reused handle rely on:
 * (1) a cell of a symbol's planes at a position can be non-zero only if the symbol is the position's reference base / LINK_M or is marked
 * in the position's occupancy word (every writer of any other cell marks it: uvc_device.h occ_mark; uvc_kernels_score.hip type_mask);
 * (2) a (plane family, symbol, 4 096-position block) nobody marked holds only zeros (the fill skips it, the gather skips its FAMINFO /
 * DUPLEX planes); (3) cIAQ / cIAD / cIDQ of a strand are non-zero only behind a P5 bucket of that (strand, position).
 * Sweeps every plane of the last accumulate; *n_violations = cells that contradict one of them (0 expected).
 * The test suite and the soak scripts run it behind every accumulate (UVCGPU_CHECK_PRESENCE=1 in uvc_amd/region.py). */
int uvcgpu_region_check_presence(uvcgpu_region_t *r, int64_t *n_violations);
/* Measurement hooks (bench.py): HIP-event timing of every kernel of the LAST accumulate, recorded on the handle's stream.
 * kernel_times returns the number of kernels; `names` receives their names separated by ';'.  The report calls add their stages to
 * the list (at most 32 entries in all); set_profiling starts it anew, as an accumulate does. */
int uvcgpu_region_set_profiling(uvcgpu_region_t *r, int on);
int uvcgpu_region_kernel_times(uvcgpu_region_t *r, char *names, int names_bytes, float *ms, int capacity);
/* For tests only: the queue of mismatching bases of the LAST accumulate (one item per base of a work-list entry that differs from the
 * reference: the alignment's rank, the position, symbol | value << 8), in the order the device happened to write it.  Waits for the
 * handle's streams; copies min(*n, cap) items to `out`; *n is the device's count, *total (may be NULL) the count set_reads made. */
typedef struct UvcMisItem { int32_t rank, epos, symval; } UvcMisItem;
int uvcgpu_region_debug_mis_queue(uvcgpu_region_t *r, UvcMisItem *out, int64_t cap, int64_t *n, int64_t *total);
void uvcgpu_region_destroy(uvcgpu_region_t *r);

/* ---------------------------------------------------------------- BGZF inflate on the device -- */
/* Replaces the zlib inflate behind htslib's bgzf_read for a batch of BGZF blocks (grouping.cpp:617-731 reads every alignment through it):
 * n raw DEFLATE payloads at comp + in_off[i] (in_len[i] bytes: the block without its 12 + XLEN header bytes and its 8 footer bytes) are
 * inflated to out + out_off[i] (out_len[i] = ISIZE bytes).  comp and out are HOST buffers of comp_bytes / out_bytes bytes.  The outputs
 * must tile one span of `out` in block order (out_off[i + 1] == out_off[i] + out_len[i], as a reader's batch does; UVCGPU_EINVAL otherwise):
 * only that span is written.  One lane per block, the Huffman tables of a wave's 64 decoders in LDS (uvc_inflate.hip).  The
 * CRC-32 of the footer is left to the caller (uvcio checks it on the returned bytes).  The signature is uvcio_inflate_fn of uvcio.h: pass
 * the function to uvcio_set_inflater.  Needs uvcgpu_init on the calling thread; UVCGPU_EINVAL names the first block whose stream is corrupt. */
int uvcgpu_bgzf_inflate(void *ctx, const uint8_t *comp, int64_t comp_bytes, const int64_t *in_off, const int32_t *in_len,
                        const int64_t *out_off, const int32_t *out_len, int64_t n_blocks, uint8_t *out, int64_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UVCGPU_H_INCLUDED */
