// uvc_prep.h -- interface between uvc_host.cpp and uvc_prep.hip (the device-side preparation of uvcgpu_region_set_reads).
#ifndef UVC_PREP_H
#define UVC_PREP_H
#include "uvc_device.h"

// the UvcReadSoA columns as device pointers
struct UvcPrepIn {
    int64_t n_reads, n_bases, n_cigar_ops; int32_t n_fams;
    const int32_t *pos, *mpos, *isize, *nm, *l_qseq, *n_cigar, *frag_id, *fam_id;
    const uint16_t *flag; const uint8_t *mapq, *fam_strand, *fam_dflag;
    const int64_t *seq_off, *cigar_off;
    const uint32_t *cigars;
    const uint8_t *quals;        // [n_bases]
    const int32_t *zero_qual;    // device word: some quality byte of the column is 0 (set by the kernels that pack base | quality); NULL: not known
};
// device arrays (owned by the allocator's context) and host-side totals
struct UvcPrepOut {
    int32_t *endpos, *kind, *dflag_of, *frag_of, *fs_of, *p2_first, *complex_ids;
    int32_t *frag_beg, *frag_strand;   // FragRec::beg / strand as columns (keys of the fragment order)
    int64_t *table_off, *item_off, *gap_off;
    FragRec *frags; FsRec *fss;
    int32_t *generic_fs, *generic_sorted, *sweep_frags, *dup_units; int64_t *dup_off;
    int32_t *p2_aln, *p2_beg, *p2_end, *p2_qb, *p2_cls;   // P2 work-list entries in read order (the caller sorts them by (class, begin))
    int32_t n_frags, n_fs, n_complex, n_simple, n_generic, n_dup, n_sweep, n_frag_strand0;
    int32_t max_frag_span, max_unit_span, max_unit_frags, max_p2_span, max_frag_depth, any_amplicon;
    int32_t p2_off[5];
    int64_t n_p2, table_rows, item_slots, gap_slots, ins_total, work, dup_work;
};
typedef void *(*UvcPrepAlloc)(void *ctx, size_t bytes, int zero);   // device memory that lives as long as the reads of the handle; NULL on failure
extern "C" int uvc_prep_reads(const UvcPrepIn *in, const UvcParams *P, int32_t rbeg, int32_t rend, int64_t npos, UvcPrepAlloc alloc, void *ctx, hipStream_t s,
                              UvcPrepOut *out, char *errmsg, int errcap);
// after uvcgpu_region_correct_bq: FragRec::stat_kind 2 and the sweep list for the fragments that now hold a base without value
extern "C" int uvc_prep_zero_value_qual(const UvcParams *P);
extern "C" void uvc_prep_requalify(const uint8_t *quals, const int64_t *seq_off, const int32_t *l_qseq, const UvcParams *P, int32_t n_frags, FragRec *frags, int32_t *sweep_frags, int32_t n_sweep, int32_t *n_joined, hipStream_t s);
#endif
