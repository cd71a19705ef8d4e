// uvc_launch.h -- the host-kernel boundary inside libuvcgpu.so: every launcher and helper that one HIP translation unit defines and another
// calls, and the structs that cross with them (by value into a kernel, or as a table the host fills and a kernel reads).  Each file that
// defines or calls one of these includes this header, so the compiler checks every definition against the one declaration.
#ifndef UVC_LAUNCH_H
#define UVC_LAUNCH_H
#include "uvc_device.h"
#include "uvc_link.h"

// the caller's columns as they are (uvcgpu_region_set_reads) + what uvc_prep.hip derives per read; by value into k_aln_bm / k_aln_prelude.
// fast_rank: the slot of a simple alignment's entry in RegionDev::frec2, -1 for every other alignment (k_gather4)
struct RawReads {
    const int32_t *pos, *endpos, *mpos, *isize, *nm, *l_qseq, *n_cigar, *frag, *fs, *dflag, *kind, *fast_rank;
    const uint16_t *flag; const uint8_t *mapq;
    const int64_t *seq_off, *cigar_off, *table_off, *item_off, *gap_off;
};
static_assert(sizeof(RawReads) == 19 * sizeof(void *), "RawReads is 19 device pointers");
// optional per-kernel HIP-event timing on the handle's own stream (bench.py roofline leg): the entries of uvcgpu_region_kernel_times
struct UvcProf { int on; int n; const char *name[32]; hipEvent_t ev[32][2]; };
// One more entry around what is launched between the two calls on stream s: -1 (and nothing recorded) with profiling off, without a UvcProf
// or with the 32 entries taken; the events of an entry are created at its first use and live as long as the handle.
static inline int uvc_prof_begin(UvcProf *p, const char *name, hipStream_t s) {
    if (!p || !p->on || p->n >= 32) return -1;
    const int i = p->n++;
    p->name[i] = name;
    if (!p->ev[i][0]) { hipEventCreate(&p->ev[i][0]); hipEventCreate(&p->ev[i][1]); }
    hipEventRecord(p->ev[i][0], s);
    return i;
}
static inline void uvc_prof_end(UvcProf *p, int i, hipStream_t s) { if (i >= 0) hipEventRecord(p->ev[i][1], s); }
// one range of uvcgpu_region_score_ranges on the device: [beg, end) in zerobased_pos, first = the compact position of beg (exclusive prefix
// of the lengths), flags bit 0 = base_at_pos_beg
struct UvcScoreRangeDev { int beg, end, first, flags; };
static_assert(sizeof(UvcScoreRangeDev) == 16, "the host uploads the range table as 16-byte rows");
// one chunk of a streamed score (k_chunk_cut writes the table, the host reads it back): first group of the request (even: a position
// boundary), group count, first record, record count
struct UvcChunkDev { long long g0, ng, r0, nr; };
static_assert(sizeof(UvcChunkDev) == 32, "the host reads the chunk table back as 32-byte rows");
// one range of the plane readers (uvcgpu_region_coverage, _error_profile, _callable): plane index of the range's first position; its first
// compact position (the exclusive prefix of the lengths).  Entry n_ranges of a table: { 0, n_total }.  The host builds it in one place
// (range_table of uvc_host.cpp), the kernels look a compact position up through UvcRangeCursor.
struct UvcRangeRow { int x0, first; };
static_assert(sizeof(UvcRangeRow) == 8, "the host uploads the range table as 8-byte rows");
// A lane's range: compact positions [first, next), plane index x0 of the first, kept while the lane's positions stay inside.  uvc_range_find
// moves it to the last range whose first compact position is <= i (ranges are not empty: `first` strictly ascends), i in [0, n_total).
struct UvcRangeCursor { int rid = -1, first = 0, next = 0, x0 = 0; };
DEV void uvc_range_find(UvcRangeCursor &g, const UvcRangeRow *tab, int n_ranges, long long i) {
    if (i >= g.first && i < g.next) return;
    int lo = 0, hi = n_ranges;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tab[mid].first <= i) lo = mid; else hi = mid; }
    g.rid = lo; g.first = tab[lo].first; g.x0 = tab[lo].x0; g.next = tab[lo + 1].first;
}
// uvcgpu_region_family_stats: smallest pos and largest reference end of the alignments of one family-strand unit (scratch the host sizes)
struct UvcUnitSpan { int lo, hi; };
static_assert(sizeof(UvcUnitSpan) == 8, "the host sizes the span scratch as 8-byte rows");
// uvcgpu_region_fragment_profile: smallest pos and largest reference end of the counted forward and of the counted reverse alignments of one
// fragment (scratch the host sizes; a unit's template span of that call is a UvcUnitSpan)
struct UvcFragSpan { int loF, hiF, loR, hiR; };
static_assert(sizeof(UvcFragSpan) == 16, "the host sizes the fragment span scratch as 16-byte rows");

// What the three score launchers share (host-side aggregate; ScorePrep of uvc_host.cpp owns one).  ranges: the device table of
// uvcgpu_region_score_ranges or NULL; n_compact: the length of the compact axis the ranges make.  force_sites: device copy of
// UvcScoreRequest::force_sites or NULL.  scratch: uvc_score_scratch_bytes (one call) / uvc_score_stream_pos_bytes (stream).
struct UvcScoreIn {
    const RegionDev *R; const UvcParams *P; const UvcScoreRequest *req;
    const UvcIndelAllele *alleles; const int32_t *allele_rows; int64_t n_alleles;
    const UvcGapRow *gap_rows; const uint8_t *gap_seq; const UvcTumorKey *tkeys;
    char *scratch; const int32_t *force_sites;
    const UvcScoreRangeDev *ranges; int64_t n_ranges, n_compact;
};
// The streams and events of one accumulate (host-side aggregate): the handle's stream, the two side streams (NULL: everything on `s`) and
// the events of the forks and joins between them (see uvc_launch_accumulate).
struct UvcAccStreams { hipStream_t s, side, side3; hipEvent_t e_fork, e_join, e_fork2, e_join3, e_stat, e_alleles, e_link_fork, e_link_join; };
// elements of one tile of the reports' tile scan = threads of a block (uvc_launch_tile_sums)
#define UVC_SCAN_TILE 256
static inline int64_t uvc_scan_tiles(int64_t n) { return (n + UVC_SCAN_TILE - 1) / UVC_SCAN_TILE; }

extern "C" {
// ---- uvc_kernels_acc.hip ----
void uvc_launch_correct_bq(const RegionDev *R, int bq_max, int bq_inc, hipStream_t s);
void uvc_launch_pack_bq(const uint8_t *bases, const uint8_t *quals, uint16_t *bq, int64_t n, int32_t *bad, hipStream_t s);
void uvc_launch_build_p2list(const RegionDev *R, const int32_t *fast_rank, const int32_t *aln, const int32_t *cbeg, const int32_t *cend, const int32_t *qb, hipStream_t s);
void uvc_launch_prelude(const RegionDev *R, const RawReads *W, const UvcParams *P, hipStream_t s);
void uvc_launch_zero_state(char *slab, const ZeroPlane *planes, int n_planes, uint8_t *dirty, int ndblk, int64_t npos, hipStream_t s);
void uvc_launch_check_dirty(const RegionDev *R, unsigned long long *d_n_bad, hipStream_t s);
// link_eager: the completion pass of LINK_M over every window inside the accumulate (UVCGPU_LINK=eager), else over the windows with an InDel mark at its end
void uvc_launch_accumulate(const RegionDev *R, const UvcParams *P, int half_ratio_phred, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_dup_work,
                           const UvcAccStreams *st, int link_eager, UvcProf *prof);
// the completion pass of LINK_M for a scope of windows (uvc_link.h); split: what uvc_acc_split_windows said at the accumulate.  d_xs (POSITIONS):
// entry t is d_xs[t * xs_stride] - xs_off.  An INDEL or POSITIONS pass of the plain forms takes the sparse form (UVCGPU_LINK_FORM forces);
// kname: its name in the profile
int uvc_acc_split_windows(const RegionDev *R);
int uvc_acc_p2_plain(const RegionDev *R, const UvcParams *P);   // the plain P2 forms: only their base pass carries the five cells of LINK_M, so only they can be lazy
void uvc_launch_link_complete(const RegionDev *R, const UvcParams *P, int split, int scope, const int32_t *d_xs, int64_t n_xs, int xs_stride, int xs_off,
                              const char *kname, UvcProf *prof, hipStream_t s);
void uvc_launch_hap_cand(const RegionDev *R, const HapWork *H, int units, hipStream_t s);
void uvc_launch_hap_events(const RegionDev *R, const UvcParams *P, const HapWork *H, int units, int n_cand, hipStream_t s);
// uvcgpu_region_family_concordance: two stages (the units, the duplex families with the fold of the copies), each one entry of
// uvcgpu_region_kernel_times.  d_tab = the n_ranges + 1 rows of UvcRangeRow; dup_units / dup_off: the duplex work list of
// uvc_launch_accumulate; d_out: one row of UVC_FAMCONC_ROW words; d_scratch: uvc_famconcord_scratch_cells() words
void uvc_launch_famconcord(const RegionDev *R, const UvcParams *P, const UvcRangeRow *d_tab, int n_ranges, const int32_t *dup_units, int n_dup, const int64_t *dup_off, int64_t n_dup_work,
                           long long *d_out, long long *d_scratch, UvcProf *prof, hipStream_t s);
const char *uvc_famconcord_section_name(int id);
int64_t uvc_famconcord_scratch_cells(void);
// ---- uvc_kernels_score.hip ----
// The staged rows, their layouts and the sizes below come from one table (uvc_score_rows.h).  The caller zeroes the first
// uvc_score_scratch_zero_bytes of in->scratch on the stream in front of uvc_launch_score / uvc_launch_score_gate; the record counts (all
// records, kept records) are its first two int64.  d_fields_kept (kept_only): a second [fields][capacity] array.  In both forms the rows
// per record hold `capacity` / `chunk_records` records and the rows per group min(groups of the request, that many) groups.
int uvc_launch_score(const UvcScoreIn *in, int32_t *d_fields, int64_t capacity, int32_t *d_fields_kept, hipStream_t s);
size_t uvc_score_scratch_bytes(int64_t npos_scored, int64_t capacity);
size_t uvc_score_scratch_zero_bytes(int64_t npos_scored, int64_t capacity);
// the streamed form (uvcgpu_region_score_stream_*): one gate pass + the chunk cut (the header of 4 x int64 and the UvcChunkDev table at
// uvc_score_stream_table_offset of the scratch), then the per-record kernels per chunk into a row set: `win` is the chunk's table entry,
// win_groups a bound of its active groups that sizes the grids (at most its groups, its records and the rows)
int uvc_launch_score_gate(const UvcScoreIn *in, int64_t chunk_records, int64_t tab_cap, hipStream_t s);
int uvc_launch_score_chunk(const UvcScoreIn *in, char *set, int64_t chunk_records, int with_kept, const UvcChunkDev *win, int64_t win_groups, hipStream_t s);
size_t uvc_score_set_bytes(int64_t chunk_records, int64_t ngroups, int with_kept);
size_t uvc_score_set_bytes_per_record(void);
int32_t *uvc_score_set_fields(char *set, int64_t chunk_records, int64_t ngroups, int kept);
size_t uvc_score_stream_pos_bytes(int64_t npos_scored, int64_t tab_cap);
size_t uvc_score_stream_table_offset(int64_t npos_scored);
void uvc_launch_check_presence(const RegionDev *R, unsigned long long *d_n_bad, hipStream_t s);
void uvc_launch_block_stats(const RegionDev *R, const UvcParams *P, int64_t x0, int64_t n, int32_t *d_out, hipStream_t s);
void uvc_launch_block_stats_windows(const RegionDev *R, const UvcParams *P, const long long *d_win, int n_win, int64_t n, int32_t *d_out, hipStream_t s);
// ---- uvc_report_common.hip: the kernels several reports launch ----
// the array scan (the block counts of the callable and the MSI call, the waves' row counts of the site call, the tile sums below): in
// place, a[i] becomes the sum of a[0 .. i), a[n] -- one element behind the input -- the total (one block of 1 024 threads)
void uvc_launch_block_scan(int *d_a, int n, hipStream_t s);
// the tile scan of n values, d_out[i] = the sum of the values in front of i and d_out[n] their total, in three launches: tile_sums into
// uvc_scan_tiles(n) + 1 ints, uvc_launch_block_scan over them, tile_prefix (d_out may be d_in).  chunks: 0 scans the values as they are,
// 1 the 64-element chunks of each length, ceil(v / 64)
void uvc_launch_tile_sums(const int32_t *d_in, int64_t n, int chunks, int32_t *d_tile_sums, hipStream_t s);
void uvc_launch_tile_prefix(const int32_t *d_in, int n, int chunks, const int32_t *d_tile_pref, int32_t *d_out, hipStream_t s);
// d_out[i] = the sum over `shards` copies of a row of `cells` words, laid one behind the other in d_parts
void uvc_launch_sum_fold(const long long *d_parts, int shards, int cells, long long *d_out, hipStream_t s);
// ---- uvc_coverage.hip, uvc_errprofile.hip: d_tab = the n_ranges + 1 rows of UvcRangeRow ----
void uvc_launch_coverage(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const int32_t *thr, int n_thr, long long *d_out, long long *d_scratch, int64_t scratch_rows, hipStream_t s);
const char *uvc_coverage_name(int id);
int64_t uvc_coverage_scratch_rows(int n_ranges, int64_t n_total);
void uvc_launch_errprofile(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, int min_depth, int max_alt_permille, long long *d_out, long long *d_scratch, hipStream_t s);
const char *uvc_errprofile_level_name(int id);
int64_t uvc_errprofile_scratch_cells(void);
// ---- uvc_famstats.hip: pos / endpos / fs_of = the per-alignment columns of RawReads; d_span: n_fs rows of scratch; d_ranges: the caller's
// n_ranges rows; d_rows: n_ranges rows of UVC_FAMSTAT_ROW words ----
void uvc_launch_famstats(const RegionDev *R, const int32_t *pos, const int32_t *endpos, const int32_t *fs_of, UvcUnitSpan *d_span, const UvcFamilyRange *d_ranges, int n_ranges, long long *d_rows, hipStream_t s);
const char *uvc_famstats_name(int id);
// ---- uvc_fragprofile.hip: W = the per-alignment columns (pos, endpos, frag, flag, mapq are read); d_fspan: n_frags rows and d_uspan: n_fs
// rows of scratch; d_ranges: the caller's n_ranges rows; d_out: n_ranges rows of UVC_FRAGPROF_TARGET_ROW words and the profile row of
// UVC_FRAGPROF_ROW words behind them; d_parts: uvc_fragprofile_copies() rows of UVC_FRAGPROF_ROW words ----
void uvc_launch_fragprofile(const RegionDev *R, const RawReads *W, const UvcFragmentProfileRequest *req, UvcFragSpan *d_fspan, UvcUnitSpan *d_uspan, const UvcFamilyRange *d_ranges, int n_ranges,
                            long long *d_out, long long *d_parts, hipStream_t s);
const char *uvc_fragprofile_name(int id);
int64_t uvc_fragprofile_copies(void);
// ---- uvc_readprofile.hip: three stages, each one entry of uvcgpu_region_kernel_times.  d_dx / d_x: npos ints each (zero at the start: the depth
// differences, on return of the status stage the depth; the mismatches); d_status: npos bytes; d_parts: uvc_readprofile_copies() rows of
// UVC_READPROF_ROW words, zero at the start; d_out: one row; d_scratch: uvc_readprofile_scratch_ints(n_alns, npos) ints.  A handle without
// reads runs the status stage and the fold of the bin stage alone ----
void uvc_launch_readprofile_depth(const RegionDev *R, const RawReads *W, int64_t n_bases, int min_mapq, int32_t *d_dx, int32_t *d_x, int32_t *d_scratch, hipStream_t s);
void uvc_launch_readprofile_status(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int min_depth, int max_alt_permille, int32_t *d_dx, const int32_t *d_x, uint8_t *d_status,
                                   long long *d_parts, int32_t *d_scratch, hipStream_t s);
void uvc_launch_readprofile_bin(const RegionDev *R, const RawReads *W, int64_t n_bases, int min_mapq, const uint8_t *d_status, long long *d_parts, long long *d_out, const int32_t *d_scratch, hipStream_t s);
const char *uvc_readprofile_class_name(int c);
int64_t uvc_readprofile_copies(void);
int64_t uvc_readprofile_scratch_ints(int64_t n_alns, int64_t npos);
// ---- uvc_sitereads.hip: two stages, each one entry of uvcgpu_region_kernel_times.  d_sites: the caller's n_sites positions; d_counts:
// n_sites rows of UVC_SITEREAD_NCOL ints, zero at the start; d_scratch: uvc_sitereads_scratch_ints(n_alns, n_sites) ints, the first two zero
// at the start: behind the count they hold the 64-bit number of (alignment, site) items, and entry uvc_sitereads_rows_at the number of kept
// rows.  The write follows a count with the same arguments; d_rows: room for that many rows ----
void uvc_launch_sitereads_count(const RegionDev *R, const RawReads *W, const int32_t *d_sites, int n_sites, const UvcSiteReadsRequest *req, int32_t *d_counts, int32_t *d_scratch, hipStream_t s);
void uvc_launch_sitereads_write(const RegionDev *R, const RawReads *W, const int32_t *d_sites, int n_sites, const UvcSiteReadsRequest *req, int32_t *d_scratch, UvcSiteRead *d_rows, hipStream_t s);
int64_t uvc_sitereads_scratch_ints(int64_t n_alns, int64_t n_sites);
int64_t uvc_sitereads_rows_at(int64_t n_alns, int64_t n_sites);
const char *uvc_sitereads_kind_name(int k);
// ---- uvc_clipsites.hip: two stages, each one entry of uvcgpu_region_kernel_times.  d_tab = n_ranges + 1 rows; d_totals: UVC_CLIPSITE_NTOTAL
// words and d_pos: uvc_clipsites_pos_ints(npos) ints, both zero at the start; d_keys: key_room ints (no call has more sites than
// min(2 positions of the ranges, 2 alignments)); d_scratch: uvc_clipsites_scratch_ints(n_alns, npos) ints: behind the find, entry
// uvc_clipsites_sites_at holds the number of sites and entry uvc_clipsites_reads_at the number of event rows.  The fill follows a find with
// the same arguments; d_rows: n_sites rows of UVC_CLIPSITE_ROW words, zero at the start; d_reads: room for the event rows, or NULL ----
void uvc_launch_clipsites_find(const RegionDev *R, const RawReads *W, const UvcRangeRow *d_tab, int n_ranges, const UvcClipSitesRequest *req, long long *d_totals, int32_t *d_pos,
                               int32_t *d_keys, int64_t key_room, int32_t *d_scratch, hipStream_t s);
void uvc_launch_clipsites_fill(const RegionDev *R, const RawReads *W, const UvcRangeRow *d_tab, int n_ranges, const UvcClipSitesRequest *req, const int32_t *d_pos, const int32_t *d_keys,
                               int n_sites, const int32_t *d_scratch, long long *d_rows, UvcClipRead *d_reads, hipStream_t s);
int64_t uvc_clipsites_pos_ints(int64_t npos);
int64_t uvc_clipsites_scratch_ints(int64_t n_alns, int64_t npos);
int64_t uvc_clipsites_sites_at(int64_t n_alns, int64_t npos);
int64_t uvc_clipsites_reads_at(int64_t n_alns, int64_t npos);
const char *uvc_clipsites_name(int id);
// ---- uvc_clipjunc.hip: four stages, each one entry of uvcgpu_region_kernel_times.  d_ref2 / d_inv: uvc_clipjunc_ref_words(npos) 64-bit words
// each (the pack writes all of them); d_sites: the caller's n_sites rows of UVC_CLIPSITE_ROW words; d_query: uvc_clipjunc_query_bytes(n_sites)
// bytes, d_best: n_sites words and d_hist: n_sites x UVC_CLIPJUNC_NHIST ints, all three written by the queries stage for every site;
// d_mpos / d_midx: the plane indices and row indices of the n_left LEFT sites ascending, behind them those of the RIGHT sites; d_rows:
// n_sites rows of UVC_CLIPJUNC_ROW words.  The stages follow each other with the same arguments.  uvc_clipjunc_naive: 1 in a build of the
// file with -DUVC_CLIPJUNC_NAIVE (the byte-per-base search the packed one is tested and measured against; its pack launches nothing) ----
void uvc_launch_clipjunc_pack(const RegionDev *R, unsigned long long *d_ref2, unsigned long long *d_inv, hipStream_t s);
void uvc_launch_clipjunc_queries(const RegionDev *R, const long long *d_sites, int n_sites, const UvcClipJunctionsRequest *req, void *d_query, unsigned long long *d_best, unsigned *d_hist, hipStream_t s);
void uvc_launch_clipjunc_search(const RegionDev *R, const unsigned long long *d_ref2, const unsigned long long *d_inv, const void *d_query, int n_sites, const UvcClipJunctionsRequest *req,
                                unsigned long long *d_best, unsigned *d_hist, hipStream_t s);
void uvc_launch_clipjunc_finish(const RegionDev *R, const void *d_query, int n_sites, const UvcClipJunctionsRequest *req, const unsigned long long *d_best, const unsigned *d_hist,
                                const int32_t *d_mpos, const int32_t *d_midx, int n_left, long long *d_rows, hipStream_t s);
int64_t uvc_clipjunc_ref_words(int64_t npos);
int64_t uvc_clipjunc_query_bytes(int64_t n_sites);
const char *uvc_clipjunc_name(int id);
const char *uvc_clipjunc_class_name(int k);
int uvc_clipjunc_naive(void);
// ---- uvc_clipmates.hip: five stages (count, scatter, rank, cut, reduce), each one entry of uvcgpu_region_kernel_times; the host waits behind
// the count, the cut and the reduce.
// L: the site lists and the mtid column on the device.  d_rows: n_sites rows of UVC_CLIPMATE_SITE_ROW words, d_totals: UVC_CLIPMATE_NTOTAL
// words and d_site_ints: uvc_clipmates_site_ints(n_sites) ints, all three zero at the start.  Behind the count the ints at
// uvc_clipmates_n_witnesses_at / _n_rank_blocks_at hold the two numbers the scatter and the rank need (n_wit >= 1); d_key / d_okey: n_wit words each;
// d_wit_ints: uvc_clipmates_witness_ints(n_wit) ints.  Behind the cut the int at uvc_clipmates_n_clusters_at holds n_clus; d_crow: n_clus
// rows of UVC_CLIPMATE_ROW words, zero at the start; d_out: room for n_clus rows; d_reads: n_wit rows or NULL; d_clus_ints:
// uvc_clipmates_cluster_ints(n_clus) ints.  Behind the reduce the int at uvc_clipmates_n_kept_at holds the number of rows in d_out ----
struct UvcClipMateLists { const int32_t *spos, *sidx, *mtid; int n_sites, n_left; };
void uvc_launch_clipmates_count(const RawReads *W, int64_t n_alns, const UvcClipMateLists *L, const UvcClipMatesRequest *req, long long *d_rows, long long *d_totals, int32_t *d_site_ints, hipStream_t s);
void uvc_launch_clipmates_scatter(const RawReads *W, int64_t n_alns, const UvcClipMateLists *L, const UvcClipMatesRequest *req, int32_t *d_site_ints, int n_wit,
                                  unsigned long long *d_key, int32_t *d_wit_ints, hipStream_t s);
void uvc_launch_clipmates_rank(const UvcClipMateLists *L, const int32_t *d_site_ints, int n_wit, int n_rank_blocks, const unsigned long long *d_key, unsigned long long *d_okey,
                               int32_t *d_wit_ints, hipStream_t s);
void uvc_launch_clipmates_cut(const UvcClipMateLists *L, const UvcClipMatesRequest *req, const int32_t *d_site_ints, int n_wit, const unsigned long long *d_okey, int32_t *d_wit_ints, hipStream_t s);
void uvc_launch_clipmates_reduce(const RawReads *W, const UvcClipMateLists *L, const UvcClipMatesRequest *req, int n_wit, int n_clus, const unsigned long long *d_okey, int32_t *d_wit_ints,
                                 long long *d_crow, long long *d_rows, long long *d_out, UvcClipMate *d_reads, int32_t *d_clus_ints, hipStream_t s);
int64_t uvc_clipmates_site_ints(int64_t n_sites);
int64_t uvc_clipmates_witness_ints(int64_t n_wit);
int64_t uvc_clipmates_cluster_ints(int64_t n_clus);
const int32_t *uvc_clipmates_n_witnesses_at(const int32_t *d_site_ints, int64_t n_sites);
const int32_t *uvc_clipmates_n_rank_blocks_at(const int32_t *d_site_ints, int64_t n_sites);
const int32_t *uvc_clipmates_n_clusters_at(const int32_t *d_wit_ints, int64_t n_wit);
const int32_t *uvc_clipmates_n_kept_at(const int32_t *d_clus_ints, int64_t n_clus);
const char *uvc_clipmates_site_name(int id);
const char *uvc_clipmates_cluster_name(int id);
const char *uvc_clipmates_class_name(int k);
// ---- uvc_callable.hip: d_tab = n_ranges + 1 rows; d_mask: n_total bytes; d_blocks: uvc_callable_blocks(n_total) + 1 ints, the last one the
// number of runs once the count has run; d_runs: room for that many runs.  The emit follows a count with the same arguments ----
void uvc_launch_callable_count(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const UvcCallableRequest *req, unsigned char *d_mask, int *d_blocks, hipStream_t s);
void uvc_launch_callable_emit(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const unsigned char *d_mask, const int *d_blocks, UvcCallableRun *d_runs, hipStream_t s);
int64_t uvc_callable_blocks(int64_t n_total);
const char *uvc_callable_name(int bit);
// ---- the scalar DEV functions of the scoring and accumulate kernels on their own, for tests: one thread per row of `in` (n rows of n_in
// doubles; integer arguments travel as doubles, all below 2^31) writes a row of `out` (n_out doubles; integer results as doubles).  The op
// fixes how many arguments a row holds and how many results it gives: a call with fewer, an unknown op or n < 1 launches nothing and
// returns -1.  uvc_launch_math_probe hands the ops of uvc_kernels_acc.hip on to uvc_launch_math_probe_acc, which checks its own three ops the same way ----
enum UvcProbeOp {
    UVC_PROBE_phred2nat, UVC_PROBE_numstates2phred, UVC_PROBE_numstates2deciphred, UVC_PROBE_prob2odds, UVC_PROBE_logit2,
    UVC_PROBE_binom_llr,                 // prob, a, b
    UVC_PROBE_dp4,                       // bidir, overseq_disabled, then dp4's eleven arguments -> 2
    UVC_PROBE_indel_len_rusize_phred_s,  // indel_len, repeatunit_size (not 0)
    UVC_PROBE_indel_phred_s,             // ampfact, rs, rn
    UVC_PROBE_more_STR_s,                // rulen1, rc1, rulen2, rc2, strmax
    UVC_PROBE_norm_fa, UVC_PROBE_i32_as_x86,
    UVC_PROBE_het_lodq,                  // a1, a2, expfrac, powlaw_exponent
    UVC_PROBE_normv_quals,               // its eleven arguments -> 4
    UVC_PROBE_normv_quals2,              // its seven arguments -> 4
    UVC_PROBE_symbols_mutated,           // ref, alt
    UVC_PROBE_sscs_phred,                // con, alt, fam_phred_sscs_indel_open, _indel_ext, _transition_CG_TA, _transition_AT_GC, _transversion_CG_AT, _transversion_other, tumor_vcf_fname_nonempty
    UVC_PROBE_infer_max_qual,            // 16 bucket counts, max_qual, dec_qual (> 0), totDP -> maxvqual, argmaxAD, argmaxBQ
    UVC_PROBE_infer_max_qual_regs,       // 16 bucket counts, max_qual, totDP -> the same three
    UVC_PROBE_infer_max_qual_one,        // bucket index, its count, max_qual, dec_qual, totDP: a histogram with one bucket filled -> the same three
    UVC_PROBE_infer_max_qual_regs_one,   // the same row (dec_qual is not read) through infer_max_qual_regs
    UVC_PROBE_proton_cigarlen2phred, UVC_PROBE_phred2prob, UVC_PROBE_phred2prob_tab,   // (uvc_kernels_acc.hip)
    UVC_PROBE_END
};
int uvc_launch_math_probe(int op, int64_t n, const double *in, int n_in, double *out, int n_out, hipStream_t s);
int uvc_launch_math_probe_acc(int op, int64_t n, const double *in, int n_in, double *out, int n_out, hipStream_t s);
// ---- uvc_msi.hip: d_tab = n_ranges + 1 rows; d_blocks: uvc_msi_blocks(n_total) + 1 ints, the last one the number of loci once the kernels
// have run; d_heads: `room` ints (the region-relative head of each locus, ascending); d_rows: `room` rows of UVC_MSI_ROW ints, zero at the
// start.  Loci beyond `room` are counted and not written; room 0 runs the count alone ----
void uvc_launch_msi(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const UvcMsiRequest *req, int *d_blocks, int32_t *d_heads, int32_t *d_rows, int64_t room, hipStream_t s);
int64_t uvc_msi_blocks(int64_t n_total);
const char *uvc_msi_name(int id);
// ---- uvc_gap.hip: the rocPRIM sorts and the small gathers ----
size_t uvc_gap_sort_tmp_bytes(size_t n);
int uvc_gap_sort(void *tmp, size_t tmp_bytes, const unsigned long long *kin, unsigned long long *kout, const unsigned long long *vin, unsigned long long *vout, size_t n, int end_bit, hipStream_t s);
size_t uvc_sort32_tmp_bytes(size_t n);
int uvc_sort_by_pos_cls(const int32_t *d_pos, const int32_t *d_cls, int32_t beg, int pos_bits, int cls_bits, int64_t n, uint32_t *work /* [4 n] */, void *tmp, size_t tmp_bytes, hipStream_t s);
void uvc_launch_gather4(const uint32_t *perm, int64_t n, const int32_t *a0, const int32_t *a1, const int32_t *a2, const int32_t *a3, int32_t *o0, int32_t *o1, int32_t *o2, int32_t *o3,
                        const int32_t *kind, int64_t n_alns, int32_t *slot, hipStream_t s);
void uvc_launch_rank_from_sorted(const uint32_t *perm, int64_t n, int64_t n_first, int32_t *out_ids, int32_t *rank, hipStream_t s);
void uvc_launch_gather_columns(const char *const *base, const int32_t *first_col, const int32_t *elem, int64_t npos, const int32_t *d_xs, int64_t n, long long *d_out, hipStream_t s);
// ---- uvc_prep.hip (uvc_prep_reads itself: uvc_prep.h) ----
size_t uvc_prep_compact_tmp_bytes(int64_t n);
int uvc_prep_compact(const int32_t *l_qseq, const int32_t *n_cigar, int64_t n, int64_t n_bases, const uint8_t *bases4, int64_t n_b4, const uint8_t *quals, int64_t *seq_off_out, const int64_t *seq_off_in,
                     int64_t *cigar_off_out, int64_t *b4_off, uint8_t *bases_out, uint16_t *bq_out, int32_t *bad, void *tmp, size_t tmp_bytes, hipStream_t s);
}
#endif
