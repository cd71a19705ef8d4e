/* uvcio.h -- C ABI of the file readers in front of the MI355X UVC hot path ("next" row N3).
 *
 * Replaces the htslib calls of the reference's ingest: sam_open / sam_hdr_read / sam_index_load / sam_itr_queryi / sam_itr_next
 * (grouping.cpp:157-314, 617-731) and fai_load / faidx_fetch_seq (main.cpp:99-130, 529-531) -- BGZF + BAM + BAI and FASTA + .fai,
 * written against the SAM/BAM specification (SAMv1.pdf sections 4 and 5) on zlib only.  Host code, no GPU: the columns it returns are
 * exactly what include/uvcgroup.h (family assignment) and UvcReadSoA (include/uvcgpu.h) take.
 *
 * Return codes: 0 or a negative UVCGPU_E* value of uvcgpu.h; uvcio_last_error() has the text.
 */
#ifndef UVCIO_H
#define UVCIO_H
#include <stddef.h>
#include <stdint.h>
#include "uvcgpu.h"   /* UvcTumorKey, UVCGPU_E* */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct uvcio_bam uvcio_bam_t;
typedef struct uvcio_fasta uvcio_fasta_t;

/* Alignments of one query, in file order, as columns.  The arrays belong to the handle and stay valid until its next fetch / close. */
typedef struct UvcBamBatch {
    int64_t n_alns;
    const int32_t *tid, *pos, *endpos /* bam_endpos: pos + reference-consuming CIGAR lengths, pos + 1 if there are none */;
    const int32_t *mtid, *mpos, *isize;
    const uint16_t *flag;
    const uint8_t *mapq;
    const int32_t *nm;          /* NM aux tag (bam_aux2i), -1 if absent */
    const int32_t *l_qseq, *n_cigar;
    const int64_t *seq_off, *cigar_off, *qname_off;
    int64_t n_bases;
    const uint8_t *bases;       /* seq_nt16_int codes: A C G T -> 0..3, everything else 4 */
    const uint8_t *quals;
    int64_t n_cigar_ops;
    const uint32_t *cigars;     /* BAM-packed: len << 4 | op */
    int64_t n_qname_bytes;
    const char *qnames;         /* NUL-terminated names, qname_off[i] is the start of the i-th */
} UvcBamBatch;

const char *uvcio_last_error(void);

/* sam_open + sam_hdr_read + sam_index_load (<path>.bai or <path minus .bam>.bai; without an index every fetch scans the file) */
int uvcio_bam_open(uvcio_bam_t **out, const char *path);
int32_t uvcio_bam_n_refs(const uvcio_bam_t *b);
const char *uvcio_bam_ref_name(const uvcio_bam_t *b, int32_t tid);
int64_t uvcio_bam_ref_len(const uvcio_bam_t *b, int32_t tid);
int uvcio_bam_has_index(const uvcio_bam_t *b);
/* sam_itr_queryi(idx, tid, beg, end) + the sam_itr_next loop: every alignment of `tid` with pos < end and bam_endpos > beg (0-based,
 * half-open), in file order; unmapped reads placed on `tid` take part with endpos = pos + 1, as in htslib */
int uvcio_bam_fetch(uvcio_bam_t *b, int32_t tid, int64_t beg, int64_t end, UvcBamBatch *out);
void uvcio_bam_close(uvcio_bam_t *b);

/* fai_load + faidx_fetch_seq: needs <path>.fai; the sequence comes back upper-cased (main.cpp:124-127 does the same) */
int uvcio_fasta_open(uvcio_fasta_t **out, const char *path);
int64_t uvcio_fasta_seq_len(const uvcio_fasta_t *f, const char *name);      /* -1 if unknown */
int uvcio_fasta_fetch(uvcio_fasta_t *f, const char *name, int64_t beg, int64_t end, char *dst /* [end - beg] */);
void uvcio_fasta_close(uvcio_fasta_t *f);

/* BGZF writer: the block-gzipped stream the reference writes its VCF through (bgzf_open / bgzf_write / bgzf_close, main.cpp:1196-1215,
 * 1571-1583): blocks of at most 0xff00 input bytes and the 28-byte end-of-file marker.  level 0..9, anything else = 6. */
typedef struct uvcio_bgzf_writer uvcio_bgzf_writer_t;
int uvcio_bgzf_write_open(uvcio_bgzf_writer_t **out, const char *path, int32_t level);
int uvcio_bgzf_write(uvcio_bgzf_writer_t *w, const void *data, int64_t n);
int uvcio_bgzf_write_close(uvcio_bgzf_writer_t *w);

/* The region planner: SamIter::iternext without a BED file (grouping.cpp:225-312; its memory model grouping.cpp:28-67) over the
 * alignment columns of a file or query in file order.  One cut per block the reference would hand to process_batch: `flag` = 16 contig
 * changed | 8 gap of more than 200 bp | 4 per-thread memory budget | 2 end of file, `batch` = the iternext() call that returns it. */
typedef struct UvcRegionCut { int32_t tid, beg, end, flag, batch; int64_t n_reads; } UvcRegionCut;
/* The same walk as a stream (it keeps a handful of scalars between alignments): feed the alignment columns piece by piece in file order, take the
 * finished cuts as they appear, finish at the end of the file.  Memory is bounded by the piece, not by the file. */
typedef struct uvcio_planner uvcio_planner_t;
int uvcio_planner_open(uvcio_planner_t **out, const int64_t *target_len, int32_t n_targets, int32_t nthreads, int64_t mem_per_thread_mb);
int uvcio_planner_feed(uvcio_planner_t *p, const int32_t *tid, const int32_t *pos, const int32_t *endpos, const uint16_t *flag, int64_t n);
int uvcio_planner_finish(uvcio_planner_t *p);
int64_t uvcio_planner_take(uvcio_planner_t *p, UvcRegionCut *out, int64_t capacity);
int64_t uvcio_planner_pending(const uvcio_planner_t *p);
void uvcio_planner_close(uvcio_planner_t *p);
int uvcio_plan_regions(const int32_t *tid, const int32_t *pos, const int32_t *endpos, const uint16_t *flag, int64_t n,
                       const int64_t *target_len, int32_t n_targets, int32_t nthreads, int64_t mem_per_thread_mb,
                       UvcRegionCut *out, int64_t capacity, int64_t *n_out);

/* ---- the tumor VCF of a T/N pair: rescue_variants_from_vcf, main.cpp:183-398 ----
 * Reads the (block-gzipped or plain) VCF the tumor pass wrote and turns every record into the integers the normal pass reads:
 * key (contig, symbolpos, VTI[1]) with symbolpos = POS - 1 for substitutions / MGVCF block / ADDITIONAL_INDEL_CANDIDATE lines and POS for
 * InDels (main.cpp:279), FORMAT BDPb, bDPf, bDPr, CDP1x, cDP1x, cVQ1, cPCQ1, CDP2x, cDP2x, cVQ2, cPCQ2, bNMQ, vHGQ, CDP1b, cDP1f, cDP1r,
 * CDP2b (main.cpp:294-372), the presence of _C2XP (:386-388) and the length of the inserted / deleted string (REF / ALT, main.cpp:867-880).
 * Lines with a symbolic ALT other than <NON_REF> / <ADDITIONAL_INDEL_CANDIDATE> are skipped, and those two as well unless
 * is_tumor_format_retrieved (main.cpp:265-272); lines without FORMAT/VTI are skipped (:275).  The reference reads through htslib's synced
 * reader restricted to the regions of the batch; here the file is read once and queried per region.
 * `contig_names` maps CHROM to tid (the BAM header's order). */
typedef struct uvcio_tumor_vcf uvcio_tumor_vcf_t;
int uvcio_tumor_vcf_open(uvcio_tumor_vcf_t **out, const char *path, const char *const *contig_names, int32_t n_contigs, int32_t is_tumor_format_retrieved);
/* The same records without a file: the tumor pass hands its record lines over in memory (uvc1-mi355x --normal-bam).  The handle starts
 * empty; uvcio_tumor_vcf_add_lines parses record lines with the parser of uvcio_tumor_vcf_open (header lines are skipped, `sample_name`
 * is what uvcio_tumor_vcf_sample_name returns).  Lines of any number of tiles, in any order; records of one key keep the order in which
 * they were added, so after adds in genome order (tile by tile, the order a tumor VCF holds them in) fetch and n_records return what
 * uvcio_tumor_vcf_open returns on a file of the same lines.  Adds and fetches may come from several threads at once. */
int uvcio_tumor_vcf_create(uvcio_tumor_vcf_t **out, const char *sample_name, const char *const *contig_names, int32_t n_contigs,
                           int32_t is_tumor_format_retrieved);
int uvcio_tumor_vcf_add_lines(uvcio_tumor_vcf_t *v, const char *text, int64_t len);
const char *uvcio_tumor_vcf_sample_name(const uvcio_tumor_vcf_t *v);   /* last column of the #CHROM line ("" if there is none) */
int64_t uvcio_tumor_vcf_n_records(const uvcio_tumor_vcf_t *v);
/* The records of `tid` with pos_beg <= symbolpos <= pos_end, sorted by (symbolpos, symbol) -- tkis_beg .. tkis_end of main.cpp:532-533 --
 * as UvcScoreRequest::tumor_keys / tumor_sample_columns / tumor_ref_alt take them.  The arrays belong to the handle.  A handle of
 * uvcio_tumor_vcf_open: valid until it is closed.  A handle of uvcio_tumor_vcf_create: a copy in storage the handle keeps for the calling
 * thread, valid until that thread's next fetch on the handle or its close; other threads' adds and fetches leave it alone. */
int uvcio_tumor_vcf_fetch(const uvcio_tumor_vcf_t *v, int32_t tid, int32_t pos_beg, int32_t pos_end, const UvcTumorKey **keys, const char *const **sample_columns,
                          const char *const **ref_alts, int64_t *n);
void uvcio_tumor_vcf_close(uvcio_tumor_vcf_t *v);

/* Force-output sites (uvc1-mi355x --force-sites, UvcScoreRequest::force_sites) read from a BED or a VCF, plain or (block-)gzipped.
 * A file whose first line starts with ##fileformat or #CHROM is a VCF: of each record only CHROM and POS are read, and POS p is the site
 * p.  Anything else is a BED file (lines starting with #, track or browser are skipped): every base x of an interval [start, end) is the
 * site x + 1.  A site is a zerobased_pos: the VCF POS of the records it selects (BASE records of refpos POS - 1, LINK records of refpos
 * POS).  Contig names map through contig_names (the BAM header); an unknown contig or a malformed line fails with UVCGPU_EINVAL and a
 * message that names the file and the line.  The sites are sorted and de-duplicated per contig. */
typedef struct uvcio_sites uvcio_sites_t;
int uvcio_sites_open(uvcio_sites_t **out, const char *path, const char *const *contig_names, int32_t n_contigs);
int64_t uvcio_sites_count(const uvcio_sites_t *s);
/* The sites of `tid` with pos_beg <= site < pos_end, ascending: a pointer into the handle (valid until it is closed) and the count. */
int uvcio_sites_fetch(const uvcio_sites_t *s, int32_t tid, int64_t pos_beg, int64_t pos_end, const int32_t **sites, int64_t *n);
void uvcio_sites_close(uvcio_sites_t *s);

/* CRC-32 (the zlib / BGZF footer polynomial) as the reader and the writer compute it: carry-less multiplication on CPUs that have it. */
/* Where the two large columns of a batch (UvcBamBatch::bases, ::quals) live: NULL, NULL = the C heap.  A caller that hands the batch to
 * uvcgpu_region_set_reads passes page-locked memory of the GPU library here (wrappers of uvcgpu_host_alloc / uvcgpu_host_free), so that the
 * 2 x 300 MB of a 1 Mb x 300x tile travel by DMA.  Set it before the first uvcio_bam_fetch; buffers are kept and grown per BAM handle. */
void uvcio_set_column_allocator(void *(*alloc_fn)(size_t), void (*free_fn)(void *));

/* The BGZF blocks of a batch inflated somewhere else than on the host's cores.  fn gets the raw DEFLATE payloads of n blocks (in_off / in_len
 * inside comp) and the place of each block's output (out_off / out_len = the block's ISIZE) and returns 0 when every byte of every block is
 * in place; the reader then checks each block's CRC-32 itself.  Anything else (non-zero return, a CRC mismatch) and the reader inflates the
 * batch on the host as if no function had been set.  uvcgpu_bgzf_inflate (uvcgpu.h) has this signature: uvc1-mi355x --device-inflate sets
 * it (the calling thread must have selected its device, uvcgpu_init).  Batches with fewer than min_blocks blocks stay on the host.
 * Replaces bgzf_read's inflate of the reference's reader (htslib behind grouping.cpp:617-731).  Process-wide; set it before the first fetch.
 * The reader hands over whole batches: the outputs of the n blocks tile one span of `out` in block order (out_off[i + 1] == out_off[i] + out_len[i]). */
typedef int (*uvcio_inflate_fn)(void *ctx, const uint8_t *comp, int64_t comp_bytes, const int64_t *in_off, const int32_t *in_len,
                                const int64_t *out_off, const int32_t *out_len, int64_t n, uint8_t *out, int64_t out_bytes);
void uvcio_set_inflate(uvcio_inflate_fn fn, void *ctx, int32_t min_blocks);
uint32_t uvcio_crc32(const void *p, int64_t n);
/* Test hook: one raw DEFLATE stream of known output size through the library's own decoder (uvc_inflate_fast.h), which the BGZF reader tries
 * before zlib: 1 = decoded (out holds out_len bytes), 0 = declined (the reader would hand the block to zlib). */
int uvcio_inflate_raw_fast(const void *in, int64_t in_len, void *out, int64_t out_len);

/* ---- region shards ----
 * The reference balances its chunks by reads and positions (main.cpp:1380-1400).  Without reading the alignments the cost of a tile is
 * estimated from the BAI linear index: the compressed bytes between the 16 kb windows that hold its two ends (0 without an index). */
int64_t uvcio_bam_region_bytes(const uvcio_bam_t *b, int32_t tid, int64_t beg, int64_t end);
/* Cuts an ordered list of n tiles with the given costs into n_shards contiguous runs of about equal total cost: shard_of[i] is
 * non-decreasing in i, so that the outputs of the shards, concatenated in shard order, are in tile order (uvcTN.sh:92-101 does the
 * same per chromosome with bcftools concat).  A tile goes to the shard that holds the midpoint of its cost interval. */
int uvcio_plan_shards(const int64_t *cost, int64_t n, int32_t n_shards, int32_t *shard_of);
/* ---- BED lines merged into device regions (uvc1-mi355x --merge-regions) ----
 * From BED lines (tid, beg, end: 0-based, half open) in file order, the batches of consecutive lines that become one device region.  A line
 * joins the open batch when it is on the same contig, begins at or after the previous line's end plus one (the score ranges of two lines
 * include both of their end points and must stay disjoint), begins within merge_distance of the previous line's end, and keeps the batch's
 * span (its first line's begin to this line's end) within max_span; otherwise it opens a new batch.  A line longer than max_span is cut
 * into pieces of max_span, as --tile cuts it, and every piece is a batch of its own which no line joins.  Lines with end <= beg give
 * nothing.  Unsorted or overlapping files therefore still work: they merely merge less.  merge_distance 0 merges nothing.
 * One UvcBedPiece per line (or per piece of a cut line), in file order; `batch` counts up from 0.  *n_pieces = the number of pieces;
 * UVCGPU_ENOMEM when capacity is smaller (call with capacity 0 for the size). */
typedef struct UvcBedPiece { int64_t line, batch, beg, end; } UvcBedPiece;
int uvcio_plan_bed_batches(const int32_t *tid, const int64_t *beg, const int64_t *end, int64_t n_lines, int64_t merge_distance, int64_t max_span,
                           UvcBedPiece *out, int64_t capacity, int64_t *n_pieces);
/* ---- the per-target coverage report (uvc1-mi355x --coverage-out) ----
 * A table of targets (BED lines or fixed windows) and, per target, the merged statistics of the pieces that tiles report for it.  A row
 * of statistics is what uvcgpu_region_coverage returns for one range: n_measures x 11 int64, per measure sum, min, max and 8 threshold
 * counts (only the first n_thresholds are kept).  Pieces of one target are disjoint stretches of it; they merge by sum +, min, max,
 * counts +, in any order and from any thread (add_piece locks).  Positions of a target that no piece covers count as depth 0: they pull
 * the minimum to 0 and count for a threshold of 0.  A target without any piece is a row of zeros.
 * write: "#chrom beg end name len" and, per measure, <measure>_sum _min _max _ge<T>..., tab-separated, one line per target in the order of
 * add_target, integers only; a path that ends in .gz is written block-gzipped (uvcio_bgzf_write_*). */
typedef struct uvcio_coverage uvcio_coverage_t;
int uvcio_coverage_open(uvcio_coverage_t **out, const char *const *measure_names, int32_t n_measures, const int32_t *thresholds, int32_t n_thresholds /* 0..8 */);
/* beg / end: as printed (the BED line's own numbers); len: the positions of the target inside its contig.  Returns the target's index, or a negative code. */
int64_t uvcio_coverage_add_target(uvcio_coverage_t *c, const char *chrom, int64_t beg, int64_t end, const char *name /* NULL = "." */, int64_t len);
int uvcio_coverage_add_piece(uvcio_coverage_t *c, int64_t target, int64_t piece_len, const int64_t *row /* [n_measures][11] */);
int uvcio_coverage_write(const uvcio_coverage_t *c, const char *path);
void uvcio_coverage_close(uvcio_coverage_t *c);
/* ---- the background error profile (uvc1-mi355x --error-profile-out) ----
 * The sum of the profiles that tiles report (uvcgpu_region_error_profile: n_levels x 712 int64 -- per level 256 BASE bins [ctx][A C G T], 448
 * LINK bins [ctx][M D3P D2 D1 I3P I2 I1], 8 counters).  Profiles of disjoint position sets add; add locks, so pieces come in any order and
 * from any thread.
 * write: "##error_profile_min_depth=<n>" and "##error_profile_max_alt_permille=<n>", "#level\tcounter\tcount" and one line per level and
 * counter (BASE_counted BASE_low_depth BASE_high_alt LINK_counted LINK_low_depth LINK_high_alt no_context), then
 * "#level\tkind\tcontext\tsymbol\tcount\tref_count" and one line per bin of a (level, kind, context) that is not empty, in level, kind (BASE,
 * LINK), context (AAA AAC .. TTT) and symbol order; ref_count is the reference symbol's bin of the same level, kind and context (the
 * context's middle base; M).  Integers only; a path that ends in .gz is written block-gzipped (uvcio_bgzf_write_*). */
typedef struct uvcio_errprofile uvcio_errprofile_t;
int uvcio_errprofile_open(uvcio_errprofile_t **out, const char *const *level_names, int32_t n_levels, int32_t min_depth, int32_t max_alt_permille);
int uvcio_errprofile_add(uvcio_errprofile_t *e, const int64_t *profile /* [n_levels][712] */);
int uvcio_errprofile_write(const uvcio_errprofile_t *e, const char *path);
void uvcio_errprofile_close(uvcio_errprofile_t *e);
/* ---- the family concordance report (uvc1-mi355x --family-concordance-out) ----
 * The sum of the rows that tiles report (uvcgpu_region_family_concordance: 1429 int64; include/uvc_famconcord.def).  Rows of disjoint
 * position sets add; add locks, so pieces come in any order and from any thread.
 * write: "##family_concordance_sections=" with name:first:words of every section, "##family_concordance_bins=1,2,3,4,5-7,8-15,16-31,32+",
 * "#counter\tcount" and one line per counter (units_seen unit_positions base_no_vote link_no_vote base_no_ref duplex_no_vote
 * duplex_base_no_ref); "#summary\tkind\tbin\tminority_votes\tvotes" and one line per bin and kind (BASE: both reference classes; LINK): the
 * votes off the diagonal and all votes of the bin, two integers and no ratio; then one "#<KIND>\t<columns>" line per kind and one line per cell that is not 0:
 *   BASE <TAB> refclass (REF, ALT) <TAB> bin <TAB> consensus <TAB> vote <TAB> count        LINK <TAB> bin <TAB> consensus <TAB> vote <TAB> count
 *   BASE_POS <TAB> refclass <TAB> bin <TAB> positions <TAB> unanimous                      LINK_POS <TAB> bin <TAB> positions <TAB> unanimous
 *   DUPLEX_BASE <TAB> ref <TAB> strand0 <TAB> strand1 <TAB> count                          DUPLEX_LINK <TAB> strand0 <TAB> strand1 <TAB> count
 * with the symbols A C G T N NN and M D3P D2 D1 I3P I2 I1 NN, and NONE for a strand without a vote.  Integers only; a path that ends in
 * .gz is written block-gzipped (uvcio_bgzf_write_*). */
typedef struct uvcio_famconcord uvcio_famconcord_t;
int uvcio_famconcord_open(uvcio_famconcord_t **out);
int uvcio_famconcord_add(uvcio_famconcord_t *f, const int64_t *row /* [1429] */);
int uvcio_famconcord_write(const uvcio_famconcord_t *f, const char *path);
void uvcio_famconcord_close(uvcio_famconcord_t *f);
/* ---- the UMI family report (uvc1-mi355x --family-stats-out) ----
 * What tiles report with uvcgpu_region_family_stats (rows of 365 int64: the TARGET block of 4 counters, the FIRST block of 8 counters,
 * size[64] and strands[17][17]), kept per target and per run.  Targets are added in report order before the pieces; add_piece adds the
 * TARGET block of a row to its target and the FIRST block to the run's sum, under a lock: pieces come in any order and from any thread.
 * write: two "##" lines; "#summary" and name<TAB>value lines -- families fragments alignments families_both_strands families_umi
 * families_duplex_tag families_amplicon of the FIRST sum, duplication_permille = 1000 (fragments - families) / fragments,
 * mean_family_size_x1000 = 1000 fragments / families, both_strands_permille = 1000 families_both_strands / families (integer division,
 * 0 for an empty denominator); "#family_size\tfamilies" and 64 lines (1 .. 63, 64+); "#strand0_size\tstrand1_size\tfamilies" and the
 * non-empty bins (sizes capped as 16+); "#chrom\tbeg\tend\tname\tfamilies\tfragments\talignments\tfamilies_both_strands\t
 * mean_family_size_x1000\tboth_strands_permille" and one line per target in the order they were added, zeros for a target without
 * pieces.  Integers only; a path that ends in .gz is written block-gzipped (uvcio_bgzf_write_*). */
typedef struct uvcio_famstats uvcio_famstats_t;
int uvcio_famstats_open(uvcio_famstats_t **out);
int64_t uvcio_famstats_add_target(uvcio_famstats_t *f, const char *chrom, int64_t beg, int64_t end, const char *name /* NULL or empty: "." */);   /* -> its index, < 0 on error */
int uvcio_famstats_add_piece(uvcio_famstats_t *f, int64_t target, const int64_t *row /* [365] */);
int uvcio_famstats_write(const uvcio_famstats_t *f, const char *path);
void uvcio_famstats_close(uvcio_famstats_t *f);
/* ---- the fragment length and end-motif profile (uvc1-mi355x --fragment-profile-out) ----
 * What tiles report with uvcgpu_region_fragment_profile: per piece a TARGET row (8 int64: pairs others singles len_sum short long families,
 * a reserved 0) and per call the profile row (2320 int64: 16 counters, LEN[1024], FAMLEN[1024], MOTIF[256]; include/uvc_fragprofile.def).
 * Targets are added in report order before the pieces; add_piece adds a TARGET row to its target and add_profile a profile row to the
 * run's sum, under a lock: both come in any order and from any thread.
 * write: "##fragment_profile=1", "##fragment_profile_min_mapq=", "##fragment_profile_short=A-B", "##fragment_profile_long=A-B" and one more
 * "##" line; "#summary" and name<TAB>value lines -- pairs others singles len_sum short long families families_both_strands ends
 * ends_off_region ends_no_ref of the profile sum; "#length\tfragments\tfamilies" and 1024 lines (0 .. 1022, 1023+: LEN and FAMLEN);
 * "#end_motif\tcount" and 256 lines (AAAA .. TTTT); "#chrom\tbeg\tend\tname\tpairs\tothers\tsingles\tlen_sum\tshort\tlong\tfamilies" and one
 * line per target in the order they were added, zeros for a target without pieces.  Integers only: ratios are the reader's.  A path that
 * ends in .gz is written block-gzipped (uvcio_bgzf_write_*). */
typedef struct uvcio_fragprofile uvcio_fragprofile_t;
int uvcio_fragprofile_open(uvcio_fragprofile_t **out, int32_t min_mapq, int32_t short_lo, int32_t short_hi, int32_t long_lo, int32_t long_hi);
int64_t uvcio_fragprofile_add_target(uvcio_fragprofile_t *f, const char *chrom, int64_t beg, int64_t end, const char *name /* NULL or empty: "." */);   /* -> its index, < 0 on error */
int uvcio_fragprofile_add_piece(uvcio_fragprofile_t *f, int64_t target, const int64_t *row /* [8] */);
int uvcio_fragprofile_add_profile(uvcio_fragprofile_t *f, const int64_t *profile /* [2320] */);
int uvcio_fragprofile_write(const uvcio_fragprofile_t *f, const char *path);
void uvcio_fragprofile_close(uvcio_fragprofile_t *f);
/* ---- the reads and families behind listed sites (uvc1-mi355x --site-reads-out) ----
 * What tiles report with uvcgpu_region_site_reads.  add() takes one call's sites of one contig (zero-based, the `sites` of the call), per
 * site the reference base (`ref`, n_sites chars; NULL: unknown, written as "."), the counts (NULL: zeros -- a listed site that no tile
 * reports on) and the rows, with the columns of the call's alignments that the text needs, indexed by UvcSiteRead::read: qname (entries of
 * alignments without rows may be NULL), flag, mapq, l_qseq, fam_id, fam_strand, frag_id and the bases (one byte per base, 0..3 = ACGT) at
 * seq_off for the inserted sequences.  It copies what it keeps, under a lock: any thread, any order; the rows of a site come from one call.
 * write: "##site_reads_min_mapq=", "##site_reads_alt_only=", the three "#S", "#A", "#R" column lines, then per site in (contig id, pos) order
 *   S contig pos(1-based) ref depth A C G T N DEL INS DEL_after        depth = the six kinds summed; also for a site without observations
 *   A contig pos allele reads fragments families families_both_strands  one per allele with rows: a kind's name, +<inserted bases> or
 *     -<deleted length>; a row with an event counts under its event allele(s) and not under its base; fragments and families are the
 *     distinct (fam_id, fam_strand, frag_id) and fam_id among the allele's rows, families_both_strands those with rows of both fam_strand
 *     values; kinds first in their order, then the insertions by their bases, then the deletions by length
 *   R contig pos obs qual cycle class mapq qname flag family strand ins del   one per row, ordered by (family, qname, flag); cycle =
 *     (flag & 0x10) ? l_qseq - 1 - q : q; class as in the read profile; family = the 1-based rank of the row's family among the families
 *     with rows at this site, ordered by the smallest (qname, flag) of their rows there (ids of a tile do not show); ins = the inserted
 *     bases or "."; del = the deleted length or 0.
 * Integers and names only, tab-separated.  A path that ends in .gz is written block-gzipped. */
typedef struct uvcio_sitereads uvcio_sitereads_t;
int uvcio_sitereads_open(uvcio_sitereads_t **out, const char *const *kind_names /* [6] */, const char *const *class_names /* [4] */, int32_t min_mapq, int32_t alt_only);
int uvcio_sitereads_add(uvcio_sitereads_t *f, int32_t tid, const char *contig, const int32_t *sites, const char *ref, int64_t n_sites, const int32_t *counts /* [n_sites][8] */,
                        const UvcSiteRead *rows, int64_t n_rows, int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *l_qseq,
                        const int32_t *fam_id, const uint8_t *fam_strand, const int32_t *frag_id, const uint8_t *bases, const int64_t *seq_off);
int uvcio_sitereads_write(const uvcio_sitereads_t *f, const char *path);
void uvcio_sitereads_close(uvcio_sitereads_t *f);
/* ---- clipped-read breakpoint sites (uvc1-mi355x --clip-sites-out) ----
 * What tiles report with uvcgpu_region_clip_sites (want_reads = 1).  add() takes one call's site rows of one contig ([n_sites][176], the
 * `sites` of the call) and its event rows, with the columns of the call's alignments that the text needs, indexed by UvcClipRead::read:
 * qname (entries of alignments without rows may be NULL), flag, mapq, fam_id, fam_strand and frag_id.  It copies what it keeps, under a
 * lock: any thread, any order; a site comes from one call (the tile that owns its position).  A site that two calls report -- a position
 * inside two overlapping targets -- is kept once: the report with the lexicographically larger row from `reads` on, the first of equal ones.
 * write: "##clip_sites_min_mapq=", "##clip_sites_min_clip=", "##clip_sites_min_reads=", "##clip_sites_reads=", the "#S" and "#R" column
 * lines, then per site in (contig id, pos, side) order
 *   S contig pos(1-based) side(L|R) reads fwd supp secondary hard len_sum len_max mapq_sum spanning fragments families
 *     families_both_strands cons_len cons      fragments and families are the distinct (fam_id, fam_strand, frag_id) and fam_id among the
 *     site's events, families_both_strands those with events of both fam_strand values (ids are local to a call); cons_len = the vote
 *     indices k with at least one vote; cons = one letter per such k, the base with the most votes (ties to the smaller code, N for code 4),
 *     lower-case iff winner * 3 < total * 2, a LEFT site in reference direction (k descending), a RIGHT site with k ascending; "." when
 *     cons_len is 0
 *   R contig pos side qname flag mapq soft_len hard_len family_rank strand   with reads = 1 one per event behind the site, ordered by
 *     (family_rank, qname, flag): the 1-based rank of the event's family among the families of the site, ordered by the smallest (qname,
 *     flag) of their events there.
 * Junctions (uvcgpu_region_clip_junctions, uvc1-mi355x --clip-sites-junctions 1): set_junctions() turns them on and keeps the five request
 * values; add_junctions() is add() with the call's junction rows ([n_sites][UVC_CLIPJUNC_ROW], one per site row; NULL: add()).  write()
 * then adds "##clip_sites_junction_min_votes=", "_min_len=", "_max_mismatch=", "_max_dist=" and "_slop=" behind "##clip_sites_reads=", the
 * "#J" column line behind "#R", and directly behind the S line of every site that came with a junction row
 *   J contig pos side query_len cmp_len status best_mm n_best second_mm partner_pos(1-based) strand(+|-) class(NONE|DEL|DUP|INV|ADJACENT) len
 *     mate_pos(1-based) mate_side(L|R)      "." where a field has no value; the mate is written as the position and side of its row.
 * Of a site that two calls report, the J line is that of the call whose site row is kept.  Without set_junctions the file is the one above.
 * Mates (uvcgpu_region_clip_mates, uvc1-mi355x --clip-sites-mates 1): set_mates() turns them on and keeps the five request values and the
 * contig names of the BAM header (mate contig ids index them).  add_mates() is add_junctions() with the call's site_rows ([n_sites]
 * [UVC_CLIPMATE_SITE_ROW]; NULL: add_junctions()), kept cluster rows ([n_clusters][UVC_CLIPMATE_ROW]) and witness rows (UvcClipMate, as
 * want_reads = 1 returns them).  write() then adds "##clip_sites_mate_window=", "_overhang=", "_min_dist=", "_max_gap=" and "_min_pairs="
 * behind the lines above, the "#P" and "#M" column lines behind "#R" (and "#J"), and behind the S line of every site that came with a
 * site row, and behind its J line if there is one,
 *   P contig pos side facing concordant other_contig same_strand far clusters clusters_kept
 *   M contig pos side mate_contig mate_beg mate_end mate_strand(+|-) pairs other_contig same_strand far mapq_sum fragments families
 *     families_both_strands      one per kept cluster of the site, in witness order.  mate_beg / mate_end are 1-based, mpos_min + 1 and
 *     mpos_max + 1: the leftmost coordinates of the mates, not their ends; mate_contig is "." for an id the names do not hold.  fragments,
 *     families and families_both_strands are counted over the cluster's witnesses as the S line counts them over its events.
 * Of a site that two calls report, the P and M lines are those of the call whose site row is kept.  Witnesses are the reads of the call,
 * so the P and M lines of a site closer than the window to a border of its call may depend on how the run is cut into calls.  Without
 * set_mates the file is the one above.
 * Integers and names only, tab-separated.  A path that ends in .gz is written block-gzipped. */
typedef struct uvcio_clipsites uvcio_clipsites_t;
int uvcio_clipsites_open(uvcio_clipsites_t **out, int32_t min_mapq, int32_t min_clip, int32_t min_reads, int32_t with_reads);
int uvcio_clipsites_add(uvcio_clipsites_t *f, int32_t tid, const char *contig, const int64_t *sites /* [n_sites][UVC_CLIPSITE_ROW] */, int64_t n_sites, const UvcClipRead *reads, int64_t n_reads,
                        int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *fam_id, const uint8_t *fam_strand, const int32_t *frag_id);
int uvcio_clipsites_set_junctions(uvcio_clipsites_t *f, int32_t min_votes, int32_t min_len, int32_t max_mismatch, int32_t max_dist, int32_t mate_slop);
int uvcio_clipsites_add_junctions(uvcio_clipsites_t *f, int32_t tid, const char *contig, const int64_t *sites /* [n_sites][UVC_CLIPSITE_ROW] */, const int64_t *junctions /* [n_sites][UVC_CLIPJUNC_ROW] or NULL */,
                                  int64_t n_sites, const UvcClipRead *reads, int64_t n_reads, int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *fam_id,
                                  const uint8_t *fam_strand, const int32_t *frag_id);
int uvcio_clipsites_set_mates(uvcio_clipsites_t *f, int32_t window, int32_t overhang, int32_t min_dist, int32_t max_gap, int32_t min_pairs, const char *const *contig_names, int32_t n_contigs);
int uvcio_clipsites_add_mates(uvcio_clipsites_t *f, int32_t tid, const char *contig, const int64_t *sites /* [n_sites][UVC_CLIPSITE_ROW] */, const int64_t *junctions /* [n_sites][UVC_CLIPJUNC_ROW] or NULL */,
                              int64_t n_sites, const UvcClipRead *reads, int64_t n_reads, int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *fam_id,
                              const uint8_t *fam_strand, const int32_t *frag_id, const int64_t *site_rows /* [n_sites][UVC_CLIPMATE_SITE_ROW] or NULL */,
                              const int64_t *clusters /* [n_clusters][UVC_CLIPMATE_ROW] */, int64_t n_clusters, const UvcClipMate *mates, int64_t n_mates);
int uvcio_clipsites_write(const uvcio_clipsites_t *f, const char *path);
void uvcio_clipsites_close(uvcio_clipsites_t *f);
/* ---- the read profile (uvc1-mi355x --read-profile-out) ----
 * The sum of the rows that tiles report with uvcgpu_region_read_profile (5712 int64: Q[4][64][2], CYC[4][256][5], SUB[4][4][4], 16 counters);
 * rows of disjoint position sets add, so add() sums under a lock, from any thread in any order.  write(): "##read_profile_min_mapq=",
 * "##read_profile_min_depth=", "##read_profile_max_alt_permille=" and "##empirical_quality=-10*log10((mismatch+1)/(match+mismatch+2))" (the
 * quality a bin's counts stand for; left to the reader, the file holds integers only); "#counter\tcount" and the ten counters;
 * "#class\tquality\tmatch\tmismatch" and one line per (class, quality bin) that is not empty; "#class\tcycle\tmatch\tmismatch\tins\tdel\tclip"
 * likewise per (class, cycle bin); "#class\tref\tread\tcount" per non-zero substitution bin.  Class, quality and cycle ascend.  A path that
 * ends in .gz is written block-gzipped (uvcio_bgzf_write_*). */
typedef struct uvcio_readprofile uvcio_readprofile_t;
int uvcio_readprofile_open(uvcio_readprofile_t **out, const char *const *class_names /* [4] */, int32_t min_mapq, int32_t min_depth, int32_t max_alt_permille);
int uvcio_readprofile_add(uvcio_readprofile_t *p, const int64_t *row /* [5712] */);
int uvcio_readprofile_write(const uvcio_readprofile_t *p, const char *path);
void uvcio_readprofile_close(uvcio_readprofile_t *p);
/* ---- the callable-region BED (uvc1-mi355x --callable-out) ----
 * The targets in report order and, per target, the runs that tiles report for its pieces with uvcgpu_region_callable.  add_runs takes the
 * runs of one call as they came back and the target of each of the call's ranges, under a lock: pieces come in any order and from any
 * thread; a run outside its target is refused.  write, in target order: sorts a target's runs by position, FILLS every position of the
 * target that no piece reported with the mask of depth 0 (NO_COVERAGE and every tested LOW_* bit -- the rule by which the coverage report
 * counts such positions as depth 0) and JOINS neighbouring runs of equal mask inside the target, never across targets: the text does not
 * depend on how tiles cut a target.  Overlapping pieces fail the write.
 * Text: "##callable_regions=1", "#min_depth<TAB>aDP=N,...", "#max_aDP<TAB>N", "#chrom beg end class target"; one BED line per run, class =
 * CALLABLE or the names of the set bits joined by commas in bit order, target = the name given or "."; then "#summary<TAB>positions<TAB>N",
 * "#summary<TAB>CALLABLE<TAB>N" and one "#summary<TAB>bit<TAB>N" per bit.  Tab-separated integers; a path that ends in .gz is written
 * block-gzipped (uvcio_bgzf_write_*).  The store holds 16 bytes per run until close. */
typedef struct uvcio_callable uvcio_callable_t;
int uvcio_callable_open(uvcio_callable_t **out, const char *const *measure_names, int32_t n_measures, const int32_t *min_depth /* [n_measures] */, int32_t max_aDP,
                        const char *const *bit_names, int32_t n_bits /* n_measures + 2: LOW_* per measure, EXCESS_aDP, NO_COVERAGE */);
/* [beg, end): the positions of the target inside its contig (end <= beg: a target without positions, no line).  Returns the target's index, or a negative code. */
int64_t uvcio_callable_add_target(uvcio_callable_t *c, const char *chrom, int64_t beg, int64_t end, const char *name /* NULL or empty: "." */);
int uvcio_callable_add_runs(uvcio_callable_t *c, const int64_t *target_of_range, int64_t n_ranges, const UvcCallableRun *runs, int64_t n_runs);
int64_t uvcio_callable_n_runs(const uvcio_callable_t *c);   /* the runs held so far */
int uvcio_callable_write(const uvcio_callable_t *c, const char *path);
void uvcio_callable_close(uvcio_callable_t *c);
/* ---- the microsatellite tally (uvc1-mi355x --msi-out) ----
 * The targets in report order and the loci that tiles report with uvcgpu_region_msi (rows of UVC_MSI_ROW int32, include/uvc_msi.def).  add
 * takes the rows of one call as they came back, the target of each of the call's ranges and, per locus, the reference bases of its first
 * unit as text, under a lock: tiles come in any order and from any thread; a locus that begins outside its target is refused.  write, in
 * target order then position: one line per locus -- chrom, beg, end = beg + tracklen, unit, unitlen, units = tracklen / unitlen, target,
 * flags ("." or "EDGE"), then per level b, c, c2, d (beside bDP, cDP12, cDP2, dDP1): depth, shifted = the sum of the twelve shift bins,
 * other, and the bins m6..m1 p1..p6 -- and "#summary<TAB>loci<TAB>N", "#summary<TAB>loci_EDGE<TAB>N" and per level "#summary<TAB>level<TAB>
 * assessable<TAB>N<TAB>unstable<TAB>M": N = the loci without EDGE whose depth is >= min_depth, M = those of them with 1000 * shifted >=
 * unstable_permille * depth.  The header says what the file is: a tally for a classifier with a baseline, not an MSI call.  Tab-separated;
 * a path that ends in .gz is written block-gzipped.  The store holds a row and a unit per locus until close. */
typedef struct uvcio_msi uvcio_msi_t;
int uvcio_msi_open(uvcio_msi_t **out, int32_t min_tracklen, int32_t min_units, int32_t max_unitlen, int32_t min_depth, int32_t unstable_permille);
int64_t uvcio_msi_add_target(uvcio_msi_t *m, const char *chrom, int64_t beg, int64_t end, const char *name /* NULL or empty: "." */);   /* the target's index, or a negative code */
int uvcio_msi_add(uvcio_msi_t *m, const int64_t *target_of_range, int64_t n_ranges, const int32_t *loci /* [n_loci][UVC_MSI_ROW] */, const char *const *units /* [n_loci] */, int64_t n_loci);
int64_t uvcio_msi_n_loci(const uvcio_msi_t *m);   /* the loci held so far */
int uvcio_msi_write(const uvcio_msi_t *m, const char *path);
void uvcio_msi_close(uvcio_msi_t *m);
/* bcftools concat -n (uvcTN.sh:100): the BGZF files one after the other, the 28-byte end-of-file marker of all but the last dropped. */
int uvcio_bgzf_concat(const char *out_path, const char *const *in_paths, int32_t n_in);
/* The whole text of a (block-)gzipped or plain file (the tumor VCF of a T/N pair); *buf is malloc'ed, the caller frees it. */
int uvcio_read_text_file(const char *path, char **buf, int64_t *len);

#ifdef __cplusplus
}
#endif
#endif
