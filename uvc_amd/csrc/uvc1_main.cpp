// uvc1-mi355x -- BAM + FASTA -> block-gzipped VCF: the host chain of the reference's uvc1 (main.cpp:1196-1603, process_batch :458-1193)
// in C++ on the three C ABIs of this repository (uvcio.h readers / writer, uvcgroup.h family assignment, uvcgpu.h hot path + record text).
// Every option of the reference's command line (CmdLineArgs.cpp:188-1000) is accepted under its name, as `--opt value` or `--opt=value`:
// the hot-path parameters by the library's name table (uvcgpu_param_set), the rest by the class table OPTS below (--help lists all).
//
// Region shards.  The reference fans its regions out over threads with `schedule(dynamic, 1)` and writes the chunk outputs in
// order (main.cpp:1478-1551); uvcTN.sh:92-101 adds one process per chromosome and `bcftools concat -n`.  Here:
//   * one process, several GPUs: --devices 0,1,.. (default: all visible).  Worker thread w binds to devices[w % n]; the workers pull tiles
//     from one queue (dynamic balance: a tile costs what its reads cost), each owns its file handles and one region handle that is reset
//     from tile to tile; the lines are written in tile order and a worker never runs more than 4 * threads tiles ahead of the writer.
//   * several processes: --shard i/n takes the i-th of n contiguous runs of the tile list, balanced by the compressed bytes the BAM index
//     attributes to each tile plus its length (reads and positions, main.cpp:1390-1392); shard 0 writes the header; `--concat out in..`
//     joins the shard outputs like bcftools concat -n.  No GPU ever talks to another one: there is no collective on this path.
// Regions are fixed tiles (--tile); every zerobased_pos has exactly one owner (UvcScoreRequest::base_at_pos_beg), so the tiles of one
// covered stretch write the records of one uncut region.
#include "uvcgpu.h"
#include "uvcgroup.h"
#include "uvcio.h"
#include "uvc_cpus.h"

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {
const int32_t MAX_INSERT_SIZE = 2000, MAX_STR_N_BASES = 100;   // common.hpp:63-64

// The reports beside the VCF (DESIGN.md 4i, 4j, 4k, 4l, 4n, 4m, 4o, 4p, 4q with 4r, 4t), in the order their options are checked: of several faults the first in
// this order is the one reported.
// A row holds what the command line says of a report in more than one place: parse (the path, "a sub-option was given", the checks behind
// the loop), split_pair (pair mode writes none) and main (the probe of the path).  A new report is a row here, an Opts store, a
// *_of_tile and its open / write lines in main.
enum ReportId { R_COVERAGE, R_ERRPROF, R_FAMSTATS, R_CALLABLE, R_MSI, R_READPROF, R_FRAGPROF, R_SITEREADS, R_CLIPSITES, R_FAMCONC, N_REPORTS };
struct ReportRow {
    const char *out;                 // --X-out PATH
    const char *subs[18];            // the options that only shape this report: each needs --X-out (the list ends with a null)
    const char *window;              // the one of them that cuts the targets into windows (refuse_report_windows), or none
    const char *why_no_shard, *why_no_repeat;   // refuse_report_runs
    const char *pair_writes_no;      // split_pair: "pair mode ... writes no <this>"
    const char *needs;               // the sentence for sub-options without --X-out; none: one per sub-option, "<sub> needs <out>: it only shapes that report"
};
const ReportRow REPORTS[N_REPORTS] = {
    { "--coverage-out", { "--coverage-thresholds", "--coverage-window" }, "--coverage-window", "a target can straddle shards", "every tile would be counted that many times", "coverage report", nullptr },
    { "--error-profile-out", { "--error-profile-min-depth", "--error-profile-max-alt-permille" }, nullptr, "every shard would write a part of the table", "every tile would be counted that many times", "error profile",
      "--error-profile-min-depth and --error-profile-max-alt-permille need --error-profile-out: they only gate that report" },
    { "--family-stats-out", { "--family-stats-window" }, "--family-stats-window", "a target can straddle shards", "every tile would be counted that many times", "family report", nullptr },
    { "--callable-out", { "--callable-min-depth", "--callable-max-aDP" }, nullptr, "a target can straddle shards", "every tile would report its runs that many times", "callable regions",
      "--callable-min-depth and --callable-max-aDP need --callable-out: they only set the criteria of that file" },
    { "--msi-out", { "--msi-min-tract", "--msi-min-units", "--msi-max-unit", "--msi-min-depth", "--msi-unstable-permille" }, nullptr, "a target can straddle shards", "every tile would report its loci that many times", "microsatellite tally",
      "--msi-min-tract, --msi-min-units, --msi-max-unit, --msi-min-depth and --msi-unstable-permille need --msi-out: they only shape that file" },
    { "--read-profile-out", { "--read-profile-min-mapq", "--read-profile-min-depth", "--read-profile-max-alt-permille" }, nullptr, "every shard would write a part of the profile", "every tile would be counted that many times", "read profile",
      "--read-profile-min-mapq, --read-profile-min-depth and --read-profile-max-alt-permille need --read-profile-out: they only gate that report" },
    { "--fragment-profile-out", { "--fragment-profile-window", "--fragment-profile-min-mapq", "--fragment-profile-short", "--fragment-profile-long" }, "--fragment-profile-window", "a target can straddle shards",
      "every tile would be counted that many times", "fragment profile", nullptr },
    { "--site-reads-out", { "--site-reads-sites", "--site-reads-min-mapq", "--site-reads-alt-only" }, nullptr, "every shard would write the sites of its tiles", "every tile would report its rows that many times", "site reads report", nullptr },
    { "--clip-sites-out", { "--clip-sites-min-clip", "--clip-sites-min-reads", "--clip-sites-min-mapq", "--clip-sites-reads", "--clip-sites-junctions", "--clip-sites-junction-min-len", "--clip-sites-junction-max-mismatch",
                            "--clip-sites-junction-min-votes", "--clip-sites-junction-max-dist", "--clip-sites-junction-slop", "--clip-sites-mates", "--clip-sites-mate-window", "--clip-sites-mate-overhang",
                            "--clip-sites-mate-min-dist", "--clip-sites-mate-max-gap", "--clip-sites-mate-min-pairs" }, nullptr, "every shard would write the sites of its tiles", "every tile would report its sites that many times",
      "clip sites report", nullptr },
    { "--family-concordance-out", { nullptr }, nullptr, "every shard would write a part of the row", "every tile would be counted that many times", "family concordance report", nullptr },
};
// the row that `name` is an option of, or -1; *sub: which of the row's sub-options, -1 for --X-out itself
int report_of(const std::string &name, int *sub) {
    for (int r = 0; r < N_REPORTS; r++) {
        *sub = -1;
        if (name == REPORTS[r].out) return r;
        for (int s = 0; REPORTS[r].subs[s]; s++) if (name == REPORTS[r].subs[s]) { *sub = s; return r; }
    }
    return -1;
}

struct Opts {
    std::string bam, fasta, out, sample = "-", targets, bed, tumor_vcf, bed_out, bed_in, umi_struct, force_sites;
    std::vector<int> devices;
    int threads = 0, repeat = 1, shard = 0, n_shards = 1, tumor_format = 1;
    int sequencing_platform = UVC_PLATFORM_AUTO, assay_type = 0;   // --sequencing-platform (0 AUTO, 1 ILLUMINA, 2 IONTORRENT, 3 OTHER), --assay-type (0 inferred per tile, 1 CAPTURE, 2 AMPLICON)
    int64_t tile = 0;            // 0 = no fixed tiles: the regions are the reference's own cuts (uvcio_plan_regions = SamIter::iternext); --tile N overrides
    int64_t mem_per_thread = 1536;   // --mem-per-thread (MB), CmdLineArgs.hpp:33: enters the reference's region cuts
    int64_t merge = 0;           // --merge-regions N: BED lines at most N bp apart become ranges of one device region (0 = one region per line)
    int64_t score_mem_mb = 0;    // --score-mem-mb N: score every tile as a stream of chunks whose row sets and record buffers fit N MiB per worker (0 = one call per tile)
    // the reports beside the VCF, one row of REPORTS each: --X-out PATH (empty = none), which of its sub-options were given (bit s: the
    // row's s-th), and --X-window N where the row has one: the targets are windows of N bp (0: the BED lines)
    struct Report { std::string path; uint32_t subs_given = 0; int64_t window = 0; } report[N_REPORTS];
    std::vector<int32_t> coverage_thr{ 1, 20, 100, 500 };   // --coverage-thresholds
    uvcio_coverage_t *cov = nullptr;   // --coverage-out: the report's store, filled by the workers (main)
    UvcErrorProfileRequest errprof_req{ 20, 50 };   // --error-profile-min-depth, --error-profile-max-alt-permille
    uvcio_errprofile_t *errprof = nullptr;   // --error-profile-out: the run's table, summed over the tiles by the workers (main)
    uvcio_famstats_t *fam = nullptr;   // --family-stats-out: the report's store, filled by the workers (main)
    uvcio_famconcord_t *famconc = nullptr;   // --family-concordance-out: the run's row, summed over the tiles by the workers (main)
    UvcCallableRequest call_req = [] { UvcCallableRequest q{}; q.min_depth[UVC_COV_cDP12] = 20; return q; }();   // --callable-min-depth, --callable-max-aDP
    uvcio_callable_t *callable = nullptr;   // --callable-out: the BED's store, filled by the workers (main)
    std::vector<int64_t> call_contig_target;   // without a BED file: per contig the store's target of its called span (-1: not called)
    std::vector<std::pair<int64_t, int64_t>> call_target_span;   // per target of the store its [beg, end): a tile's stretch is clipped to it
    UvcMsiRequest msi_req{ 10, 5, 6 }; int32_t msi_min_depth = 30, msi_unstable_permille = 200;   // --msi-min-tract, --msi-min-units, --msi-max-unit; --msi-min-depth, --msi-unstable-permille
    uvcio_msi_t *msi = nullptr;   // --msi-out: the tally's store, filled by the workers (main); its targets are those of --callable-out (call_contig_target, call_target_span)
    UvcReadProfileRequest readprof_req{ 0, 20, 50 };   // --read-profile-min-mapq, --read-profile-min-depth, --read-profile-max-alt-permille
    uvcio_readprofile_t *readprof = nullptr;   // --read-profile-out: the run's row, summed over the tiles by the workers (main)
    UvcFragmentProfileRequest fragprof_req{ 0, 100, 150, 151, 220 };   // --fragment-profile-min-mapq, --fragment-profile-short A-B, --fragment-profile-long A-B
    uvcio_fragprofile_t *fragprof = nullptr;   // --fragment-profile-out: the report's store, filled by the workers (main)
    std::string sitereads_sites; UvcSiteReadsRequest sitereads_req{ 0, 1 };   // --site-reads-sites, --site-reads-min-mapq, --site-reads-alt-only
    uvcio_sitereads_t *sitereads = nullptr; uvcio_sites_t *sitereads_list = nullptr;   // --site-reads-out: the report's store, filled by the workers, and the listed sites (main)
    UvcClipSitesRequest clipsites_req{ 0, 10, 3, 1 }; int32_t clipsites_reads = 0;   // --clip-sites-min-mapq, --clip-sites-min-clip, --clip-sites-min-reads (the call always asks for the event rows); --clip-sites-reads
    uvcio_clipsites_t *clipsites = nullptr;   // --clip-sites-out: the report's store, filled by the workers (main)
    int32_t clipsites_mates = 0; UvcClipMatesRequest clipmates_req{ 0, 0, 500, 5, 1000, 500, 2, 1 };   // --clip-sites-mates; --clip-sites-mate-window, -overhang, -min-dist, -max-gap, -min-pairs (tid per tile, min_mapq = --clip-sites-min-mapq, always with the witness rows)
    int32_t clipsites_junctions = 0; UvcClipJunctionsRequest clipjunc_req{ 2, 16, 1, 0, 10 };   // --clip-sites-junctions; --clip-sites-junction-min-votes, -min-len, -max-mismatch, -max-dist, -slop
    bool timing = false, no_header = false, device_inflate = false, print_params = false;
    UvcParams P;                 // the reference's defaults and the user's values; the platform step comes on top (main)
    UvcGroupParams G;
    const uvcio_sites_t *sites = nullptr;   // --force-sites, read once the BAM header is known (main)
};
[[noreturn]] void die(const std::string &m) { fprintf(stderr, "uvc1-mi355x: %s\n", m.c_str()); exit(2); }
const char *const ONLY_PRINT_VCF_HEADER = "/only-print-vcf-header/";   // OPT_ONLY_PRINT_VCF_HEADER, common.hpp:58

// Every option of the reference's command line (CmdLineArgs.cpp:188-1000) falls into one class:
//   PARAM / GROUP  a row of include/uvc_params.def / uvc_group_params.def, named in option form (--fam-thres-highBQ-snv): set through
//                  uvcgpu_param_set.  These rows come from the library's name table (uvcgpu_param_info), so a new .def row is an option
//                  with no edit here; the derived rows (inferred_*, tumor_vcf_*) are not options.
//   CLI            files, regions, threads and this program's own switches
//   MODE           switches that are not a plain row, or whose row needs wiring: see main / call_tile
//   INERT          the reference parses it and its value changes nothing the reference writes (logging, a stderr warning, no live
//                  reader): accepted, no effect
//   UNSUPPORTED    what this program does not produce: refused (exit 2) off its default, accepted at it
// The table below holds every option that is not a PARAM / GROUP row; a name here wins over a .def row of the same name.
enum OptClass { O_CLI, O_MODE, O_INERT, O_UNSUPPORTED, O_PARAM, O_GROUP };
const char *const CLASS_NAME[] = { "CLI", "MODE", "INERT", "UNSUPPORTED", "PARAM", "GROUP" };
struct OptRow { const char *names; OptClass cls; bool flag; const char *dflt; const char *what; };
const OptRow OPTS[] = {
    { "-f,--fasta", O_CLI, false, "", "reference FASTA (with .fai)" },
    { "-o,--output", O_CLI, false, "", "block-gzipped VCF to write" },
    { "-s,--sample", O_CLI, false, "-", "sample name" },
    { "--targets", O_CLI, false, "", "chr or chr:beg-end (1-based, inclusive)" },
    { "-R,--regions-file", O_CLI, false, "", "BED file of the regions to call" },
    { "-t,--threads", O_CLI, false, "0", "tiles in flight (0: half the usable cores, 1..8 per device)" },
    { "-A,--all-out", O_CLI, true, "", "every allele of every position (should_output_all = 1)" },
    { "--force-sites", O_CLI, false, "", "BED or VCF(.gz) of sites: at each listed POS every allele record as -A writes it, the default gate elsewhere" },
    { "-q,--vqual", O_CLI, false, "15", "minimum variant quality (the vqual row)" },
    { "--outvar-flag", O_CLI, false, "62", "output-variant bits (the outvar_flag row)" },
    { "--tumor-vcf", O_CLI, false, "", "the tumor pass's VCF: this BAM is the normal sample of a T/N pair" },
    { "--tn-is-paired", O_CLI, false, "0", "the tn_is_paired row" },
    { "--is-tumor-format-retrieved", O_CLI, false, "1", "carry the tumor's FORMAT column into the normal pass's records" },
    { "--bed-in-fname", O_CLI, false, "", "BED file of regions (overrides -R)" },
    { "--bed-out-fname", O_CLI, false, "", "write the region table here" },
    { "--mem-per-thread", O_CLI, false, "1536", "MB per thread in the reference's region cuts" },
    { "--tile", O_CLI, false, "0", "fixed tiles of this many bp instead of the reference's region cuts" },
    { "--merge-regions", O_CLI, false, "0", "with -R / --bed-in-fname: BED lines at most this many bp apart are called as ranges of one region of at most --tile bp (0: one region per line); a merged region starts its repeat track and BAQ sums at the batch's begin and sees the reads of the gaps, as a --tile region does" },
    { "--devices,--device", O_CLI, false, "", "comma-separated HIP device ids (default: all visible)" },
    { "--shard", O_CLI, false, "0/1", "i/n: this process takes the i-th of n runs of tiles" },
    { "--no-header", O_CLI, true, "", "no VCF header" },
    { "--score-mem-mb", O_CLI, false, "0", "score every tile in chunks whose device rows and page-locked record buffers take at most this many MiB per worker (-t), chunk k + 1 computed and copied while chunk k is written; 0: one score call per tile, sized by all its records (14 per position under -A).  The output does not depend on it" },
    { "--coverage-out", O_CLI, false, "", "write the per-target coverage report here (tab-separated; block-gzipped when the name ends in .gz): per BED line, or per --coverage-window, sum / min / max and positions at or above each threshold of six depths the caller itself works with (aDP raw segments, bDP fragments, cDP1 families, cDP12 BQ-filtered families, cDP2 single-strand-consensus families, dDP1 duplex families), reduced on the device from the planes of each tile.  The VCF does not depend on it" },
    { "--coverage-thresholds", O_CLI, false, "1,20,100,500", "with --coverage-out: at most 8 ascending depths; the report counts the positions at or above each" },
    { "--coverage-window", O_CLI, false, "0", "with --coverage-out and no BED file: the targets are windows of this many bp, aligned to multiples of it on each contig and clipped to the called span" },
    { "--error-profile-out", O_CLI, false, "", "write the background error profile here (tab-separated; block-gzipped when the name ends in .gz): how often each base and each InDel symbol is seen at positions that do not look variant, per reference trinucleotide and per evidence level (bDP fragments, cDP1 families, cDP12 BQ-filtered families, cDP2 single-strand-consensus families, dDP1 duplex families), reduced on the device from the planes of each tile over the positions the tile owns.  The VCF does not depend on it" },
    { "--error-profile-min-depth", O_CLI, false, "20", "with --error-profile-out: a position enters a level's bins only where the level's depth is at least this (1 or more)" },
    { "--error-profile-max-alt-permille", O_CLI, false, "50", "with --error-profile-out: a position whose largest non-reference count is above this many thousandths of the level's depth counts as variant and stays out of the bins (0..1000)" },
    { "--family-stats-out", O_CLI, false, "", "write the UMI family report here (tab-separated; block-gzipped when the name ends in .gz): over all targets the number of read families, fragments and alignments, the families seen on both strands, with a UMI, a duplex tag or the amplicon flag, the duplication rate, the family-size histogram (1 .. 64+) and the strand0 x strand1 size histogram (0 .. 16+), then per BED line, or per --family-stats-window, the families that overlap it -- the families exactly as this caller groups and consumes them, reduced on the device from each tile's family units.  The VCF does not depend on it" },
    { "--family-concordance-out", O_CLI, false, "", "write the family concordance report here (tab-separated; block-gzipped when the name ends in .gz): what the consensus of every read family out-voted -- the votes of a family's fragments by consensus symbol, voted symbol and family depth (1, 2, 3, 4, 5-7, 8-15, 16-31, 32+), apart for positions whose consensus is the reference base and the others -- and where the two strands of a duplex family cast different votes, by reference base: the substitution spectrum of the errors the families corrected and the signature of single-strand damage.  The votes are evaluated again on the device behind each tile's accumulate, over the positions the tile owns.  The VCF does not depend on it" },
    { "--family-stats-window", O_CLI, false, "0", "with --family-stats-out and no BED file: the targets are windows of this many bp, aligned to multiples of it on each contig and clipped to the called span" },
    { "--callable-out", O_CLI, false, "", "write the callable regions here as BED lines contig, beg, end, class, target (tab-separated; block-gzipped when the name ends in .gz): every target -- BED line, or called contig span without a BED file -- cut into stretches of equal class, CALLABLE or the criteria the stretch fails (LOW_<depth>, EXCESS_aDP, NO_COVERAGE), classified on the device from the planes of each tile over the six depths of --coverage-out; #summary lines count the positions per class.  The VCF does not depend on it" },
    { "--callable-min-depth", O_CLI, false, "cDP12=20", "with --callable-out: NAME=N[,NAME=N...], the smallest depth a callable position has of each named depth (aDP bDP cDP1 cDP12 cDP2 dDP1; 0 or unnamed: not tested)" },
    { "--callable-max-aDP", O_CLI, false, "0", "with --callable-out: the largest raw depth aDP a callable position has (0: not tested)" },
    { "--msi-out", O_CLI, false, "", "write the microsatellite length-shift tally here (tab-separated; block-gzipped when the name ends in .gz): one line per microsatellite of the caller's own repeat tracks whose first base lies in a target -- BED line, or called contig span without a BED file -- with, per evidence level (b fragments, c UMI families, c2 consensus families, d duplex families), the smallest depth along the tract and the InDel alleles that shift its length by -6..+6 whole units or otherwise, tallied on the device from the planes and allele rows of each tile; #summary lines count the assessable and the unstable loci per level.  A tally for a classifier with a baseline, not an MSI call.  The VCF does not depend on it" },
    { "--msi-min-tract", O_CLI, false, "10", "with --msi-out: the shortest tract in bp" },
    { "--msi-min-units", O_CLI, false, "5", "with --msi-out: the fewest whole repeat units of a tract" },
    { "--msi-max-unit", O_CLI, false, "6", "with --msi-out: the longest repeat unit in bp" },
    { "--msi-min-depth", O_CLI, false, "30", "with --msi-out: the smallest depth along the tract at which the #summary lines count a locus as assessable at a level" },
    { "--msi-unstable-permille", O_CLI, false, "200", "with --msi-out: an assessable locus counts as unstable in the #summary lines when its shifted alleles are at least this many thousandths of its depth" },
    { "--read-profile-out", O_CLI, false, "", "write the read profile here (tab-separated; block-gzipped when the name ends in .gz): per read class (R1 / R2, forward / reverse) the matches and mismatches by reported base quality, the matches, mismatches, inserted bases, deletions and soft-clipped bases by sequencing cycle and the substitution matrix, at positions that do not look variant, reduced on the device from the read bases of each tile over the positions the tile owns, with the BAM's own qualities.  The VCF does not depend on it" },
    { "--read-profile-min-mapq", O_CLI, false, "0", "with --read-profile-out: only alignments of at least this mapping quality are counted (0..255)" },
    { "--read-profile-min-depth", O_CLI, false, "20", "with --read-profile-out: a base enters the bins only where at least this many counted A/C/G/T bases cover the position (1 or more)" },
    { "--read-profile-max-alt-permille", O_CLI, false, "50", "with --read-profile-out: a position whose mismatching bases are above this many thousandths of its depth counts as variant and stays out of the bins (0..1000)" },
    { "--fragment-profile-out", O_CLI, false, "", "write the fragment length and end-motif profile here (tab-separated; block-gzipped when the name ends in .gz): of the fragments and read families the caller formed, over all targets the FR pairs, other two-orientation and one-orientation fragments, the template lengths of the pairs and of the families in 1024 one-bp bins, the short and long pairs and the 256 four-base reference motifs at the 5' ends of the pairs, each counted once, and per target -- BED line, or --fragment-profile-window -- the same counters; integers only" },
    { "--fragment-profile-window", O_CLI, false, "0", "with --fragment-profile-out and no BED file: the targets are windows of this many bp, aligned to multiples of it on each contig and clipped to the called span" },
    { "--fragment-profile-min-mapq", O_CLI, false, "0", "with --fragment-profile-out: only alignments of at least this mapping quality are counted (0..255)" },
    { "--fragment-profile-short", O_CLI, false, "100-150", "with --fragment-profile-out: A-B, the template lengths in bp (both inclusive) of a short pair" },
    { "--fragment-profile-long", O_CLI, false, "151-220", "with --fragment-profile-out: A-B, the template lengths in bp (both inclusive) of a long pair" },
    { "--site-reads-out", O_CLI, false, "", "write the reads and families behind listed sites here (tab-separated; block-gzipped when the name ends in .gz): per site of --site-reads-sites an S line with the depth and the reads showing A C G T N, a deletion, an insertion or a deletion behind the site; per allele an A line with its reads, fragments, UMI families and families seen on both strands; per read an R line with base, corrected quality, cycle, read class, mapping quality, name, flag, family rank and strand -- found on the device among each tile's read bases, with the fragments and families the caller itself formed.  The VCF does not depend on it" },
    { "--site-reads-sites", O_CLI, false, "", "with --site-reads-out (required): BED or VCF(.gz) of the sites, read as --force-sites reads its file" },
    { "--site-reads-min-mapq", O_CLI, false, "0", "with --site-reads-out: only alignments of at least this mapping quality are counted (0..255)" },
    { "--site-reads-alt-only", O_CLI, false, "1", "with --site-reads-out: 1 (or true) writes R and A lines only for reads that differ from the reference at the site -- another base, a deletion, an InDel behind the site; 0 (or false) for every read.  The S lines count every read either way" },
    { "--clip-sites-out", O_CLI, false, "", "write the clipped-read breakpoint sites here (tab-separated; block-gzipped when the name ends in .gz): per (position, side) at which the soft or hard clips of enough alignments end an S line with the reads, their strands, supplementary, secondary and hard-clipped ones, the clip lengths, the reads that span the junction aligned, the fragments, UMI families and families seen on both strands behind the clips, and the consensus of the clipped bases counted outward from the junction -- found on the device among each tile's reads over the positions the tile owns, with the fragments and families the caller itself formed.  The VCF does not depend on it" },
    { "--clip-sites-min-clip", O_CLI, false, "10", "with --clip-sites-out: a clip counts from this many clipped bases on, soft and hard together (1 or more)" },
    { "--clip-sites-min-reads", O_CLI, false, "3", "with --clip-sites-out: a site is written when the clips of at least this many alignments end there (1 or more)" },
    { "--clip-sites-min-mapq", O_CLI, false, "0", "with --clip-sites-out: only alignments of at least this mapping quality are counted (0..255)" },
    { "--clip-sites-reads", O_CLI, false, "0", "with --clip-sites-out: 1 (or true) writes an R line per clipped read behind each S line -- name, flag, mapping quality, soft and hard clip length, family rank and strand; 0 (or false) the S lines alone" },
    { "--clip-sites-junctions", O_CLI, false, "0", "with --clip-sites-out: 1 (or true) searches the consensus of every site's clipped bases in the reference of the site's region, on both strands, and writes a J line behind the S line: where it lies (partner_pos, strand, mismatches, how many equally good places), what that makes of the site (DEL, DUP, INV, ADJACENT), the length and the site that is the other end of the event.  A partner is found only inside the region the site was searched in (the tile with its halo, or the merged BED batch), so J lines depend on how the run is cut; S and R lines do not" },
    { "--clip-sites-junction-min-len", O_CLI, false, "16", "with --clip-sites-junctions 1: a site is searched when at least this many of its 32 consensus bases are compared (1..32)" },
    { "--clip-sites-junction-max-mismatch", O_CLI, false, "1", "with --clip-sites-junctions 1: a place counts with at most this many mismatches among the compared bases (0..7)" },
    { "--clip-sites-junction-min-votes", O_CLI, false, "2", "with --clip-sites-junctions 1: a consensus base is compared when at least this many reads vote there and two thirds of them agree on A, C, G or T (1 or more)" },
    { "--clip-sites-junction-max-dist", O_CLI, false, "0", "with --clip-sites-junctions 1: only places whose partner junction lies at most this far from the site count; 0 is the whole region" },
    { "--clip-sites-junction-slop", O_CLI, false, "10", "with --clip-sites-junctions 1: the mate of a site is the nearest site of the expected side at most this far from the partner junction (microhomology moves the two ends apart)" },
    { "--clip-sites-mates", O_CLI, false, "0", "with --clip-sites-out: 1 (or true) gathers the read pairs that face each site and clusters the mates of the discordant ones -- a P line per site (facing, concordant, other contig, same strand, far, clusters) and an M line per kept cluster (mate contig, span, strand, pairs, families): the partner of a fusion or translocation, on another contig or beyond the tile. A site closer than the window to a tile border sees the reads of its tile alone" },
    { "--clip-sites-mate-window", O_CLI, false, "500", "with --clip-sites-mates 1: a read faces a site when it ends (forward read, RIGHT site) or begins (reverse read, LEFT site) less than this many bp in front of it (1 or more)" },
    { "--clip-sites-mate-overhang", O_CLI, false, "5", "with --clip-sites-mates 1: a facing read may reach this many bp across the site (0 or more)" },
    { "--clip-sites-mate-min-dist", O_CLI, false, "1000", "with --clip-sites-mates 1: a pair on one contig and opposite strands is discordant (far) when the mate begins at least this many bp from the read (1 or more)" },
    { "--clip-sites-mate-max-gap", O_CLI, false, "500", "with --clip-sites-mates 1: mates of one contig and strand whose start positions lie at most this far apart join one cluster (0 or more)" },
    { "--clip-sites-mate-min-pairs", O_CLI, false, "2", "with --clip-sites-mates 1: a cluster gets an M line from this many pairs on (1 or more)" },
    { "--timing", O_CLI, true, "", "per-stage thread-seconds on stderr; with --score-mem-mb also the chunks per tile" },
    { "--device-inflate", O_CLI, true, "", "inflate the BGZF blocks on the GPU" },
    { "--repeat", O_CLI, false, "1", "benchmark aid: the tile list n times" },
    { "--normal-bam", O_CLI, false, "", "T/N pair in one run (uvcTN.sh): the normal sample's BAM; inputBAM is the tumor's, -o the normal VCF" },
    { "--tumor-output", O_CLI, false, "", "with --normal-bam: the tumor VCF" },
    { "--tumor-params", O_CLI, true, "", "with --normal-bam: the options after it go to the tumor side only" },
    { "--normal-params", O_CLI, true, "", "with --normal-bam: the options after it go to the normal side only" },
    { "--print-params", O_CLI, true, "", "print the resolved parameters as name=value lines in .def order and exit (no device)" },
    { "-h,--help", O_CLI, true, "", "this text" },
    { "-v,--version", O_CLI, true, "", "the version" },
    { "--assay-type", O_MODE, false, "0", "0 inferred per region, 1 CAPTURE, 2 AMPLICON (main.cpp:511)" },
    { "--sequencing-platform", O_MODE, false, "0", "0 AUTO, 1 ILLUMINA, 2 IONTORRENT (taken as given), 3 OTHER (inferred, no platform deltas)" },
    { "--molecule-tag", O_MODE, false, "0", "0 AUTO, 1 NONE, 2 BARCODING, 3 DUPLEX: read-name UMIs" },
    { "--disable-duplex", O_MODE, false, "0", "0 or 1 (1: a duplex UMI counts as a plain one)" },
    { "--pair-end-merge", O_MODE, false, "0", "0 YES, 1 NO" },
    { "--all-germline-out", O_MODE, true, "", "every allele of germline variants (should_output_all_germline = 1)" },
    { "--central-readlen", O_MODE, false, "0", "read length of the assay (0: inferred)" },
    // INERT: parsed by the reference, no effect on what it writes (each grepped in the reference)
    { "--always-log", O_INERT, false, "0", "logging only (grouping.cpp:947, main.cpp:477)" },
    { "--bias-orientation-counter-avg-end-len", O_INERT, false, "20", "no statement reads it" },
    { "--bias-thres-aLPxT-perc", O_INERT, false, "160", "no statement reads it" },
    { "--bias-thres-aXM1T-add", O_INERT, false, "30", "its use is commented out (main.hpp:1883)" },
    { "--microadjust-fam-lowfreq-invFA", O_INERT, false, "1000", "its uses are commented out (main.hpp:4996-4999)" },
    { "--microadjust-ref-MQ-dec-max", O_INERT, false, "15", "no statement reads it" },
    { "--debug-warn-min-read-end-ins-cigar-oplen", O_INERT, false, "16", "a warning on stderr only (main.hpp:2015)" },
    // not options of the reference as built (COMPILATION_ENABLE_XMGOT is 0, common.hpp:4; main.hpp:1259-1267) or commented out there
    // (CmdLineArgs.cpp:418-425, grouping.cpp:837-845): accepted for command lines written for builds that have them
    { "--bias-thres-PFXM1T-add", O_INERT, false, "130", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFXM2T-add", O_INERT, false, "20", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFGO1T-add", O_INERT, false, "125", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFGO2T-add", O_INERT, false, "15", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFXM1T-perc", O_INERT, false, "50", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFXM2T-perc", O_INERT, false, "70", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFGO1T-perc", O_INERT, false, "50", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFGO2T-perc", O_INERT, false, "70", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFXM1NT-perc", O_INERT, false, "70", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--bias-thres-PFGO1NT-perc", O_INERT, false, "70", "compiled out (COMPILATION_ENABLE_XMGOT 0)" },
    { "--dedup-amplicon-count-to-surrcount-ratio", O_INERT, false, "16", "commented out (grouping.cpp:837-845)" },
    { "--dedup-amplicon-count-to-surrcount-ratio-twosided", O_INERT, false, "4", "commented out (grouping.cpp:837-845)" },
    // UNSUPPORTED
    { "--fam-consensus-out-fastq", O_UNSUPPORTED, false, "", "the consensus FASTQ of UMI families is not written" },
    { "--fam-consensus-out-fastq-thres-dup1add", O_UNSUPPORTED, false, "1", "the consensus FASTQ of UMI families is not written" },
    { "--should-add-note", O_UNSUPPORTED, false, "0", "the FORMAT/note field is not written" },
    { "--debug-note-flag", O_UNSUPPORTED, false, "0", "the debug notes of the records (INFO/RBAQ, main.hpp:6229) are not written" },
    { "--debug-tid", O_UNSUPPORTED, false, "-1", "the per-locus debug dump is not written" },
    { "--debug-pos", O_UNSUPPORTED, false, "-1", "the per-locus debug dump is not written" },
    { "--bed-in-avg-sequencing-DP", O_UNSUPPORTED, false, "-1", "the regions are not planned from BED read counts" },
    { "--bed-in-avg-sequencing-DP-n-from-t", O_UNSUPPORTED, false, "0", "the regions are not planned from BED read counts" },
};

// fn(item) for every item of the comma-separated v, the empty ones included ("" is one empty item)
template <class F> void for_items(const std::string &v, F fn) {
    for (size_t at = 0; at <= v.size();) { size_t c = v.find(',', at); if (c == std::string::npos) c = v.size(); fn(v.substr(at, c - at)); at = c + 1; }
}
const OptRow *find_opt(const std::string &name) {
    for (const OptRow &r : OPTS) {
        bool hit = false;
        for_items(r.names, [&](const std::string &n) { hit |= (n == name); });
        if (hit) return &r;
    }
    return nullptr;
}
// the settable .def row whose option form is `--name`, else -1
int32_t find_param(const std::string &opt) {
    if (opt.size() < 3 || opt.compare(0, 2, "--") != 0) return -1;
    const std::string field = opt.substr(2);
    for (int32_t i = 0, n = uvcgpu_param_count(); i < n; i++) {
        const char *nm; int32_t settable;
        uvcgpu_param_info(i, &nm, nullptr, nullptr, nullptr, &settable);
        std::string f = nm; std::replace(f.begin(), f.end(), '_', '-');
        if (settable && f == field) return i;
    }
    return -1;
}
std::string option_name(const char *field) { std::string f = std::string("--") + field; std::replace(f.begin(), f.end(), '_', '-'); return f; }
std::string fmt_value(int32_t kind, double v) { char b[64]; if (kind == UVC_PARAM_INT) snprintf(b, sizeof(b), "%d", (int)v); else snprintf(b, sizeof(b), "%.17g", v); return b; }
bool number(const std::string &s, double *v) {   // a whole decimal number, or true / false
    if (s == "true" || s == "false") { *v = (s == "true"); return true; }
    if (s.empty() || isspace((unsigned char)s[0])) return false;
    char *e = nullptr; *v = strtod(s.c_str(), &e); return *e == 0 && std::isfinite(*v);
}

// A whole number of lo..hi in one of the three spellings the options have grown:
//   N_STRTOD       what number() takes, without true / false: 1e3, 0x10 and +5 pass; '', ' 5', '5 ' and 2.5 do not
//   N_DIGITS       [0-9]+ only
//   N_STRTOD_BOOL  N_STRTOD, and true is 1, false is 0
enum Spelling { N_STRTOD, N_DIGITS, N_STRTOD_BOOL };
bool is_whole(const std::string &v, double lo, double hi, Spelling sp, int64_t *n) {
    double x;
    if (sp != N_STRTOD_BOOL && (v == "true" || v == "false")) return false;
    if (sp == N_DIGITS && v.find_first_not_of("0123456789") != std::string::npos) return false;
    if (!number(v, &x) || x < lo || x > hi || x != (double)(int64_t)x) return false;   // range first: the cast needs it
    *n = (int64_t)x; return true;
}
int64_t whole_number(const std::string &opt, const std::string &v, double lo, double hi, const char *takes, Spelling sp = N_STRTOD) {
    int64_t n;
    if (!is_whole(v, lo, hi, sp, &n)) die(opt + " takes " + takes + ", not '" + v + "'");
    return n;
}

// What the report options (the rows of REPORTS) share on the command line.  Each option gives its own words for why; the sentences are these.
// the runs no report can come from: the header-only run, one shard of many, a repeated tile list
void refuse_report_runs(const Opts &o, const std::string &opt, const char *why_no_shard, const char *why_no_repeat) {
    if (o.bam == ONLY_PRINT_VCF_HEADER) die(opt + " cannot go with " + ONLY_PRINT_VCF_HEADER + ": no tile is called");
    if (o.n_shards > 1) die(opt + " cannot go with --shard " + std::to_string(o.shard) + "/" + std::to_string(o.n_shards) + ": " + why_no_shard + ", and --concat joins VCFs only");
    if (o.repeat != 1) die(opt + " cannot go with --repeat " + std::to_string(o.repeat) + ": " + why_no_repeat);
}
// the targets of a report with target lines: the lines of the BED file, or windows of `window` bp (wopt) without one
void refuse_report_windows(const Opts &o, const std::string &opt, const std::string &wopt, int64_t window) {
    const bool has_bed = (!o.bed.empty() || !o.bed_in.empty());
    if (has_bed && window > 0) die(wopt + " cannot go with -R / --bed-in-fname: with a BED file the targets of " + opt + " are its lines");
    if (!has_bed && window <= 0) die(opt + " needs " + wopt + " N without -R / --bed-in-fname: there are no BED lines to report on");
}
// the windows of N bp, aligned to multiples of N, that [beg, end) reaches into, each clipped to it: fn(k, begin, end) of window k
template <class F> void for_windows(int64_t beg, int64_t end, int64_t N, F fn) {
    for (int64_t k = beg / N; k * N < end; k++) fn(k, std::max(k * N, beg), std::min((k + 1) * N, end));
}
void probe_create(const std::string &opt, const std::string &path) {   // an empty file now: the run's last step writes the report over it
    FILE *probe = fopen(path.c_str(), "wb");
    if (!probe) die(opt + ": cannot create " + path);
    fclose(probe);
}

void help() {
    printf("usage: uvc1-mi355x inputBAM -f ref.fa -o out.vcf.gz [options]\n"
           "       uvc1-mi355x /only-print-vcf-header/ [options]     the VCF header of the resolved parameters on stdout\n"
           "       uvc1-mi355x inputBAM --print-params [options]     the resolved parameters as name=value lines\n"
           "       uvc1-mi355x TUMOR.bam --normal-bam NORMAL.bam -f ref.fa -o normal.vcf.gz --tumor-output tumor.vcf.gz -s TUM,NOR [options]\n"
           "                   [--tumor-params OPT..] [--normal-params OPT..]     a tumor/normal pair in one run (uvcTN.sh)\n"
           "       uvc1-mi355x --concat out.vcf.gz shard0.vcf.gz shard1.vcf.gz ...\n"
           "Every option takes `--opt value` or `--opt=value`.  User values come first, then the platform step of --sequencing-platform\n"
           "adds its deltas on top of them (CmdLineArgs.cpp:37-134).  [CLASS]: PARAM / GROUP = a parameter of the hot path / of the family\n"
           "pass; INERT = accepted, no effect (the reference reads no such value); UNSUPPORTED = refused unless at its default.\n");
    for (const OptRow &r : OPTS) printf("  %s [%s] default=%s  %s\n", r.names, CLASS_NAME[r.cls], r.flag ? "off" : (*r.dflt ? r.dflt : "\"\""), r.what);
    for (int32_t i = 0, n = uvcgpu_param_count(); i < n; i++) {
        const char *nm; int32_t kind, owner, settable; double d;
        uvcgpu_param_info(i, &nm, &kind, &owner, &d, &settable);
        const std::string opt = option_name(nm);
        if (!settable || find_opt(opt)) continue;
        printf("  %s [%s] default=%s  %s\n", opt.c_str(), owner == UVC_PARAM_OF_GROUP ? "GROUP" : "PARAM", fmt_value(kind, d).c_str(), kind == UVC_PARAM_INT ? "int" : "double");
    }
}

Opts parse(int argc, char **argv) {
    Opts o;
    uvcgpu_params_default(&o.P);
    uvcgpu_group_params_default(&o.G);
    auto set_row = [&](const char *row, const std::string &opt, const std::string &v) {
        if (uvcgpu_param_set(&o.P, &o.G, row, v.c_str())) die(opt + ": " + uvcgpu_last_error());
    };
    auto enum_value = [&](const std::string &opt, const std::string &v, int hi) {
        int64_t x; if (!is_whole(v, 0, hi, N_STRTOD_BOOL, &x)) die(opt + ": '" + v + "' is not one of 0.." + std::to_string(hi));
        return (int)x;
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a.empty() || a[0] != '-') {
            if (o.bam.empty()) o.bam = a; else die("more than one inputBAM");
            continue;
        }
        std::string name = a, inline_value; bool has_value = false;
        if (a.compare(0, 2, "--") == 0 && a.find('=') != std::string::npos) { name = a.substr(0, a.find('=')); inline_value = a.substr(a.find('=') + 1); has_value = true; }
        const OptRow *row = find_opt(name);
        const int32_t prow = row ? -1 : find_param(name);
        if (!row && prow < 0) die("unknown option " + a + " (uvc1-mi355x --help lists every option)");
        if (row && row->flag && has_value) die(name + " takes no value");
        auto val = [&]() -> std::string { if (has_value) return inline_value; if (i + 1 >= argc) die("missing value of " + name); return argv[++i]; };
        if (!row) {   // PARAM / GROUP
            const char *field; uvcgpu_param_info(prow, &field, nullptr, nullptr, nullptr, nullptr);
            set_row(field, name, val());
            continue;
        }
        const std::string n0 = std::string(row->names).substr(0, std::string(row->names).find(','));   // the first name of the row
        if (row->cls == O_INERT) { const std::string v = val(); double x; if (!number(v, &x)) die(name + ": '" + v + "' is not a number"); continue; }
        if (row->cls == O_UNSUPPORTED) {
            const std::string v = val(); double x, d;
            const bool at_default = (v == row->dflt) || (!*row->dflt && v == ".") || (number(v, &x) && number(row->dflt, &d) && x == d);
            if (!at_default) die(name + " " + v + " is not supported: " + row->what);
            continue;
        }
        int sub; const int rep = report_of(n0, &sub);
        if (rep >= 0 && sub < 0) { o.report[rep].path = val(); if (o.report[rep].path.empty()) die(n0 + " needs a path"); continue; }
        if (rep >= 0) o.report[rep].subs_given |= 1u << sub;
        if (n0 == "-f") o.fasta = val();
        else if (n0 == "-o") o.out = val();
        else if (n0 == "-s") o.sample = val();
        else if (n0 == "--targets") o.targets = val();
        else if (n0 == "-R") o.bed = val();
        else if (n0 == "-t") o.threads = std::max(1, atoi(val().c_str()));
        else if (n0 == "-A") set_row("should_output_all", name, "1");
        else if (n0 == "--force-sites") { o.force_sites = val(); if (o.force_sites.empty()) die("--force-sites needs a path"); }
        else if (n0 == "-q") set_row("vqual", name, val());
        else if (n0 == "--outvar-flag") set_row("outvar_flag", name, val());
        else if (n0 == "--tile") o.tile = std::max<int64_t>(100, atoll(val().c_str()));
        else if (n0 == "--merge-regions") o.merge = whole_number(n0, val(), 0, 2e9, "a distance in bp (0 = off)", N_STRTOD_BOOL);
        else if (n0 == "--score-mem-mb") o.score_mem_mb = whole_number(n0, val(), 0, 1e9, "a size in MiB (0 = off)");
        else if (n0 == "--coverage-thresholds") {   // a,b,c: whole decimal numbers, ascending, at most 8
            const std::string v = val(); o.coverage_thr.clear();
            for_items(v, [&](const std::string &item) {
                int64_t x;
                if (!is_whole(item, 0, 2e9, N_STRTOD, &x)) die("--coverage-thresholds takes up to 8 ascending depths such as 1,20,100,500, not '" + v + "' ('" + item + "' is not a depth)");
                if (!o.coverage_thr.empty() && (int32_t)x <= o.coverage_thr.back()) die("--coverage-thresholds must ascend: '" + v + "' has " + item + " behind " + std::to_string(o.coverage_thr.back()));
                o.coverage_thr.push_back((int32_t)x);
                if (o.coverage_thr.size() > (size_t)UVC_COV_MAX_THRESHOLDS) die("--coverage-thresholds takes at most " + std::to_string((int)UVC_COV_MAX_THRESHOLDS) + " depths, not '" + v + "'");
            });
        }
        else if (n0 == "--coverage-window" || n0 == "--family-stats-window" || n0 == "--fragment-profile-window") o.report[rep].window = whole_number(n0, val(), 1, 2e9, "a window length in bp");
        else if (n0 == "--error-profile-min-depth") o.errprof_req.min_depth = (int32_t)whole_number(n0, val(), 1, 2e9, "a depth of at least 1");
        else if (n0 == "--error-profile-max-alt-permille") o.errprof_req.max_alt_permille = (int32_t)whole_number(n0, val(), 0, 1000, "thousandths from 0 to 1000");
        else if (n0 == "--callable-min-depth") {   // NAME=N,...: the names of uvcgpu_coverage_measure_name, each at most once, whole numbers >= 0
            const std::string v = val();
            bool seen[UVC_NCOV] = {};
            for (int32_t m = 0; m < UVC_NCOV; m++) o.call_req.min_depth[m] = 0;
            for_items(v, [&](const std::string &item) {
                const size_t eq = item.find('=');
                const std::string name = item.substr(0, eq), num = (eq == std::string::npos ? "" : item.substr(eq + 1));
                int32_t m = -1;
                for (int32_t q = 0; q < UVC_NCOV; q++) if (name == uvcgpu_coverage_measure_name(q)) m = q;
                int64_t x;
                if (m < 0) die("--callable-min-depth takes NAME=N[,NAME=N...] with the names aDP bDP cDP1 cDP12 cDP2 dDP1, not '" + v + "' ('" + name + "' is not a depth)");
                if (!is_whole(num, 0, 2e9, N_DIGITS, &x)) die("--callable-min-depth takes NAME=N[,NAME=N...], not '" + v + "' ('" + num + "' is not a whole number >= 0)");
                if (seen[m]) die("--callable-min-depth names " + name + " twice in '" + v + "'");
                seen[m] = true; o.call_req.min_depth[m] = (int32_t)x;
            });
        }
        else if (n0 == "--callable-max-aDP") o.call_req.max_aDP = (int32_t)whole_number(n0, val(), 0, 2e9, "a depth (0 = off)", N_DIGITS);
        else if (n0 == "--msi-min-tract") o.msi_req.min_tracklen = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--msi-min-units") o.msi_req.min_units = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--msi-max-unit") o.msi_req.max_unitlen = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--msi-min-depth") o.msi_min_depth = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--msi-unstable-permille") o.msi_unstable_permille = (int32_t)whole_number(n0, val(), 0, 2e9, "thousandths of the depth (a whole number >= 0)");
        else if (n0 == "--read-profile-min-mapq") o.readprof_req.min_mapq = (int32_t)whole_number(n0, val(), 0, 255, "a mapping quality from 0 to 255");
        else if (n0 == "--read-profile-min-depth") o.readprof_req.min_depth = (int32_t)whole_number(n0, val(), 1, 2e9, "a depth of at least 1");
        else if (n0 == "--read-profile-max-alt-permille") o.readprof_req.max_alt_permille = (int32_t)whole_number(n0, val(), 0, 1000, "thousandths from 0 to 1000");
        else if (n0 == "--fragment-profile-min-mapq") o.fragprof_req.min_mapq = (int32_t)whole_number(n0, val(), 0, 255, "a mapping quality from 0 to 255");
        else if (n0 == "--fragment-profile-short" || n0 == "--fragment-profile-long") {   // A-B: two whole numbers >= 0, A <= B
            const std::string v = val();
            const size_t dash = v.find('-');
            int64_t a = 0, b = 0;
            if (dash == std::string::npos || !is_whole(v.substr(0, dash), 0, 2e9, N_DIGITS, &a) || !is_whole(v.substr(dash + 1), 0, 2e9, N_DIGITS, &b)) die(n0 + " takes A-B, two lengths in bp such as 100-150, not '" + v + "'");
            if (a > b) die(n0 + " takes A-B with A at most B, not '" + v + "'");
            if (n0 == "--fragment-profile-short") { o.fragprof_req.short_lo = (int32_t)a; o.fragprof_req.short_hi = (int32_t)b; } else { o.fragprof_req.long_lo = (int32_t)a; o.fragprof_req.long_hi = (int32_t)b; }
        }
        else if (n0 == "--site-reads-sites") { o.sitereads_sites = val(); if (o.sitereads_sites.empty()) die("--site-reads-sites needs a path"); }
        else if (n0 == "--site-reads-min-mapq") o.sitereads_req.min_mapq = (int32_t)whole_number(n0, val(), 0, 255, "a mapping quality from 0 to 255");
        else if (n0 == "--site-reads-alt-only") o.sitereads_req.alt_only = (int32_t)whole_number(n0, val(), 0, 1, "0 or 1 (false or true)", N_STRTOD_BOOL);
        else if (n0 == "--clip-sites-min-clip") o.clipsites_req.min_clip = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--clip-sites-min-reads") o.clipsites_req.min_reads = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--clip-sites-min-mapq") o.clipsites_req.min_mapq = (int32_t)whole_number(n0, val(), 0, 255, "a mapping quality from 0 to 255");
        else if (n0 == "--clip-sites-reads") o.clipsites_reads = (int32_t)whole_number(n0, val(), 0, 1, "0 or 1 (false or true)", N_STRTOD_BOOL);
        else if (n0 == "--clip-sites-junctions") o.clipsites_junctions = (int32_t)whole_number(n0, val(), 0, 1, "0 or 1 (false or true)", N_STRTOD_BOOL);
        else if (n0 == "--clip-sites-junction-min-len") o.clipjunc_req.min_len = (int32_t)whole_number(n0, val(), 1, UVC_CLIPSITE_NCONS, "a whole number from 1 to 32");
        else if (n0 == "--clip-sites-junction-max-mismatch") o.clipjunc_req.max_mismatch = (int32_t)whole_number(n0, val(), 0, UVC_CLIPJUNC_NHIST - 1, "a whole number from 0 to 7");
        else if (n0 == "--clip-sites-junction-min-votes") o.clipjunc_req.min_votes = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--clip-sites-junction-max-dist") o.clipjunc_req.max_dist = (int32_t)whole_number(n0, val(), 0, 2e9, "a distance in bp (0 = the whole region)");
        else if (n0 == "--clip-sites-junction-slop") o.clipjunc_req.mate_slop = (int32_t)whole_number(n0, val(), 0, 2e9, "a distance in bp");
        else if (n0 == "--clip-sites-mates") o.clipsites_mates = (int32_t)whole_number(n0, val(), 0, 1, "0 or 1 (false or true)", N_STRTOD_BOOL);
        else if (n0 == "--clip-sites-mate-window") o.clipmates_req.window = (int32_t)whole_number(n0, val(), 1, 2e9, "a distance in bp of at least 1");
        else if (n0 == "--clip-sites-mate-overhang") o.clipmates_req.overhang = (int32_t)whole_number(n0, val(), 0, 2e9, "a distance in bp");
        else if (n0 == "--clip-sites-mate-min-dist") o.clipmates_req.min_dist = (int32_t)whole_number(n0, val(), 1, 2e9, "a distance in bp of at least 1");
        else if (n0 == "--clip-sites-mate-max-gap") o.clipmates_req.max_gap = (int32_t)whole_number(n0, val(), 0, 2e9, "a distance in bp");
        else if (n0 == "--clip-sites-mate-min-pairs") o.clipmates_req.min_pairs = (int32_t)whole_number(n0, val(), 1, 2e9, "a whole number of at least 1");
        else if (n0 == "--mem-per-thread") o.mem_per_thread = std::max<int64_t>(1, atoll(val().c_str()));
        else if (n0 == "--devices") {   // comma-separated HIP device ids; an id may repeat (two workers sets on one GPU)
            o.devices.clear();
            for_items(val(), [&](const std::string &id) { if (!id.empty()) o.devices.push_back(atoi(id.c_str())); });
            if (o.devices.empty()) die("--devices needs at least one id");
        }
        else if (n0 == "--shard") { const std::string v = val(); if (sscanf(v.c_str(), "%d/%d", &o.shard, &o.n_shards) != 2 || o.n_shards < 1 || o.shard < 0 || o.shard >= o.n_shards) die("--shard takes i/n with 0 <= i < n"); }
        else if (n0 == "--no-header") o.no_header = true;
        else if (n0 == "--timing") o.timing = true;
        else if (n0 == "--device-inflate") o.device_inflate = true;   // the BGZF blocks of the BAM inflated by the GPU (uvcgpu_bgzf_inflate) instead of the host cores
        else if (n0 == "--tumor-vcf") o.tumor_vcf = val();
        else if (n0 == "--tn-is-paired") set_row("tn_is_paired", name, val());
        else if (n0 == "--is-tumor-format-retrieved") o.tumor_format = atoi(val().c_str());
        else if (n0 == "--bed-out-fname") o.bed_out = val();
        else if (n0 == "--bed-in-fname") o.bed_in = val();
        else if (n0 == "--repeat") o.repeat = std::max(1, atoi(val().c_str()));   // benchmark aid: the tile list n times (steady state on a small file)
        else if (n0 == "--print-params") o.print_params = true;
        else if (n0 == "--normal-bam" || n0 == "--tumor-output" || n0 == "--tumor-params" || n0 == "--normal-params") die(name + " belongs to pair mode (split_pair)");
        else if (n0 == "-h") { help(); exit(0); }
        else if (n0 == "-v") { printf("uvc1-mi355x (%s)\n", uvcgpu_version()); exit(0); }
        // MODE
        else if (n0 == "--assay-type") o.assay_type = enum_value(name, val(), 2);
        else if (n0 == "--sequencing-platform") o.sequencing_platform = enum_value(name, val(), 3);
        // the enum values of common.hpp:124-146 only: the reference merges for every pair_end_merge but NO (grouping.cpp:627), the family
        // pass for YES alone (uvc_group.hip), so a value outside them would not mean the same here
        else if (n0 == "--molecule-tag") set_row("molecule_tag", name, std::to_string(enum_value(name, val(), 3)));   // read-name digest + UvcGroupParams (call_tile)
        else if (n0 == "--disable-duplex") set_row("disable_duplex", name, std::to_string(enum_value(name, val(), 1)));
        else if (n0 == "--pair-end-merge") set_row("pair_end_merge", name, std::to_string(enum_value(name, val(), 1)));
        else if (n0 == "--all-germline-out") set_row("should_output_all_germline", name, "1");
        else if (n0 == "--central-readlen") set_row("central_readlen", name, val());  // 0 = inferred by the platform step
        else die("option without a handler: " + name);
    }
    if (o.bam.empty() || (!o.print_params && o.bam != ONLY_PRINT_VCF_HEADER && (o.fasta.empty() || o.out.empty()))) {
        fprintf(stderr, "usage: uvc1-mi355x inputBAM -f ref.fa -o out.vcf.gz [options] (--help lists them)\n");
        exit(2);
    }
    if (!o.force_sites.empty()) {   // before any file or device
        if (!o.tumor_vcf.empty()) die("--force-sites cannot go with --tumor-vcf: the normal sample's gate is the tumor's rescue set");
        if (o.bam == ONLY_PRINT_VCF_HEADER) die(std::string("--force-sites cannot go with ") + ONLY_PRINT_VCF_HEADER + ": there are no records to force");
    }
    // the report options, before any file or device
    for (int r = 0; r < N_REPORTS; r++) {
        const ReportRow &R = REPORTS[r];
        if (o.report[r].path.empty()) {
            if (o.report[r].subs_given && R.needs) die(R.needs);
            for (int s = 0; R.subs[s]; s++) if ((o.report[r].subs_given >> s) & 1) die(std::string(R.subs[s]) + " needs " + R.out + ": it only shapes that report");
            continue;
        }
        refuse_report_runs(o, R.out, R.why_no_shard, R.why_no_repeat);
        if (R.window) refuse_report_windows(o, R.out, R.window, o.report[r].window);
        if (r == R_CLIPSITES && !o.clipsites_junctions)   // the junction sub-options shape the J lines alone
            for (int s = 0; R.subs[s]; s++) if (((o.report[r].subs_given >> s) & 1) && !strncmp(R.subs[s], "--clip-sites-junction-", 22)) die(std::string(R.subs[s]) + " needs --clip-sites-junctions 1: it only shapes the J lines");
        if (r == R_CLIPSITES && !o.clipsites_mates)   // the mate sub-options shape the P and M lines alone
            for (int s = 0; R.subs[s]; s++) if (((o.report[r].subs_given >> s) & 1) && !strncmp(R.subs[s], "--clip-sites-mate-", 18)) die(std::string(R.subs[s]) + " needs --clip-sites-mates 1: it only shapes the P and M lines");
        if (r == R_SITEREADS && o.sitereads_sites.empty()) die("--site-reads-out needs --site-reads-sites FILE: the report is about the sites of that file");
    }
    if (o.merge > 0) {   // before any file or device
        if (o.bed.empty() && o.bed_in.empty()) die("--merge-regions needs a BED file (-R / --bed-in-fname): it merges BED lines");
        if (!o.tumor_vcf.empty()) die("--merge-regions cannot go with --tumor-vcf: the normal pass of a T/N pair is called region by region");
    }
    if (const int rc = uvcgpu_params_check(&o.P)) die(std::string(uvcgpu_last_error()) + " (code " + std::to_string(rc) + ")");   // before any file or device
    if (!o.tumor_vcf.empty()) o.P.tumor_vcf_is_provided = 1;   // IS_PROVIDED(vcf_tumor_fname), common.hpp:56
    if (const char *us = getenv("ONE_STEP_UMI_STRUCT")) o.umi_struct = us;   // the reference takes the in-read UMI pattern from the environment (main.cpp:1224-1225)
    return o;
}

// --print-params: every row of both tables, in .def order
void print_params(const Opts &o, const char *prefix = "") {
    for (int32_t i = 0, n = uvcgpu_param_count(); i < n; i++) {
        const char *nm; int32_t kind; double v;
        uvcgpu_param_info(i, &nm, &kind, nullptr, nullptr, nullptr);
        uvcgpu_param_get(&o.P, &o.G, i, &v);
        printf("%s%s=%s\n", prefix, nm, fmt_value(kind, v).c_str());
    }
}

// A tile of a run of adjacent tiles.  The reference scores zerobased_pos rpos_beg .. rpos_end inclusive without the BASE sub-position of
// the first (main.cpp:608, 643): adjacent regions both write the LINK records of their shared end point.  Here a tile owns the positions
// [beg, end): `continues` (a tile ends where this one begins) = it scores `beg` completely, `has_next` = it leaves `end` to the next one.
// `run_beg` = begin of the run (incluBegPosition of the BED line the run came from, main.cpp:655-656).
// `target` (--coverage-out with a BED file): the report row of the BED line the tile was cut from.
// `fam_target` (--family-stats-out with a BED file): the same for the family report.
// `frag_target` (--fragment-profile-out with a BED file): the same for the fragment profile.
// `call_target` (--callable-out, --msi-out): the store's target the tile was cut from; -1 (the reference's own cuts): the called span of its contig.
struct Tile { int32_t tid; std::string chrom; int64_t beg, end; bool continues, has_next; int64_t run_beg; int64_t target = -1; int64_t fam_target = -1; int64_t call_target = -1; int64_t frag_target = -1; };

// one worker: its own handles, one region handle for all of its tiles
struct Worker {
    uvcio_bam_t *bam = nullptr; uvcio_fasta_t *fa = nullptr; uvcgpu_region_t *reg = nullptr;
    std::vector<uint64_t> h31, h17, u31, u17; std::vector<uint8_t> kind;
    std::vector<int32_t> filt, isz, order, fam, frag; std::vector<uint8_t> fstrand, dflag, idflag;
    std::vector<int32_t> pos, mpos, isize, nm, lq, ncig, fragp, famp; std::vector<uint16_t> flag; std::vector<uint8_t> mapq, strandp; std::vector<int64_t> soff, coff;
    std::vector<int32_t> fields; std::string ref;
    double t_fetch = 0, t_group = 0, t_region = 0, t_reads = 0, t_gpu = 0, t_text = 0;
    int64_t n_tiles = 0, score_cap = 0, text_cap = 0;   // what the last tiles needed: the next call asks for it at once
    int64_t n_chunks = 0, n_streamed = 0;               // --score-mem-mb: chunks in all, tiles scored as streams
    std::vector<UvcScoreRange> covered;
    // the reports: the pieces of one tile and their targets.  One list each for all of them: every *_of_tile clears it, fills it, calls and
    // hands the result to its store before the next one runs
    std::vector<UvcCoverageRange> ranges; std::vector<int64_t> targets;
    std::vector<UvcFamilyRange> fam_ranges;   // --family-stats-out, --fragment-profile-out: their pieces carry more than a range
    std::vector<int64_t> cov_rows, fam_rows, rp_row, frag_rows;   // --coverage-out, --family-stats-out, --read-profile-out, --fragment-profile-out: what the device call fills
    std::vector<UvcCallableRun> call_runs;   // --callable-out: the runs, as many as the last tiles had
    std::vector<int32_t> sr_sites, sr_counts; std::vector<UvcSiteRead> sr_rows; std::vector<const char *> sr_qnames;   // --site-reads-out: the sites a tile owns, their counts and rows, the names of the rows' alignments
    std::vector<int64_t> cs_junc;   // --clip-sites-junctions 1: the junction rows of a tile's sites
    std::vector<int32_t> cm_mtid; std::vector<int64_t> cm_sites, cm_clusters; std::vector<UvcClipMate> cm_reads;   // --clip-sites-mates 1: the mate contigs of the kept alignments; the site rows, kept clusters and witness rows of a tile
    std::vector<int64_t> cs_rows; std::vector<UvcClipRead> cs_reads; std::vector<const char *> cs_qnames;   // --clip-sites-out: the site rows and event rows of a tile, as many as the last tiles had, the names of the events' alignments
    std::vector<int32_t> msi_rows; std::vector<std::string> msi_units; std::vector<const char *> msi_unit_ptrs;   // --msi-out: the loci, as many as the last tiles had
};

// --coverage-out: the pieces of targets that one accumulated tile owns, reduced by one uvcgpu_region_coverage and merged into the report.
// `own`: the stretches the tile owns (ascending, disjoint); `target_of` >= 0: all of a stretch belongs to that row (a BED line); else the
// rows are windows of o.coverage_window bp and a stretch is cut at their multiples.
struct CovSpan { int64_t first = -1, origin = 0; };   // window mode, per contig: the row of the called span's first window, the span's begin
void coverage_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own, const std::vector<int64_t> &target_of, const CovSpan *span) {
    w.ranges.clear(); w.targets.clear();
    const int64_t N = o.report[R_COVERAGE].window;
    for (size_t q = 0; q < own.size(); q++) {
        const int64_t b = own[q].first, e = own[q].second;
        if (e <= b) continue;
        if (target_of[q] >= 0) { w.ranges.push_back(UvcCoverageRange{ (int32_t)b, (int32_t)e }); w.targets.push_back(target_of[q]); continue; }
        if (!span || span->first < 0) die("--coverage-out: a tile outside the planned windows (internal error)");
        for_windows(b, e, N, [&](int64_t k, int64_t wb, int64_t we) { w.ranges.push_back(UvcCoverageRange{ (int32_t)wb, (int32_t)we }); w.targets.push_back(span->first + (k - span->origin / N)); });
    }
    if (w.ranges.empty()) return;
    w.cov_rows.resize(w.ranges.size() * (size_t)UVC_NCOV * UVC_COV_ROW);
    if (uvcgpu_region_coverage(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), o.coverage_thr.data(), (int32_t)o.coverage_thr.size(), w.cov_rows.data())) die(uvcgpu_last_error());
    for (size_t q = 0; q < w.ranges.size(); q++)
        if (uvcio_coverage_add_piece(o.cov, w.targets[q], (int64_t)w.ranges[q].pos_end - w.ranges[q].pos_beg, &w.cov_rows[q * (size_t)UVC_NCOV * UVC_COV_ROW])) die(uvcio_last_error());
}
// w.ranges = the non-empty stretches of `own`; false: there are none
bool owned_ranges(Worker &w, const std::vector<std::pair<int64_t, int64_t>> &own) {
    w.ranges.clear();
    for (const auto &q : own) if (q.second > q.first) w.ranges.push_back(UvcCoverageRange{ (int32_t)q.first, (int32_t)q.second });
    return !w.ranges.empty();
}
// w.ranges, w.targets = the stretches of `own` clipped to the span of their target (of the store of `opt`), with the targets; false: nothing is left
bool target_ranges(Worker &w, const Opts &o, const char *opt, const std::vector<std::pair<int64_t, int64_t>> &own, const std::vector<int64_t> &target_of) {
    w.ranges.clear(); w.targets.clear();
    for (size_t q = 0; q < own.size(); q++) {   // a region of the reference's own cuts begins and ends with its reads, which may reach over the called span: the target's part of it
        if (target_of[q] < 0) die(std::string(opt) + ": a tile without a target (internal error)");
        const std::pair<int64_t, int64_t> &span = o.call_target_span[(size_t)target_of[q]];
        const int64_t b = std::max(own[q].first, span.first), e = std::min(own[q].second, span.second);
        if (e > b) { w.ranges.push_back(UvcCoverageRange{ (int32_t)b, (int32_t)e }); w.targets.push_back(target_of[q]); }
    }
    return !w.ranges.empty();
}
// sizes first: call(buffer, its capacity in items of `per` elements, &n) with the buffer of the last tiles, grown and called once more
// where this tile has more items; the number of items
template <class T, class F> int64_t sizes_first(std::vector<T> &buf, size_t per, F call) {
    int64_t n = 0;
    int rc = call(buf.data(), (int64_t)(buf.size() / per), &n);
    if (rc == UVCGPU_ENOMEM && n > (int64_t)(buf.size() / per)) { buf.resize((size_t)n * per); rc = call(buf.data(), n, &n); }
    if (rc) die(uvcgpu_last_error());
    return n;
}
// --error-profile-out: the profile of the stretches one accumulated tile owns -- the list coverage_of_tile reports on -- by one
// uvcgpu_region_error_profile, added to the run's table.
void errprofile_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own) {
    if (!owned_ranges(w, own)) return;
    int64_t prof[UVC_NERRLEVEL * UVC_ERR_ROW];
    if (uvcgpu_region_error_profile(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), &o.errprof_req, prof)) die(uvcgpu_last_error());
    if (uvcio_errprofile_add(o.errprof, prof)) die(uvcio_last_error());
}
// --family-concordance-out: the row of the stretches one accumulated tile owns -- the list coverage_of_tile reports on, so every position
// counts once across the tiles -- by one uvcgpu_region_family_concordance, added to the run's row.
void family_concordance_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own) {
    if (!owned_ranges(w, own)) return;
    int64_t row[UVC_FAMCONC_ROW];
    if (uvcgpu_region_family_concordance(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), row)) die(uvcgpu_last_error());
    if (uvcio_famconcord_add(o.famconc, row)) die(uvcio_last_error());
}
// --read-profile-out: the profile of the reads over the stretches one tile owns -- the list coverage_of_tile reports on -- by one
// uvcgpu_region_read_profile after set_reads, added to the run's row.
void readprofile_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own) {
    if (!owned_ranges(w, own)) return;
    w.rp_row.resize((size_t)UVC_READPROF_ROW);
    if (uvcgpu_region_read_profile(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), &o.readprof_req, w.rp_row.data())) die(uvcgpu_last_error());
    if (uvcio_readprofile_add(o.readprof, w.rp_row.data())) die(uvcio_last_error());
}
// --callable-out: the runs of the stretches one accumulated tile owns -- the list coverage_of_tile reports on -- by one
// uvcgpu_region_callable (sizes first: the buffer of the last tiles, grown where a tile has more runs), handed to the store with each
// stretch's target.  Joining across tiles is the store's.
void callable_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own, const std::vector<int64_t> &target_of) {
    if (!target_ranges(w, o, "--callable-out", own, target_of)) return;
    const int64_t n = sizes_first(w.call_runs, 1, [&](UvcCallableRun *runs, int64_t cap, int64_t *n_runs) { return uvcgpu_region_callable(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), &o.call_req, runs, cap, n_runs); });
    if (uvcio_callable_add_runs(o.callable, w.targets.data(), (int64_t)w.targets.size(), w.call_runs.data(), n)) die(uvcio_last_error());
}
// --msi-out: the loci whose head lies in the stretches one accumulated tile owns -- the list coverage_of_tile reports on, clipped to the
// targets as for --callable-out -- by one uvcgpu_region_msi (sizes first: the buffer of the last tiles, grown where a tile has more loci),
// handed to the store with each stretch's target and each locus's first unit as text.  ref: the reference bases of the region from ref_beg on.
void msi_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own, const std::vector<int64_t> &target_of, const std::string &ref, int64_t ref_beg) {
    if (!target_ranges(w, o, "--msi-out", own, target_of)) return;
    const int64_t n = sizes_first(w.msi_rows, UVC_MSI_ROW, [&](int32_t *rows, int64_t cap, int64_t *n_loci) { return uvcgpu_region_msi(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), &o.msi_req, rows, cap, n_loci); });
    w.msi_units.resize((size_t)n); w.msi_unit_ptrs.resize((size_t)n);
    for (int64_t q = 0; q < n; q++) {
        const int32_t *row = &w.msi_rows[(size_t)q * UVC_MSI_ROW];
        const int64_t at = (int64_t)row[UVC_MSI_pos_beg] - ref_beg;   // (a tract lies inside the reference bases of its region)
        w.msi_units[(size_t)q] = (at >= 0 && at + row[UVC_MSI_unitlen] <= (int64_t)ref.size()) ? ref.substr((size_t)at, (size_t)row[UVC_MSI_unitlen]) : std::string(".");
        for (char &c : w.msi_units[(size_t)q]) c = (char)toupper((unsigned char)c);
        w.msi_unit_ptrs[(size_t)q] = w.msi_units[(size_t)q].c_str();
    }
    if (uvcio_msi_add(o.msi, w.targets.data(), (int64_t)w.targets.size(), w.msi_rows.data(), w.msi_unit_ptrs.data(), n)) die(uvcio_last_error());
}
// --family-stats-out: the pieces of targets that the tiles own, planned before any worker starts (plan_family_pieces), so that the report
// does not depend on which worker takes which tile.  A piece is a tile's [beg, end), cut at the window borders in window mode: the planned
// stretch, not the stretch the reads of the tile happen to reach -- families are counted by overlap, and where there are no reads there are
// no families.  prev_end: the largest end of the pieces planned before it on the contig, at most its own begin (sorted, disjoint targets:
// the end of the piece before); flags: UVC_FAMRANGE_CONTINUES where the piece before belongs to the same target.
struct FamPiece { int64_t beg, end, prev_end; int32_t flags; int64_t target; };
// w.fam_ranges, w.targets = the pieces of a tile (of the `n_tiles` tiles of a merged batch) inside the region, with their targets; false: there are none
bool piece_ranges(Worker &w, const std::vector<FamPiece> *pieces, size_t n_tiles, int64_t ext_end) {
    w.fam_ranges.clear(); w.targets.clear();
    for (size_t q = 0; q < n_tiles; q++)
        for (const FamPiece &p : pieces[q]) {
            const int64_t e = std::min(p.end, ext_end + 1);   // (the region holds [ext_beg, ext_end]; a tile lies inside it)
            if (e > p.beg) { w.fam_ranges.push_back(UvcFamilyRange{ (int32_t)p.beg, (int32_t)e, (int32_t)p.prev_end, p.flags }); w.targets.push_back(p.target); }
        }
    return !w.fam_ranges.empty();
}
// One uvcgpu_region_family_stats over the pieces of a tile (of the `n_tiles` tiles of a merged batch), after set_reads: the rows go to the report.
void family_stats_of_tile(Worker &w, const Opts &o, const std::vector<FamPiece> *pieces, size_t n_tiles, int64_t ext_end) {
    if (!piece_ranges(w, pieces, n_tiles, ext_end)) return;
    w.fam_rows.resize(w.fam_ranges.size() * (size_t)UVC_FAMSTAT_ROW);
    if (uvcgpu_region_family_stats(w.reg, w.fam_ranges.data(), (int64_t)w.fam_ranges.size(), w.fam_rows.data())) die(uvcgpu_last_error());
    for (size_t q = 0; q < w.fam_ranges.size(); q++)
        if (uvcio_famstats_add_piece(o.fam, w.targets[q], &w.fam_rows[q * (size_t)UVC_FAMSTAT_ROW])) die(uvcio_last_error());
}
// --fragment-profile-out: one uvcgpu_region_fragment_profile over the pieces of a tile, planned as the family report's are (plan_family_pieces
// for this report's own targets or windows), after set_reads: the TARGET rows go to their targets, the profile row to the run's sum.
void fragment_profile_of_tile(Worker &w, const Opts &o, const std::vector<FamPiece> *pieces, size_t n_tiles, int64_t ext_end) {
    if (!piece_ranges(w, pieces, n_tiles, ext_end)) return;
    const size_t n = w.fam_ranges.size();
    w.frag_rows.resize(n * (size_t)UVC_FRAGPROF_TARGET_ROW + (size_t)UVC_FRAGPROF_ROW);
    int64_t *prof = &w.frag_rows[n * (size_t)UVC_FRAGPROF_TARGET_ROW];
    if (uvcgpu_region_fragment_profile(w.reg, w.fam_ranges.data(), (int64_t)n, &o.fragprof_req, w.frag_rows.data(), prof)) die(uvcgpu_last_error());
    for (size_t q = 0; q < n; q++)
        if (uvcio_fragprofile_add_piece(o.fragprof, w.targets[q], &w.frag_rows[q * (size_t)UVC_FRAGPROF_TARGET_ROW])) die(uvcio_last_error());
    if (uvcio_fragprofile_add_profile(o.fragprof, prof)) die(uvcio_last_error());
}
// --site-reads-out: the listed sites inside the stretches one tile owns -- the list coverage_of_tile reports on, so every site has one owner
// however the tiles are cut -- by one uvcgpu_region_site_reads behind correct_bq (sizes first: the buffer of the last tiles, grown where a
// tile has more rows), handed to the store with the columns of the kept alignments (alns3 order: a row's `read` indexes them) and the names
// of the batch.  A tile without an owned site makes no call.  A listed site is the VCF POS of uvcio_sites_*: the zero-based position + 1.
void site_reads_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own, const Tile &t, const UvcBamBatch &b, int64_t k) {
    w.sr_sites.clear();
    for (const auto &q : own) {
        const int32_t *s = nullptr; int64_t n = 0;
        if (q.second > q.first && uvcio_sites_fetch(o.sitereads_list, t.tid, q.first + 1, q.second + 1, &s, &n)) die(uvcio_last_error());
        for (int64_t i = 0; i < n; i++) w.sr_sites.push_back(s[i] - 1);
    }
    if (w.sr_sites.empty()) return;
    const int64_t n_sites = (int64_t)w.sr_sites.size();
    w.sr_counts.resize((size_t)n_sites * UVC_SITEREAD_NCOL);
    const int64_t n = sizes_first(w.sr_rows, 1, [&](UvcSiteRead *rows, int64_t cap, int64_t *n_rows) { return uvcgpu_region_site_reads(w.reg, w.sr_sites.data(), n_sites, &o.sitereads_req, w.sr_counts.data(), rows, cap, n_rows); });
    w.sr_qnames.assign((size_t)k, nullptr);
    for (int64_t i = 0; i < n; i++) { const int32_t a = w.sr_rows[(size_t)i].read; w.sr_qnames[(size_t)a] = b.qnames + b.qname_off[w.order[(size_t)a]]; }
    if (uvcio_sitereads_add(o.sitereads, t.tid, t.chrom.c_str(), w.sr_sites.data(), nullptr, n_sites, w.sr_counts.data(), w.sr_rows.data(), n, k, w.sr_qnames.data(), w.flag.data(), w.mapq.data(), w.lq.data(),
                            w.fam.data(), w.fstrand.data(), w.frag.data(), b.bases, w.soff.data())) die(uvcio_last_error());
}
// --clip-sites-out: the clip sites inside the stretches one tile owns -- the list coverage_of_tile reports on, so a site belongs to the tile
// that owns its position however the tiles are cut -- by one uvcgpu_region_clip_sites after set_reads, always with the event rows (sizes
// first on both arrays: the buffers of the last tiles, grown where a tile has more), handed to the store with the columns of the kept
// alignments (alns3 order: an event's `read` indexes them) and the names of the batch.
void clip_sites_of_tile(Worker &w, const Opts &o, const std::vector<std::pair<int64_t, int64_t>> &own, const Tile &t, const UvcBamBatch &b, int64_t k) {
    if (!owned_ranges(w, own)) return;
    int64_t totals[UVC_CLIPSITE_NTOTAL], n_reads = 0;
    const int64_t n_sites = sizes_first(w.cs_rows, UVC_CLIPSITE_ROW, [&](int64_t *rows, int64_t cap, int64_t *n) {
        int rc = uvcgpu_region_clip_sites(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), &o.clipsites_req, totals, rows, cap, n, w.cs_reads.data(), (int64_t)w.cs_reads.size(), &n_reads);
        if (rc == UVCGPU_ENOMEM && n_reads > (int64_t)w.cs_reads.size()) w.cs_reads.resize((size_t)n_reads);   // (sizes_first calls once more: with room for both)
        if (rc == UVCGPU_ENOMEM && *n <= cap) rc = uvcgpu_region_clip_sites(w.reg, w.ranges.data(), (int64_t)w.ranges.size(), &o.clipsites_req, totals, rows, cap, n, w.cs_reads.data(), (int64_t)w.cs_reads.size(), &n_reads);
        return rc;
    });
    if (n_sites == 0) return;
    w.cs_qnames.assign((size_t)k, nullptr);
    for (int64_t i = 0; i < n_reads; i++) { const int32_t a = w.cs_reads[(size_t)i].read; w.cs_qnames[(size_t)a] = b.qnames + b.qname_off[w.order[(size_t)a]]; }
    if (o.clipsites_junctions) {   // right behind the tile's clip-site call, on that call's rows: the partner is looked for in this tile's region
        int64_t jtotals[UVC_CLIPJUNC_NTOTAL];
        w.cs_junc.resize((size_t)n_sites * UVC_CLIPJUNC_ROW);
        if (uvcgpu_region_clip_junctions(w.reg, w.cs_rows.data(), n_sites, &o.clipjunc_req, w.cs_junc.data(), jtotals)) die(uvcgpu_last_error());
    }
    int64_t n_clusters = 0, n_mates = 0;
    if (o.clipsites_mates) {   // behind the tile's clip-site call, on that call's rows: the mate contigs of the kept alignments in their order, always with the witness rows
        int64_t mtotals[UVC_CLIPMATE_NTOTAL];
        UvcClipMatesRequest req = o.clipmates_req;
        req.tid = t.tid; req.min_mapq = o.clipsites_req.min_mapq;
        w.cm_mtid.resize((size_t)k);
        for (int64_t i = 0; i < k; i++) w.cm_mtid[(size_t)i] = b.mtid[w.order[(size_t)i]];
        w.cm_sites.resize((size_t)n_sites * UVC_CLIPMATE_SITE_ROW);
        n_clusters = sizes_first(w.cm_clusters, UVC_CLIPMATE_ROW, [&](int64_t *rows, int64_t cap, int64_t *n) {
            int rc = uvcgpu_region_clip_mates(w.reg, w.cs_rows.data(), n_sites, w.cm_mtid.data(), &req, mtotals, w.cm_sites.data(), rows, cap, n, w.cm_reads.data(), (int64_t)w.cm_reads.size(), &n_mates);
            if (rc == UVCGPU_ENOMEM && n_mates > (int64_t)w.cm_reads.size()) w.cm_reads.resize((size_t)n_mates);   // (sizes_first calls once more: with room for both)
            if (rc == UVCGPU_ENOMEM && *n <= cap) rc = uvcgpu_region_clip_mates(w.reg, w.cs_rows.data(), n_sites, w.cm_mtid.data(), &req, mtotals, w.cm_sites.data(), rows, cap, n, w.cm_reads.data(), (int64_t)w.cm_reads.size(), &n_mates);
            return rc;
        });
    }
    if (uvcio_clipsites_add_mates(o.clipsites, t.tid, t.chrom.c_str(), w.cs_rows.data(), o.clipsites_junctions ? w.cs_junc.data() : nullptr, n_sites, w.cs_reads.data(), n_reads, k, w.cs_qnames.data(), w.flag.data(), w.mapq.data(),
                                  w.fam.data(), w.fstrand.data(), w.frag.data(), o.clipsites_mates ? w.cm_sites.data() : nullptr, w.cm_clusters.data(), n_clusters, w.cm_reads.data(), n_mates)) die(uvcio_last_error());
}
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// The record text of one call behind `lines`: write(dst, room, &len) into a buffer as large as the last tiles needed (+ slack); a second
// call only when the text did not fit
template <class F> void append_text(Worker &w, std::string &lines, F write) {
    const size_t at = lines.size();
    int64_t len = 0, room = std::max<int64_t>(1 << 16, w.text_cap);
    for (;;) {
        lines.resize(at + (size_t)room);
        const int rc = write(&lines[at], room, &len);
        if (rc == UVCGPU_ENOMEM && len > room) { room = len + len / 4; continue; }
        if (rc) die(uvcgpu_last_error());
        break;
    }
    lines.resize(at + (size_t)len);
    w.text_cap = std::max<int64_t>(w.text_cap, len + len / 4);
}

// process_batch for one tile; appends the record lines to `lines`; false = nothing to call there.  *n_kept_reads: reads that passed the filters.
// `tumor_ready` (pair mode): called with the tumor records' range before they are fetched; returns once the store holds all of them
// --merge-regions: `t0_` is the first of `n_merged` consecutive tiles of one batch (BED lines, sorted and at least one base apart).  The batch
// is one region over [first line's begin, last line's end): one fetch, reset, set_reads and accumulate; every line becomes the score range
// its own tile would have asked for; one uvcgpu_region_score_ranges, one uvcgpu_region_vcf_records_ranges.  n_kept_reads then has n_merged
// entries: the kept alignments that overlap each line.  n_merged = 0: the plain call of one tile.
bool call_tile(Worker &w, const Opts &o, const UvcParams &P, const Tile &t0_, int64_t tlen, const uvcio_tumor_vcf_t *tvcf, std::string &lines, int64_t *n_kept_reads,
               const std::function<void(int32_t, int64_t, int64_t)> *tumor_ready = nullptr, size_t n_merged = 0, const CovSpan *cov_span = nullptr,
               const std::vector<FamPiece> *fam_pieces = nullptr, const std::vector<FamPiece> *frag_pieces = nullptr) {
    double t0 = now();
    for (size_t q = 0; q < std::max<size_t>(n_merged, 1); q++) n_kept_reads[q] = 0;
    Tile t = t0_;
    if (n_merged > 0) { t.end = (&t0_)[n_merged - 1].end; t.continues = t.has_next = false; }   // the batch's span
    UvcBamBatch b;
    if (uvcio_bam_fetch(w.bam, t.tid, std::max<int64_t>(0, t.beg - MAX_INSERT_SIZE), t.end + MAX_INSERT_SIZE, &b)) die(uvcio_last_error());
    w.t_fetch += now() - t0; t0 = now();
    const int64_t n = b.n_alns;
    if (n == 0) return false;
    w.h31.resize(n); w.h17.resize(n); w.u31.resize(n); w.u17.resize(n); w.kind.resize(n);
    uvcgpu_qname_digest_batch(b.qnames, b.qname_off, n, o.G.molecule_tag, o.G.disable_duplex, w.h31.data(), w.h17.data(), w.u31.data(), w.u17.data(), w.kind.data());
    if (!o.umi_struct.empty() && uvcgpu_umi_in_read_batch(o.umi_struct.c_str(), b.bases, b.seq_off, b.l_qseq, b.flag, n, w.kind.data(), nullptr)) die(uvcgpu_last_error());   // grouping.cpp:787-792
    UvcGroupParams gp = o.G;
    gp.fetch_tbeg = (int32_t)t.beg; gp.fetch_tend = (int32_t)t.end; gp.inferred_sequencing_platform = P.inferred_sequencing_platform;
    UvcGroupInput gi; memset(&gi, 0, sizeof(gi));
    gi.n_alns = n; gi.tid = b.tid; gi.pos = b.pos; gi.endpos = b.endpos; gi.mtid = b.mtid; gi.mpos = b.mpos; gi.isize = b.isize; gi.flag = b.flag; gi.mapq = b.mapq;
    gi.qname_hash31 = w.h31.data(); gi.qname_hash17 = w.h17.data(); gi.umi_hash31 = w.u31.data(); gi.umi_hash17 = w.u17.data(); gi.umi_kind = w.kind.data();
    w.filt.resize(n); w.isz.resize(n); w.order.resize(n); w.fam.resize(n); w.frag.resize(n); w.fstrand.resize(n); w.dflag.resize(n); w.idflag.resize(n);
    UvcGroupOut go; memset(&go, 0, sizeof(go));
    go.filter_reason = w.filt.data(); go.isize_norm = w.isz.data(); go.order = w.order.data(); go.fam_id = w.fam.data(); go.frag_id = w.frag.data();
    go.fam_strand = w.fstrand.data(); go.fam_dflag = w.dflag.data(); go.fam_idflag = w.idflag.data();
    if (uvcgpu_group_families(&gp, &gi, &go)) die(uvcgpu_last_error());
    w.t_group += now() - t0; t0 = now();
    const int64_t k = go.n_kept;
    if (n_merged == 0) *n_kept_reads = k;
    else for (int64_t i = 0; i < k; i++) {   // the lines a kept alignment overlaps (sorted, disjoint: the first line that ends behind its begin, and on)
        const int64_t rb = b.pos[w.order[(size_t)i]], re = b.endpos[w.order[(size_t)i]];
        size_t lo = 0, hi = n_merged;
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if ((&t0_)[mid].end <= rb) lo = mid + 1; else hi = mid; }
        for (; lo < n_merged && (&t0_)[lo].beg < re; lo++) n_kept_reads[lo]++;
    }
    if (k == 0) return false;
    // region bounds and reference, main.cpp:523-552
    const int64_t bam_beg = go.extended_inclu_beg_pos, bam_end = go.extended_exclu_end_pos;
    const int64_t ext_beg = std::max<int64_t>(0, std::min(t.beg, bam_beg) - MAX_STR_N_BASES), ext_end = std::min(tlen, std::max(t.end, bam_end) + MAX_STR_N_BASES);
    // what a tile (or a line of a batch) scores of the region: [first, excl); zerobased_pos `end` belongs to the next tile where there is one
    auto scored = [&](const Tile &l) { return std::make_pair(std::max(l.beg, bam_beg), l.has_next ? std::min(l.end, bam_end + 1) : std::min(std::min(l.end, bam_end) + 1, ext_end)); };
    const int64_t first = scored(t).first, last_excl = scored(t).second;
    // the ranges of a batch: per line what the lines above compute for a tile, with the batch's reads and extent
    std::vector<UvcScoreRange> ranges;
    for (size_t q = 0; q < n_merged; q++) {
        const Tile &l = (&t0_)[q];
        const int64_t l_first = scored(l).first, l_excl = scored(l).second;
        if (l_excl > l_first) ranges.push_back(UvcScoreRange{ (int32_t)l_first, (int32_t)l_excl, (l.continues && l_first == l.beg && l.beg > ext_beg) ? 1 : 0, (int32_t)l.run_beg });
    }
    if (n_merged > 0 ? ranges.empty() : last_excl <= first) return false;
    w.ref.resize((size_t)(ext_end - ext_beg));
    if (uvcio_fasta_fetch(w.fa, t.chrom.c_str(), ext_beg, ext_end, &w.ref[0])) die(uvcio_last_error());
    int rc = w.reg ? uvcgpu_region_reset(w.reg, t.tid, (int32_t)ext_beg, (int32_t)ext_end, w.ref.c_str())
                   : uvcgpu_region_create(&w.reg, &P, t.tid, (int32_t)ext_beg, (int32_t)ext_end, w.ref.c_str());
    if (rc) die(uvcgpu_last_error());
    w.t_region += now() - t0; t0 = now();
    // the kept alignments in alns3 order
    auto gather = [&](auto &dst, const auto *src) { dst.resize((size_t)k); for (int64_t i = 0; i < k; i++) dst[(size_t)i] = src[w.order[(size_t)i]]; };
    gather(w.pos, b.pos); gather(w.mpos, b.mpos); gather(w.isize, w.isz.data()); gather(w.flag, b.flag); gather(w.mapq, b.mapq); gather(w.nm, b.nm);
    gather(w.lq, b.l_qseq); gather(w.soff, b.seq_off); gather(w.coff, b.cigar_off); gather(w.ncig, b.n_cigar);
    UvcReadSoA rs; memset(&rs, 0, sizeof(rs)); rs.struct_size = (int32_t)sizeof(rs);
    rs.n_reads = k; rs.pos = w.pos.data(); rs.mpos = w.mpos.data(); rs.isize = w.isize.data(); rs.flag = w.flag.data(); rs.mapq = w.mapq.data(); rs.nm = w.nm.data();
    rs.l_qseq = w.lq.data(); rs.seq_off = w.soff.data(); rs.cigar_off = w.coff.data(); rs.n_cigar = w.ncig.data();
    rs.frag_id = w.frag.data(); rs.fam_id = w.fam.data(); rs.fam_strand = w.fstrand.data();
    rs.n_bases = b.n_bases; rs.bases = b.bases; rs.quals = b.quals; rs.n_cigar_ops = b.n_cigar_ops; rs.cigars = b.cigars;
    rs.n_fams = go.n_fams; rs.fam_dflag = w.dflag.data();
    if (uvcgpu_region_set_reads(w.reg, &rs)) die(uvcgpu_last_error());
    w.t_reads += now() - t0; t0 = now();
    if (o.fam && fam_pieces) family_stats_of_tile(w, o, fam_pieces, std::max<size_t>(n_merged, 1), ext_end);   // --family-stats-out: the units of set_reads, before anything else
    if (o.fragprof && frag_pieces) fragment_profile_of_tile(w, o, frag_pieces, std::max<size_t>(n_merged, 1), ext_end);   // --fragment-profile-out: the fragments and units of set_reads
    // --coverage-out, --error-profile-out, --callable-out, --read-profile-out, --site-reads-out, --family-concordance-out: the positions this tile owns -- the [first, last_excl) that scoring and
    // uvcio_sites_fetch go by, without the end point t.end itself, which lies outside every target the tile was cut from (and which two regions of
    // the reference's cuts share).  The list depends on scored() alone: made here, in front of accumulate, for the report of the reads as well.
    std::vector<std::pair<int64_t, int64_t>> own; std::vector<int64_t> target_of, call_target_of;
    if (o.cov || o.errprof || o.callable || o.readprof || o.msi || o.sitereads || o.clipsites || o.famconc) {
        auto call_target = [&](const Tile &l) { return l.call_target >= 0 || !(o.callable || o.msi) ? l.call_target : o.call_contig_target[(size_t)l.tid]; };
        for (size_t q = 0; q < std::max<size_t>(n_merged, 1); q++) {   // (n_merged = 0: t0_ alone)
            const Tile &l = (&t0_)[q];
            own.emplace_back(scored(l).first, std::min(scored(l).second, l.end)); target_of.push_back(l.target); call_target_of.push_back(call_target(l));
        }
    }
    if (o.readprof) readprofile_of_tile(w, o, own);   // the BAM's own qualities: in front of the correction
    if (o.clipsites) clip_sites_of_tile(w, o, own, t, b, k);   // the read columns, CIGARs and bases of set_reads: qualities are not read
    if (uvcgpu_region_correct_bq(w.reg) || uvcgpu_region_accumulate(w.reg)) die(uvcgpu_last_error());
    if (o.cov) coverage_of_tile(w, o, own, target_of, cov_span);
    if (o.errprof) errprofile_of_tile(w, o, own);
    if (o.famconc) family_concordance_of_tile(w, o, own);
    if (o.callable) callable_of_tile(w, o, own, call_target_of);
    if (o.msi) msi_of_tile(w, o, own, call_target_of, w.ref, ext_beg);
    if (o.sitereads) site_reads_of_tile(w, o, own, t, b, k);   // the corrected qualities: behind correct_bq
    UvcScoreRequest rq; memset(&rq, 0, sizeof(rq));
    rq.pos_beg = (int32_t)first; rq.pos_end = (int32_t)last_excl; rq.all_out = (P.should_output_all != 0);
    rq.is_amplicon = (o.assay_type == 0 ? (go.n_amplicon * 2 > k) : (o.assay_type == 2));   // inferred_assay_type, main.cpp:510-511
    rq.base_at_pos_beg = (t.continues && first == t.beg && t.beg > ext_beg) ? 1 : 0; rq.region_beg = (int32_t)t.run_beg;
    if (n_merged > 0) { rq.pos_beg = -1; rq.pos_end = -1; rq.base_at_pos_beg = 0; rq.region_beg = 0; }   // the ranges carry them
    if (tvcf) {   // normal sample of a T/N pair: the tumor records of this region (tkis_beg .. tkis_end, main.cpp:532-533)
        const UvcTumorKey *keys = nullptr; const char *const *cols = nullptr, *const *ras = nullptr; int64_t nk = 0;
        if (tumor_ready) (*tumor_ready)(t.tid, ext_beg, ext_end);
        if (uvcio_tumor_vcf_fetch(tvcf, t.tid, (int32_t)ext_beg, (int32_t)ext_end, &keys, &cols, &ras, &nk)) die(uvcio_last_error());
        rq.tumor_keys = keys; rq.n_tumor_keys = nk; rq.tumor_sample_columns = (o.tumor_format ? cols : nullptr); rq.tumor_ref_alt = ras;
    }
    if (o.sites && uvcio_sites_fetch(o.sites, t.tid, first, last_excl, &rq.force_sites, &rq.n_force_sites)) die(uvcio_last_error());   // the sites this tile owns
    rq.kept_only = 1;   // only the record groups that are written travel to the host
    const int64_t n_ranges = (int64_t)ranges.size();
    if (o.score_mem_mb > 0) {   // the same records and the same text, chunk by chunk: the stream's chunk is scored while the one before it is written
        const int64_t chunk_records = std::max<int64_t>(1, (o.score_mem_mb << 20) / uvcgpu_score_stream_bytes_per_record());
        uvcgpu_score_stream_t *ss = nullptr;
        if (uvcgpu_region_score_stream_begin(w.reg, &rq, n_merged > 0 ? ranges.data() : nullptr, n_merged > 0 ? n_ranges : 0, chunk_records, &ss)) die(std::string(uvcgpu_last_error()) + " (raise --score-mem-mb)");
        UvcScoreRequest rt = rq; rt.pos_beg = -1; rt.pos_end = -1; rt.base_at_pos_beg = 0; rt.region_beg = 0;   // the text of a chunk: the covered ranges carry them
        w.covered.resize((size_t)std::max<int64_t>(n_ranges, 1));
        UvcScoreOut chunk; int64_t n_cov = 0;
        double t_wait = now();
        while ((rc = uvcgpu_score_stream_next(ss, &chunk, w.covered.data(), &n_cov)) == 0) {
            w.t_gpu += now() - t_wait; t0 = now();
            append_text(w, lines, [&](char *dst, int64_t room, int64_t *len) { return uvcgpu_region_vcf_records_ranges(w.reg, t.chrom.c_str(), &chunk, &rt, w.covered.data(), n_cov, dst, room, len); });
            w.n_chunks++;
            w.t_text += now() - t0; t_wait = now();
        }
        if (rc != UVCGPU_STREAM_END) die(uvcgpu_last_error());
        if (uvcgpu_score_stream_end(ss)) die(uvcgpu_last_error());
        w.t_gpu += now() - t_wait;
        w.n_streamed++;
        return true;
    }
    const int64_t upper = n_merged > 0 ? uvcgpu_region_score_ranges_size(w.reg, &rq, ranges.data(), n_ranges) : uvcgpu_region_score_size(w.reg, &rq);
    int64_t cap = std::max<int64_t>(std::max<int64_t>(4096, w.score_cap), upper / (rq.all_out ? 1 : 64) + 16 * rq.n_force_sites);
    UvcScoreOut so;
    for (;;) {
        w.fields.resize((size_t)UVC_NUM_SCORE_FIELDS * (size_t)cap);
        so.capacity = cap; so.n_records = 0; so.fields = w.fields.data();
        rc = n_merged > 0 ? uvcgpu_region_score_ranges(w.reg, &rq, ranges.data(), n_ranges, &so) : uvcgpu_region_score(w.reg, &rq, &so);
        if (rc == UVCGPU_ENOMEM && so.n_records > cap) { cap = so.n_records + so.n_records / 4; continue; }
        if (rc) die(uvcgpu_last_error());
        break;
    }
    w.score_cap = cap;
    w.t_gpu += now() - t0; t0 = now();
    append_text(w, lines, [&](char *dst, int64_t room, int64_t *len) {
        return n_merged > 0 ? uvcgpu_region_vcf_records_ranges(w.reg, t.chrom.c_str(), &so, &rq, ranges.data(), n_ranges, dst, room, len)
                            : uvcgpu_region_vcf_records(w.reg, t.chrom.c_str(), &so, &rq, dst, room, len);
    });
    w.t_text += now() - t0;
    return true;
}
struct Geometry {   // the contigs of a BAM header
    std::vector<std::string> names; std::vector<int64_t> lens; std::vector<const char *> cnames;
    int32_t tid_of(const std::string &chrom) const { for (int32_t i = 0; i < (int32_t)names.size(); i++) if (names[(size_t)i] == chrom) return i; return -1; }
};
uvcio_bam_t *open_bam(const std::string &path, Geometry &g) {
    uvcio_bam_t *bam0 = nullptr;
    if (uvcio_bam_open(&bam0, path.c_str())) die(uvcio_last_error());
    if (!uvcio_bam_has_index(bam0)) fprintf(stderr, "uvc1-mi355x: no .bai next to %s, every tile scans the file\n", path.c_str());
    const int32_t nref = uvcio_bam_n_refs(bam0);
    for (int32_t i = 0; i < nref; i++) { g.names.push_back(uvcio_bam_ref_name(bam0, i)); g.lens.push_back(uvcio_bam_ref_len(bam0, i)); }
    for (auto &s : g.names) g.cnames.push_back(s.c_str());
    return bam0;
}

// the platform step without a look at the file: a given ILLUMINA / IONTORRENT needs none, and the header mode has no file
// (main.cpp:1229-1240 prints the header there before any platform step; here a given platform's deltas are in it)
bool apply_given_platform(Opts &o) {
    const bool platform_given = (o.sequencing_platform == UVC_PLATFORM_ILLUMINA || o.sequencing_platform == UVC_PLATFORM_IONTORRENT);
    if (platform_given) uvcgpu_params_apply_platform_ex(&o.P, o.sequencing_platform, 0, 0, 0);
    return platform_given;
}

// --print-params plans the region cuts with the same -t default as the run (the AUTO / OTHER inference reads the first region): the device
// count comes from the runtime's enumeration, no device is initialised; none visible = one
void default_devices_and_threads(Opts &o) {
    if (o.devices.empty()) {
        const int nd = uvcgpu_device_count();
        if (nd <= 0 && !o.print_params) die("no HIP device: uvc1-mi355x has no CPU path");
        for (int d = 0; d < std::max(nd, 1); d++) o.devices.push_back(d);
    }
    // tiles in flight: the host stages of a tile (inflate above all) cost ~1.3 core-seconds per 1 Mb x 300x, the device ~10 ms: as many workers
    // as half the cores this process may use keep the cores busy (measured on a 16-core quota: 4 -> 6.7, 8 -> 8-11, 12-16 -> 8-9.6 M positions/s),
    // never more than 8 per device (a region handle holds ~7 GB of planes) and at least one per device
    if (o.threads <= 0) { const int nd = (int)o.devices.size(); o.threads = std::max(nd, std::min(8 * nd, uvc_effective_cpus() / 2)); }
}

// ownership of the shared end points: a tile whose predecessor ends where it begins continues that one's run
void link_runs(std::vector<Tile> &tiles) {
    for (size_t q = 1; q < tiles.size(); q++) if (tiles[q].tid == tiles[q - 1].tid && tiles[q].beg == tiles[q - 1].end) { tiles[q].continues = true; tiles[q - 1].has_next = true; tiles[q].run_beg = tiles[q - 1].run_beg; }
}

// the tiles: --bed-in-fname / -R regions, --targets "chr" or "chr:beg-end" (1-based inclusive as in samtools), else every contig
// `batch_of` (--merge-regions): the batch of every tile, from uvcio_plan_bed_batches over the BED lines; consecutive tiles of one batch
// are called as the ranges of one device region
// --coverage-out: the report's rows are added here in target order -- the BED lines in file order (every tile carries its line's row), or
// the windows of every called span (cov_spans: per contig the row of the span's first window)
// --family-stats-out: its rows are added the same way (fam_spans, Tile::fam_target)
// --fragment-profile-out: and so are its (frag_spans, Tile::frag_target)
std::vector<Tile> plan_tiles(Opts &o, uvcio_bam_t *bam0, const Geometry &G, std::vector<int64_t> *batch_of = nullptr, std::vector<CovSpan> *cov_spans = nullptr, std::vector<CovSpan> *fam_spans = nullptr,
                              std::vector<CovSpan> *frag_spans = nullptr) {
    const std::vector<std::string> &names = G.names; const std::vector<int64_t> &lens = G.lens; const int32_t nref = (int32_t)names.size();
    std::vector<Tile> tiles;
    const std::string bed_path = (!o.bed_in.empty() ? o.bed_in : o.bed);
    // Without --tile and without a BED file the regions are the ones the reference itself would hand to process_batch: one pass over the
    // alignments of the targets (as SamIter::iternext makes it, grouping.cpp:225-312) through uvcio_plan_regions -- cuts at contig changes, at
    // gaps of more than 200 bp and where the per-thread memory model says so (grouping.cpp:28-67: ~20-40 kb at 300x).  Every such region is
    // then processed exactly like a process_batch call (its own reference window, repeat tracks and BAQ sums from its own start, zerobased_pos
    // beg .. end inclusive), so the records equal the reference's also next to a cut.  --tile N trades that for long regions (faster on the
    // device; qualities within one unit next to a cut).
    const bool ref_cuts = (o.tile <= 0 && bed_path.empty());
    if (o.tile <= 0) o.tile = 1000000;
    // the planning pass is a stream: every 4 Mb window of alignments goes straight into the planner, nothing per alignment is kept
    uvcio_planner_t *planner = nullptr; int64_t n_planned = 0; const double tp = now();
    if (ref_cuts && uvcio_planner_open(&planner, lens.data(), nref, (o.threads > 0 ? o.threads : 8) /* the reference's -t default (CmdLineArgs.hpp:34): enters only where a batch of regions ends */, o.mem_per_thread)) die(uvcio_last_error());
    std::vector<int32_t> pl_tid, pl_pos, pl_end; std::vector<uint16_t> pl_flag;   // one window's columns
    auto take_cuts = [&]() { UvcRegionCut c[256]; int64_t k; while ((k = uvcio_planner_take(planner, c, 256)) > 0) for (int64_t q = 0; q < k; q++) tiles.push_back(Tile{ c[q].tid, names[(size_t)c[q].tid], c[q].beg, c[q].end, false, false, c[q].beg }); };
    int64_t cov_target = -1, fam_target = -1, call_target = -1, frag_target = -1;   // the report rows of the BED line being added
    if (o.callable || o.msi) o.call_contig_target.assign((size_t)nref, -1);
    // a target of --callable-out and --msi-out: both stores take the same targets in the same order, so one index names it in both
    auto add_span_target = [&](const char *chrom, int64_t beg, int64_t end, const char *name) {
        const int64_t tc = o.callable ? uvcio_callable_add_target(o.callable, chrom, beg, end, name) : -1, tm = o.msi ? uvcio_msi_add_target(o.msi, chrom, beg, end, name) : -1;
        if ((o.callable && tc < 0) || (o.msi && tm < 0)) die(uvcio_last_error());
        if (o.callable && o.msi && tc != tm) die("--callable-out and --msi-out disagree on a target's index (internal error)");
        o.call_target_span.emplace_back(beg, std::max(beg, end));
        return o.callable ? tc : tm;
    };
    auto add = [&](int32_t tid, int64_t beg, int64_t end) {
        // window mode of a report: the windows of this span become its targets, in order; the span keeps the row of the first
        auto window_targets = [&](const char *wopt, int64_t N, CovSpan &sp, auto add_target) {
            if (sp.first >= 0) die(std::string(wopt) + ": a contig is called twice (internal error)");
            sp.origin = beg;
            for_windows(beg, end, N, [&](int64_t, int64_t wb, int64_t we) {
                const int64_t row = add_target(wb, we);
                if (row < 0) die(uvcio_last_error());
                if (sp.first < 0) sp.first = row;
            });
        };
        const char *chrom = names[(size_t)tid].c_str();
        if (o.cov && cov_spans && o.report[R_COVERAGE].window > 0 && end > beg)
            window_targets("--coverage-window", o.report[R_COVERAGE].window, (*cov_spans)[(size_t)tid], [&](int64_t wb, int64_t we) { return uvcio_coverage_add_target(o.cov, chrom, wb, we, nullptr, we - wb); });
        if (o.fam && fam_spans && o.report[R_FAMSTATS].window > 0 && end > beg)
            window_targets("--family-stats-window", o.report[R_FAMSTATS].window, (*fam_spans)[(size_t)tid], [&](int64_t wb, int64_t we) { return uvcio_famstats_add_target(o.fam, chrom, wb, we, nullptr); });
        if (o.fragprof && frag_spans && o.report[R_FRAGPROF].window > 0 && end > beg)
            window_targets("--fragment-profile-window", o.report[R_FRAGPROF].window, (*frag_spans)[(size_t)tid], [&](int64_t wb, int64_t we) { return uvcio_fragprofile_add_target(o.fragprof, chrom, wb, we, nullptr); });
        if ((o.callable || o.msi) && bed_path.empty()) {   // --callable-out, --msi-out without a BED file: the called span of the contig is one target
            if (o.call_contig_target[(size_t)tid] >= 0) die("--callable-out, --msi-out: a contig is called twice (internal error)");
            call_target = o.call_contig_target[(size_t)tid] = add_span_target(names[(size_t)tid].c_str(), beg, end, nullptr);
        }
        if (!ref_cuts) { for (int64_t b = beg; b < end; b += o.tile) tiles.push_back(Tile{ tid, names[(size_t)tid], b, std::min(b + o.tile, end), false, false, b, cov_target, fam_target, call_target, frag_target }); return; }
        const int64_t W = 4000000;   // the planning pass reads the span window by window; an alignment is taken by the window it starts in (the first window also takes those that reach into it)
        for (int64_t wb = beg; wb < end; wb += W) {
            UvcBamBatch b;
            if (uvcio_bam_fetch(bam0, tid, wb, std::min(wb + W, end), &b)) die(uvcio_last_error());
            pl_tid.clear(); pl_pos.clear(); pl_end.clear(); pl_flag.clear();
            for (int64_t i = 0; i < b.n_alns; i++) if (b.pos[i] >= wb || wb == beg) { pl_tid.push_back(b.tid[i]); pl_pos.push_back(b.pos[i]); pl_end.push_back(b.endpos[i]); pl_flag.push_back(b.flag[i]); }
            if (uvcio_planner_feed(planner, pl_tid.data(), pl_pos.data(), pl_end.data(), pl_flag.data(), (int64_t)pl_tid.size())) die(uvcio_last_error());
            n_planned += (int64_t)pl_tid.size();
            take_cuts();
        }
    };
    if (!bed_path.empty()) {   // one region per BED line (0-based, half-open), cut into tiles; overrides --targets as in the reference
        FILE *fb = fopen(bed_path.c_str(), "r");
        if (!fb) die("cannot open " + bed_path);
        char line[4096], chrom[1024], bname[1024]; long long b = 0, e = 0;
        std::vector<int32_t> l_tid; std::vector<int64_t> l_beg, l_end;   // the lines as `add` sees them
        while (fgets(line, sizeof(line), fb)) {
            if (line[0] == '#' || !strncmp(line, "track", 5) || !strncmp(line, "browser", 7)) continue;
            int n_col = sscanf(line, "%1023s %lld %lld %1023s", chrom, &b, &e, bname);
            if (n_col < 3) continue;
            if (strchr(line, '\t')) {   // a tab-separated file: column 4 is everything up to the next tab, blanks included
                const char *p = line; for (int c = 0; c < 3 && p; c++) { p = strchr(p, '\t'); if (p) p++; }
                const size_t len = p ? std::min<size_t>(strcspn(p, "\t\r\n"), sizeof(bname) - 1) : 0;
                if (len > 0) { memcpy(bname, p, len); bname[len] = 0; n_col = 4; } else n_col = 3;
            }
            int32_t tid = -1;
            for (int32_t i = 0; i < nref; i++) if (names[(size_t)i] == chrom) tid = i;
            if (tid < 0) die(std::string("the BED file names a contig that is not in the BAM header: ") + chrom);
            if (o.cov) {   // one report row per BED line: its own numbers, column 4 as the name, the positions inside the contig as the length
                cov_target = uvcio_coverage_add_target(o.cov, chrom, b, e, n_col >= 4 ? bname : nullptr, std::max<long long>(0, std::min<long long>(e, lens[(size_t)tid]) - std::max<long long>(0, b)));
                if (cov_target < 0) die(uvcio_last_error());
            }
            if (o.fam) {   // one report row per BED line, its own numbers and column 4 as the name
                fam_target = uvcio_famstats_add_target(o.fam, chrom, b, e, n_col >= 4 ? bname : nullptr);
                if (fam_target < 0) die(uvcio_last_error());
            }
            if (o.fragprof) {   // one report row per BED line, its own numbers and column 4 as the name
                frag_target = uvcio_fragprofile_add_target(o.fragprof, chrom, b, e, n_col >= 4 ? bname : nullptr);
                if (frag_target < 0) die(uvcio_last_error());
            }
            if (o.callable || o.msi)   // one target per BED line: its positions inside the contig, column 4 as the name
                call_target = add_span_target(chrom, std::max<long long>(0, b), std::min<long long>(e, lens[(size_t)tid]), n_col >= 4 ? bname : nullptr);
            add(tid, std::max<long long>(0, b), std::min<long long>(e, lens[(size_t)tid]));
            l_tid.push_back(tid); l_beg.push_back(std::max<long long>(0, b)); l_end.push_back(std::min<long long>(e, lens[(size_t)tid]));
        }
        fclose(fb);
        if (batch_of && o.merge > 0) {   // one piece per tile: the planner cuts an over-long line exactly as `add` does
            std::vector<UvcBedPiece> pieces(tiles.size() + 1); int64_t np = 0;
            if (uvcio_plan_bed_batches(l_tid.data(), l_beg.data(), l_end.data(), (int64_t)l_tid.size(), o.merge, o.tile, pieces.data(), (int64_t)pieces.size(), &np)) die(uvcio_last_error());
            if (np != (int64_t)tiles.size()) die("--merge-regions: the batch planner and the tile list disagree (internal error)");
            batch_of->resize(tiles.size());
            for (size_t q = 0; q < tiles.size(); q++) {
                if (pieces[q].beg != tiles[q].beg || pieces[q].end != tiles[q].end) die("--merge-regions: the batch planner and the tile list disagree (internal error)");
                (*batch_of)[q] = pieces[q].batch;
            }
        }
    } else if (!o.targets.empty()) {
        std::string chrom = o.targets; int64_t beg = 0, end = -1;
        const size_t c = o.targets.rfind(':');
        if (c != std::string::npos && o.targets.find('-', c) != std::string::npos) {
            chrom = o.targets.substr(0, c);
            std::string rng = o.targets.substr(c + 1); rng.erase(std::remove(rng.begin(), rng.end(), ','), rng.end());
            beg = std::max<int64_t>(0, atoll(rng.c_str()) - 1); end = atoll(rng.substr(rng.find('-') + 1).c_str());
        }
        int32_t tid = -1;
        for (int32_t i = 0; i < nref; i++) if (names[(size_t)i] == chrom) tid = i;
        if (tid < 0) die("--targets names a contig that is not in the BAM header: " + chrom);
        add(tid, beg, end < 0 ? lens[(size_t)tid] : std::min(end, lens[(size_t)tid]));
    } else for (int32_t i = 0; i < nref; i++) add(i, 0, lens[(size_t)i]);
    if (ref_cuts) {
        if (uvcio_planner_finish(planner)) die(uvcio_last_error());
        take_cuts();
        uvcio_planner_close(planner); planner = nullptr;
        fprintf(stderr, "uvc1-mi355x: %zu regions from the reference's cuts over %lld alignments (planning pass %.2f s)\n", tiles.size(), (long long)n_planned, now() - tp);
    }
    // fixed tiles only: the reference's own regions each write both end points (main.cpp:608, 643)
    if (!ref_cuts) link_runs(tiles);
    return tiles;
}

// --shard i/n: the i-th of n contiguous runs of the list, balanced by index bytes + positions
std::vector<int32_t> plan_shard_of(const Opts &o, uvcio_bam_t *bam0, const std::vector<Tile> &tiles) {
    std::vector<int64_t> cost(tiles.size()); std::vector<int32_t> shard_of(tiles.size());
    for (size_t q = 0; q < tiles.size(); q++) cost[q] = uvcio_bam_region_bytes(bam0, tiles[q].tid, tiles[q].beg, tiles[q].end) + (tiles[q].end - tiles[q].beg) / 8 + 1;
    if (uvcio_plan_shards(cost.data(), (int64_t)cost.size(), o.n_shards, shard_of.data())) die(uvcio_last_error());
    return shard_of;
}

// parameters: the reference's defaults and the user's values (parse); AUTO / OTHER infer platform and read length from the first
// alignments that are seen (CmdLineArgs.cpp:34-111 reads the first 5000 records of the file; here: of the first tile that has any)
void infer_platform(Opts &o, uvcio_bam_t *bam0, const std::vector<Tile> &tiles) {
    int platform = UVC_PLATFORM_ILLUMINA, readlen = 150, maxmq = 0; bool seen = false;
    for (size_t ti = 0; ti < tiles.size() && !seen; ti++) {
        UvcBamBatch b;
        if (uvcio_bam_fetch(bam0, tiles[ti].tid, tiles[ti].beg, tiles[ti].end, &b)) die(uvcio_last_error());
        if (b.n_alns == 0) continue;
        seen = true;
        const int64_t m = std::min<int64_t>(b.n_alns, 5000);
        std::vector<int32_t> ql{ 150 }; uint64_t pe = 0, q20f = 0, q30f = 0, q30p = 0;
        for (int64_t i = 0; i < m; i++) {
            maxmq = std::max<int>(maxmq, b.mapq[i]); pe += (b.flag[i] & 1); ql.push_back(b.l_qseq[i]);
            for (int32_t q = 0; q < b.l_qseq[i]; q++) { const uint8_t bq = b.quals[b.seq_off[i] + q]; if (bq < 30) q30f++; else q30p++; if (bq < 20) q20f++; }
        }
        std::sort(ql.begin(), ql.end());
        readlen = ql[ql.size() / 2];
        const bool fix = ((int64_t)ql[ql.size() / 2] * 100 > (int64_t)ql.back() * 95);
        if (!(pe > 0 || 4 * (q30f - q20f) < q30p || (2 * (q30f - q20f) < q30p && fix))) platform = UVC_PLATFORM_IONTORRENT;
    }
    uvcgpu_params_apply_platform_ex(&o.P, o.sequencing_platform, platform, readlen, maxmq);
}

// ##fileDate / ##reference / ##variantCallerCommand as generate_vcf_header prints them (main.hpp:5788-5794, 5870-5874)
std::string vcf_header(const Opts &o, const std::string &cmd, const char *tsample, const char *const *cnames, const int64_t *lens, int32_t nref) {
    char date[80]; { time_t raw; time(&raw); strftime(date, sizeof(date), "%F %T", localtime(&raw)); }
    int64_t len = 0;
    uvcgpu_vcf_header_ex(&o.P, o.sample.c_str(), tsample, cnames, lens, nref, date, o.fasta.c_str(), cmd.c_str(), nullptr, 0, &len);
    std::string h((size_t)len, '\0');
    if (uvcgpu_vcf_header_ex(&o.P, o.sample.c_str(), tsample, cnames, lens, nref, date, o.fasta.c_str(), cmd.c_str(), &h[0], len, &len)) die(uvcgpu_last_error());
    return h;
}

// the region table of main.cpp:1415-1436 (--bed-out-fname): the shard manifest of the normal pass of a T/N pair
void write_region_table(const Opts &o, const std::vector<const Tile *> &tiles, const std::vector<int64_t> &tile_reads) {
    FILE *fo = fopen(o.bed_out.c_str(), "w");
    if (!fo) die("cannot create " + o.bed_out);
    for (size_t ti = 0; ti < tiles.size(); ti++)
        fprintf(fo, "%s\t%lld\t%lld\tBedLineFlag\t%d\tNumberOfReadsInThisInterval\t%lld\tNumberOfRefBasesInThisInterval\t%lld\tTier1regionIndex\t0\tTier2regionIndex\t%d\tTier3regionIndex\t%zu\n",
                tiles[ti]->chrom.c_str(), (long long)tiles[ti]->beg, (long long)tiles[ti]->end, tiles[ti]->continues ? 4 : 16, (long long)tile_reads[ti], (long long)(tiles[ti]->end - tiles[ti]->beg), o.shard, ti);
    fclose(fo);
}

// The side-effect switches of the readers (process-wide, after uvcgpu_init of the first device).
void reader_switches(const Opts &o) {
    // UVC1_PINNED=1: the workers' base / quality columns live in page-locked memory of the GPU library from here on, so that set_reads copies
    // them by DMA.  Off by default: on the boxes measured the files -> VCF rate did not move with it (scripts/bench_cli.py; the chain is not
    // bound by that copy) and it locks ~ 800 MB of host memory per worker.
    // --device-inflate (or UVC1_DEVICE_INFLATE=1): the inflate is ~half of the host's work per tile and the host's cores bound files -> VCF
    // (DESIGN.md 6b).  One device call per batch of blocks costs about as much for 500 blocks as for 8 000 (every block is a wave of its own):
    // the reader takes the compressed bytes of a whole tile as one batch.
    if (o.device_inflate || getenv("UVC1_DEVICE_INFLATE")) {
        const char *mb = getenv("UVC1_DEVICE_INFLATE_MIN");   // batches with fewer blocks stay on the host (tests: 1)
        uvcio_set_inflate(uvcgpu_bgzf_inflate, nullptr, mb ? atoi(mb) : 256);
        setenv("UVCIO_BATCH_BYTES", "402653184", 0);
    }
    if (getenv("UVC1_PINNED"))
        uvcio_set_column_allocator([](size_t n) -> void * { void *q = nullptr; return uvcgpu_host_alloc(&q, (int64_t)n) == 0 ? q : nullptr; }, [](void *q) { (void)uvcgpu_host_free(q); });
}

// ---- pair mode (--normal-bam): uvcTN.sh:27-50, 120-127 in one process ----
// The command line split as uvcTN.sh splits it: options before the first --tumor-params / --normal-params go to both sides, after one of
// them to that side only, until the other.  Side lists take PARAM / GROUP / MODE / INERT options; a CLI option there is refused.
struct PairArgs { bool pair = false, side_lists = false; std::string normal_bam, tumor_out; std::vector<std::string> shared, side[2]; };
// --family-stats-out, --fragment-profile-out (`opt`): the pieces of every tile (see FamPiece), in plan order, for the report's own targets
// (`target_of` of a tile) or windows of N bp
std::vector<std::vector<FamPiece>> plan_family_pieces(const char *opt, int64_t N, int64_t Tile::*target_of, const std::vector<Tile> &tiles, const std::vector<CovSpan> &spans, int32_t nref) {
    std::vector<std::vector<FamPiece>> plan(tiles.size());
    std::vector<int64_t> reach((size_t)nref, 0);   // per contig: the largest end of the pieces planned so far
    int64_t last_target = -1;
    for (size_t q = 0; q < tiles.size(); q++) {
        const Tile &t = tiles[q];
        for (int64_t b = t.beg; b < t.end;) {
            int64_t stop = t.end, target = t.*target_of;
            if (target < 0) {   // window mode
                const CovSpan &sp = spans[(size_t)t.tid];
                if (N <= 0 || sp.first < 0 || b < sp.origin) die(std::string(opt) + ": a tile outside the planned windows (internal error)");
                stop = std::min(t.end, (b / N + 1) * N); target = sp.first + (b / N - sp.origin / N);
            }
            plan[q].push_back(FamPiece{ b, stop, std::min(b, reach[(size_t)t.tid]), target == last_target ? UVC_FAMRANGE_CONTINUES : 0, target });
            reach[(size_t)t.tid] = std::max(reach[(size_t)t.tid], stop); last_target = target; b = stop;
        }
    }
    return plan;
}

PairArgs split_pair(int argc, char **argv) {
    PairArgs a; int sec = -1;   // -1 both sides, 0 tumor, 1 normal
    for (int i = 1; i < argc; i++) {
        const std::string t = argv[i];
        std::vector<std::string> &dst = (sec < 0 ? a.shared : a.side[sec]);
        if (t.empty() || t[0] != '-') {
            if (sec >= 0) die("'" + t + "' after " + (sec ? "--normal-params" : "--tumor-params") + ": a side list takes options only");
            dst.push_back(t); continue;
        }
        std::string name = t, val; bool inl = false;
        if (t.compare(0, 2, "--") == 0 && t.find('=') != std::string::npos) { name = t.substr(0, t.find('=')); val = t.substr(t.find('=') + 1); inl = true; }
        if (name == "--tumor-params" || name == "--normal-params") {
            if (inl) die(name + " takes no value");
            sec = (name == "--tumor-params" ? 0 : 1); a.side_lists = true; continue;
        }
        const OptRow *row = find_opt(name);
        if (row && row->cls == O_CLI && sec >= 0) die(name + " is a [CLI] option: it goes before --tumor-params / --normal-params (both sides)");
        if (name == "--normal-bam" || name == "--tumor-output") {
            if (!inl) { if (i + 1 >= argc) die("missing value of " + name); val = argv[++i]; }
            if (name == "--normal-bam") { a.normal_bam = val; a.pair = true; } else a.tumor_out = val;
            continue;
        }
        const bool takes_value = row ? !row->flag : (find_param(name) >= 0);   // an unknown option is refused by parse
        dst.push_back(t);
        if (takes_value && !inl && i + 1 < argc) dst.push_back(argv[++i]);
    }
    if (!a.pair) {
        if (a.side_lists) die("--tumor-params / --normal-params need --normal-bam");
        if (!a.tumor_out.empty()) die("--tumor-output needs --normal-bam");
        return a;
    }
    if (a.normal_bam.empty()) die("--normal-bam needs a path");
    for (size_t i = 0; i < a.shared.size(); i++) {
        const std::string &t = a.shared[i];
        const std::string name = t.substr(0, t.compare(0, 2, "--") == 0 ? t.find('=') : std::string::npos);
        if (name == "--tumor-vcf" || name == "--bed-in-fname") die(name + " cannot go with --normal-bam: pair mode hands the tumor records and regions over itself");
        if (name == "--repeat") die("--repeat cannot go with --normal-bam");
        int sub; const int rep = report_of(name, &sub);   // the options of a report: pair mode writes none
        if (rep >= 0) die(name + " cannot go with --normal-bam: pair mode has its own tile loop and writes no " + REPORTS[rep].pair_writes_no);
        if (name == "--force-sites") die("--force-sites cannot go with --normal-bam: the normal pass's gate is the tumor's rescue set");
        if (name == "--merge-regions" && atoll((t.find('=') != std::string::npos ? t.substr(t.find('=') + 1) : (i + 1 < a.shared.size() ? a.shared[i + 1] : std::string("0"))).c_str()) > 0)
            die("--merge-regions cannot go with --normal-bam: pair mode calls both samples region by region");
        if (t == ONLY_PRINT_VCF_HEADER) die(std::string(ONLY_PRINT_VCF_HEADER) + " cannot go with --normal-bam");
        const OptRow *row = (t[0] == '-' ? find_opt(name) : nullptr);
        if (t[0] == '-' && t.find('=') == std::string::npos && ((row && !row->flag) || (!row && find_param(name) >= 0))) i++;   // skip the value
    }
    if (a.tumor_out.empty()) die("--normal-bam needs --tumor-output (the tumor VCF)");
    return a;
}
Opts parse_side(const char *prog, const PairArgs &a, int side) {
    std::vector<std::string> v{ prog, "--tn-is-paired", "1" };   // uvcTN.sh passes it in front of the side's own options: a later value wins
    v.insert(v.end(), a.shared.begin(), a.shared.end());
    v.insert(v.end(), a.side[side].begin(), a.side[side].end());
    std::vector<char *> av; for (auto &x : v) av.push_back(&x[0]);
    return parse((int)av.size(), av.data());
}

// One process runs both passes of uvcTN.sh: the tumor tiles first in the work order, their record lines written in order to the tumor VCF
// and added in the same order to an in-memory store (uvcio_tumor_vcf_create), the normal tiles behind them.  A normal tile's tiles are
// those the normal pass of the two-pass flow reads back from the tumor's region table; it starts its tumor fetch once every tumor tile that
// reaches into its fetch range has been added.  With --shard i/n the process also runs the tumor tiles of other shards that its normal
// tiles' fetch ranges reach (the halo) and writes nothing of them.
int run_pair(Opts &ot, Opts &on, const std::string &cmd) {
    Opts *side[2] = { &ot, &on };
    const bool given_t = apply_given_platform(ot), given_n = apply_given_platform(on);
    if (ot.print_params && given_t && given_n) { print_params(ot, "tumor."); print_params(on, "normal."); return 0; }
    setenv("GPU_MAX_HW_QUEUES", "16", 0);   // as in the single-sample run (main)
    default_devices_and_threads(ot);
    on.devices = ot.devices; on.threads = ot.threads;
    Geometry gt, gn;
    uvcio_bam_t *tb0 = open_bam(ot.bam, gt), *nb0 = open_bam(on.bam, gn);
    // the tumor pass's tiles, all of them (every shard needs the whole list: ownership and the halo are properties of it)
    const std::vector<Tile> T = plan_tiles(ot, tb0, gt);
    // the normal pass's tiles: the tumor's region table read back as BED lines (--bed-in-fname), each line cut into --tile tiles (1 Mb
    // without), linked into runs where lines abut -- not the tumor's own tiles, whose reference cuts carry no `continues`
    if (on.tile <= 0) on.tile = 1000000;
    std::vector<int32_t> t2n(gt.names.size(), -1);
    for (size_t i = 0; i < gt.names.size(); i++) t2n[i] = gn.tid_of(gt.names[i]);
    std::vector<Tile> N; std::vector<size_t> n_src;
    for (size_t g = 0; g < T.size(); g++) {
        const int32_t tid = t2n[(size_t)T[g].tid];
        if (tid < 0) die("the normal BAM's header has no contig " + T[g].chrom);
        const int64_t e = std::min<int64_t>(T[g].end, gn.lens[(size_t)tid]);
        for (int64_t b = std::max<int64_t>(0, T[g].beg); b < e; b += on.tile) { N.push_back(Tile{ tid, gn.names[(size_t)tid], b, std::min(b + on.tile, e), false, false, b }); n_src.push_back(g); }
    }
    link_runs(N);
    // shards: a normal tile goes with the tumor tile it came from, so the shards' normal outputs concatenate to the one-process output
    std::vector<char> t_own(T.size(), 1), t_run, n_own(N.size(), 1);
    if (ot.n_shards > 1) {
        const std::vector<int32_t> shard_of = plan_shard_of(ot, tb0, T);
        for (size_t g = 0; g < T.size(); g++) t_own[g] = (shard_of[g] == ot.shard);
        for (size_t j = 0; j < N.size(); j++) n_own[j] = t_own[n_src[j]];
        if (ot.shard > 0) ot.no_header = on.no_header = true;
    }
    t_run = t_own;
    if (ot.n_shards > 1) {
        // the halo: a normal tile fetches its tumor records over [ext_beg, ext_end] (call_tile), its reads' extent plus MAX_STR_N_BASES.  Its
        // reads are those of [beg - MAX_INSERT_SIZE, end + MAX_INSERT_SIZE); the reads that cross the two outer ends of a contig's own tiles
        // bound every such range, so one query at each end gives the tumor tiles the shard needs
        std::map<int32_t, std::pair<int64_t, int64_t>> span;
        for (size_t j = 0; j < N.size(); j++) if (n_own[j]) {
            auto it = span.find(N[j].tid);
            if (it == span.end()) span[N[j].tid] = { N[j].beg, N[j].end };
            else { it->second.first = std::min(it->second.first, N[j].beg); it->second.second = std::max(it->second.second, N[j].end); }
        }
        for (auto &sp : span) {
            const int32_t tid = sp.first;
            const int64_t L = std::max<int64_t>(0, sp.second.first - MAX_INSERT_SIZE), R = sp.second.second + MAX_INSERT_SIZE;
            int64_t lo = L, hi = R;
            UvcBamBatch b;
            if (uvcio_bam_fetch(nb0, tid, L, L + 1, &b)) die(uvcio_last_error());
            for (int64_t i = 0; i < b.n_alns; i++) lo = std::min<int64_t>(lo, b.pos[i]);
            if (uvcio_bam_fetch(nb0, tid, R - 1, R, &b)) die(uvcio_last_error());
            for (int64_t i = 0; i < b.n_alns; i++) hi = std::max<int64_t>(hi, b.endpos[i]);
            lo -= MAX_STR_N_BASES; hi += MAX_STR_N_BASES;
            for (size_t g = 0; g < T.size(); g++) if (t2n[(size_t)T[g].tid] == tid && T[g].beg - 1 <= hi && T[g].end + 1 >= lo) t_run[g] = 1;   // a tile's records lie in [beg, end]
        }
    }
    std::vector<size_t> tj, nj;   // the jobs of this process: tumor tiles (own + halo), normal tiles (own), each in list order
    std::vector<const Tile *> t_mine, n_mine;
    for (size_t g = 0; g < T.size(); g++) { if (t_run[g]) tj.push_back(g); if (t_own[g]) t_mine.push_back(&T[g]); }
    for (size_t j = 0; j < N.size(); j++) if (n_own[j]) { nj.push_back(j); n_mine.push_back(&N[j]); }
    if (ot.n_shards > 1)
        fprintf(stderr, "uvc1-mi355x: shard %d of %d takes %zu of %zu tiles (tumor; %zu more as the halo of its normal tiles) and %zu of %zu normal tiles\n",
                ot.shard, ot.n_shards, t_mine.size(), T.size(), tj.size() - t_mine.size(), n_mine.size(), N.size());
    // each side's parameters from its own BAM (the two-pass flow's inference, per command line)
    auto own_tiles = [](const std::vector<const Tile *> &v) { std::vector<Tile> o; for (const Tile *t : v) o.push_back(*t); return o; };
    if (!given_t) infer_platform(ot, tb0, own_tiles(t_mine));
    if (!given_n) infer_platform(on, nb0, own_tiles(n_mine));
    uvcio_bam_close(tb0); uvcio_bam_close(nb0);
    if (ot.print_params) { print_params(ot, "tumor."); print_params(on, "normal."); return 0; }

    // the dependencies: for each normal tid, every tumor tile on it as [beg - 1, end + 1] (where its records lie) with its job index (-1: not run here)
    struct Dep { int64_t lo, hi; int64_t job; };
    std::vector<std::vector<Dep>> deps(gn.names.size()); std::vector<int64_t> dep_span(gn.names.size(), 0);
    { std::vector<int64_t> job_of(T.size(), -1); for (size_t k = 0; k < tj.size(); k++) job_of[tj[k]] = (int64_t)k;
      for (size_t g = 0; g < T.size(); g++) { const int32_t tid = t2n[(size_t)T[g].tid]; deps[(size_t)tid].push_back(Dep{ T[g].beg - 1, T[g].end + 1, job_of[g] }); dep_span[(size_t)tid] = std::max(dep_span[(size_t)tid], T[g].end - T[g].beg + 2); }
      for (auto &v : deps) std::sort(v.begin(), v.end(), [](const Dep &a, const Dep &b) { return a.lo < b.lo; }); }

    if (uvcgpu_init(ot.devices[0])) die(uvcgpu_last_error());
    reader_switches(ot);
    // --timing: the device memory this process holds at its peak, from hipMemGetInfo before the handles and after every tile
    std::map<int, int64_t> mem_base, mem_low;
    if (ot.timing) {
        for (int d : ot.devices) if (!mem_base.count(d)) { int64_t fr = 0; if (uvcgpu_init(d) || uvcgpu_device_memory(&fr, nullptr)) die(uvcgpu_last_error()); mem_base[d] = mem_low[d] = fr; }
        if (uvcgpu_init(ot.devices[0])) die(uvcgpu_last_error());
    }
    uvcio_tumor_vcf_t *store = nullptr;
    if (uvcio_tumor_vcf_create(&store, ot.sample.c_str(), gn.cnames.data(), (int32_t)gn.names.size(), on.tumor_format)) die(uvcio_last_error());
    uvcio_bgzf_writer_t *zw[2] = { nullptr, nullptr };
    for (int s = 0; s < 2; s++) if (uvcio_bgzf_write_open(&zw[s], side[s]->out.c_str(), 6)) die(uvcio_last_error());
    if (!ot.no_header) {
        const std::string ht = vcf_header(ot, cmd, nullptr, gt.cnames.data(), gt.lens.data(), (int32_t)gt.names.size());
        const std::string hn = vcf_header(on, cmd, on.tumor_format ? ot.sample.c_str() : nullptr, gn.cnames.data(), gn.lens.data(), (int32_t)gn.names.size());
        if (uvcio_bgzf_write(zw[0], ht.data(), (int64_t)ht.size()) || uvcio_bgzf_write(zw[1], hn.data(), (int64_t)hn.size())) die(uvcio_last_error());
    }
    const double t_start = now();
    const std::vector<size_t> *jobs[2] = { &tj, &nj };
    const std::vector<Tile> *tl[2] = { &T, &N };
    const Geometry *geo[2] = { &gt, &gn };
    std::vector<std::string> done[2] = { std::vector<std::string>(tj.size()), std::vector<std::string>(nj.size()) };
    std::vector<char> ready[2] = { std::vector<char>(tj.size(), 0), std::vector<char>(nj.size(), 0) };
    std::vector<int64_t> tile_reads(tj.size(), 0);
    std::mutex mu; std::condition_variable cv; std::atomic<size_t> next{ 0 };
    size_t written[2] = { 0, 0 };   // jobs each writer has taken (guarded by mu)
    size_t t_added = 0;             // tumor jobs whose lines are in the store (guarded by mu): always a prefix of tj
    const size_t n_jobs = tj.size() + nj.size();
    const int nthreads = (int)std::min<size_t>((size_t)ot.threads, std::max<size_t>(n_jobs, 1));
    const size_t max_ahead = (size_t)4 * (size_t)nthreads;
    // a normal tile's tumor records over [a, b] of `tid` are complete once every tumor tile that reaches into the range is in the store
    const std::function<void(int32_t, int64_t, int64_t)> tumor_ready = [&](int32_t tid, int64_t a, int64_t b) {
        const std::vector<Dep> &v = deps[(size_t)tid];
        int64_t need = -1;
        for (size_t q = (size_t)(std::upper_bound(v.begin(), v.end(), b, [](int64_t x, const Dep &d) { return x < d.lo; }) - v.begin()); q-- > 0;) {
            if (v[q].lo + dep_span[(size_t)tid] < a) break;
            if (v[q].hi < a) continue;
            if (v[q].job < 0) die("a normal tile reaches tumor tiles outside the shard's halo (internal error)");
            need = std::max(need, v[q].job);
        }
        std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return (int64_t)t_added > need; });
    };
    std::vector<Worker> workers[2] = { std::vector<Worker>((size_t)nthreads), std::vector<Worker>((size_t)nthreads) };
    std::vector<std::thread> th;
    for (int wi = 0; wi < nthreads; wi++) th.emplace_back([&, wi]() {
        const int dev = ot.devices[(size_t)wi % ot.devices.size()];
        if (uvcgpu_init(dev)) die(uvcgpu_last_error());   // binds this host thread to its device
        for (int s = 0; s < 2; s++) if (uvcio_bam_open(&workers[s][(size_t)wi].bam, side[s]->bam.c_str()) || uvcio_fasta_open(&workers[s][(size_t)wi].fa, side[s]->fasta.c_str())) die(uvcio_last_error());
        for (;;) {
            const size_t q = next.fetch_add(1);
            if (q >= n_jobs) break;
            const int s = (q < tj.size() ? 0 : 1); const size_t k = (s ? q - tj.size() : q);
            { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return k < written[s] + max_ahead; }); }   // bounded run-ahead of each writer
            Worker &w = workers[s][(size_t)wi];
            const Tile &t = (*tl[s])[(*jobs[s])[k]];
            std::string lines; int64_t nk = 0;
            call_tile(w, *side[s], side[s]->P, t, geo[s]->lens[(size_t)t.tid], s ? store : nullptr, lines, &nk, s ? &tumor_ready : nullptr);
            w.n_tiles++;
            int64_t fr = -1;
            if (ot.timing && uvcgpu_device_memory(&fr, nullptr)) die(uvcgpu_last_error());
            { std::lock_guard<std::mutex> g(mu); done[s][k].swap(lines); ready[s][k] = 1; if (!s) tile_reads[k] = nk; if (fr >= 0) mem_low[dev] = std::min(mem_low[dev], fr); }
            cv.notify_all();
        }
        for (int s = 0; s < 2; s++) { Worker &w = workers[s][(size_t)wi]; if (w.reg) uvcgpu_region_destroy(w.reg); uvcio_bam_close(w.bam); uvcio_fasta_close(w.fa); }
    });
    // two writers, each in the order of its list: the tumor one also feeds the store, in that same order (records of one key then keep
    // the order a tumor VCF holds them in)
    int64_t n_lines[2] = { 0, 0 }, n_pos[2] = { 0, 0 };
    auto writer = [&](int s) {
        for (size_t k = 0; k < jobs[s]->size(); k++) {
            std::string lines;
            { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return ready[s][k] != 0; }); lines.swap(done[s][k]); written[s] = k + 1; }
            cv.notify_all();
            const size_t ti = (*jobs[s])[k];
            if (s == 1 || t_own[ti]) {
                n_lines[s] += std::count(lines.begin(), lines.end(), '\n'); n_pos[s] += (*tl[s])[ti].end - (*tl[s])[ti].beg;
                if (!lines.empty() && uvcio_bgzf_write(zw[s], lines.data(), (int64_t)lines.size())) die(uvcio_last_error());
            }
            if (s == 0) {
                if (!lines.empty() && uvcio_tumor_vcf_add_lines(store, lines.data(), (int64_t)lines.size())) die(uvcio_last_error());
                { std::lock_guard<std::mutex> g(mu); t_added = k + 1; }
                cv.notify_all();
            }
        }
    };
    std::thread tumor_writer(writer, 0);
    writer(1);
    tumor_writer.join();
    for (auto &t : th) t.join();
    for (int s = 0; s < 2; s++) if (uvcio_bgzf_write_close(zw[s])) die(uvcio_last_error());
    const int64_t n_tumor_records = uvcio_tumor_vcf_n_records(store);
    uvcio_tumor_vcf_close(store);
    if (!ot.bed_out.empty()) {
        std::vector<int64_t> reads_mine;
        for (size_t k = 0; k < tj.size(); k++) if (t_own[tj[k]]) reads_mine.push_back(tile_reads[k]);
        write_region_table(ot, t_mine, reads_mine);
    }
    const double dt = now() - t_start;
    for (int s = 0; s < 2; s++)
        fprintf(stderr, "uvc1-mi355x: %s: %lld record lines from %zu tiles (%lld positions)\n", s ? "normal" : "tumor", (long long)n_lines[s], s ? n_mine.size() : t_mine.size(), (long long)n_pos[s]);
    fprintf(stderr, "uvc1-mi355x: %lld tumor records handed to the normal tiles in memory; both passes in %.2f s, %d tiles in flight on %zu device(s)\n",
            (long long)n_tumor_records, dt, nthreads, ot.devices.size());
    if (ot.timing) {
        for (int s = 0; s < 2; s++) {
            double f = 0, g = 0, r = 0, x2 = 0, k = 0, x = 0;
            for (auto &w : workers[s]) { f += w.t_fetch; g += w.t_group; r += w.t_region; x2 += w.t_reads; k += w.t_gpu; x += w.t_text; }
            fprintf(stderr, "  %s thread-seconds: fetch %.2f, digest+group %.2f, reference+region %.2f, set_reads %.2f, bq+accumulate+score %.2f, record text %.2f\n", s ? "normal" : "tumor", f, g, r, x2, k, x);
        }
        for (size_t wi = 0; wi < (size_t)nthreads; wi++) fprintf(stderr, "  worker %zu on device %d: %lld tumor tiles, %lld normal tiles\n", wi, ot.devices[wi % ot.devices.size()], (long long)workers[0][wi].n_tiles, (long long)workers[1][wi].n_tiles);
        if (ot.score_mem_mb > 0) for (int s = 0; s < 2; s++) {
            int64_t nc = 0, ns = 0; for (auto &w : workers[s]) { nc += w.n_chunks; ns += w.n_streamed; }
            fprintf(stderr, "  --score-mem-mb %lld, %s: %lld chunks in %lld scored tiles = %.2f chunks per tile\n", (long long)ot.score_mem_mb, s ? "normal" : "tumor", (long long)nc, (long long)ns, ns ? (double)nc / (double)ns : 0.0);
        }
        std::string m;
        for (auto &b : mem_base) { char buf[160]; snprintf(buf, sizeof(buf), "%sdevice %d %.2f GB", m.empty() ? "" : ", ", b.first, (b.second - mem_low[b.first]) / 1e9); m += buf; }
        fprintf(stderr, "  device memory at the peak (hipMemGetInfo, %d tiles in flight, a tumor and a normal region handle each): %s\n", nthreads, m.c_str());
    }
    return 0;
}
}   // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "--concat")) {   // bcftools concat -n (uvcTN.sh:100)
        std::vector<const char *> in; for (int i = 3; i < argc; i++) in.push_back(argv[i]);
        if (uvcio_bgzf_concat(argv[2], in.data(), (int32_t)in.size())) die(uvcio_last_error());
        return 0;
    }
    std::string cmd; for (int i = 0; i < argc; i++) { cmd += argv[i]; cmd += "  "; }   // ##variantCallerCommand (main.hpp:5870-5874)
    const PairArgs pa = split_pair(argc, argv);
    if (pa.pair) {
        Opts ot = parse_side(argv[0], pa, 0), on = parse_side(argv[0], pa, 1);
        ot.out = pa.tumor_out;
        if (ot.out == on.out) die("--tumor-output is the same file as -o");
        on.bam = pa.normal_bam;
        on.P.tumor_vcf_is_provided = 1;   // the normal pass of uvcTN.sh has --tumor-vcf
        on.bed_out.clear();               // the region table is the tumor pass's
        const size_t c = ot.sample.find(',');   // -s TUM,NOR; one name N gives N_T and N_N (uvcTN.sh:71-80)
        if (c != std::string::npos) { on.sample = ot.sample.substr(c + 1); ot.sample = ot.sample.substr(0, c); }
        else { on.sample = ot.sample + "_N"; ot.sample += "_T"; }
        return run_pair(ot, on, cmd);
    }
    Opts o = parse(argc, argv);
    UvcParams &P = o.P;
    const bool platform_given = apply_given_platform(o);
    if (o.bam == ONLY_PRINT_VCF_HEADER) {
        if (!platform_given) P.inferred_sequencing_platform = o.sequencing_platform;
        const std::string h = vcf_header(o, cmd, nullptr, nullptr, nullptr, 0);
        fwrite(h.data(), 1, h.size(), stdout);
        return 0;
    }
    if (o.print_params && platform_given) { print_params(o); return 0; }
    // Each region handle has three streams and a worker's copies should run under another worker's kernels: with the runtime's default of four
    // hardware queues the streams of different handles share queues, and a kernel then waits behind another handle's 10 ms copy (bench.py's
    // pcie_inclusive leg: 16.0 ms per tile with 4 queues, 13.5 with 16).  Read by the HIP runtime when it starts; an explicit setting wins.
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    default_devices_and_threads(o);
    // the readers of all tiles in flight share one pool of inflate / decode threads inside libuvcio (as many as this process has cores:
    // quota- and affinity-aware, uvc_cpus.h); UVCIO_THREADS overrides
    Geometry G;
    uvcio_bam_t *bam0 = open_bam(o.bam, G);
    const int32_t nref = (int32_t)G.names.size();
    std::vector<int64_t> batch_of;   // --merge-regions: the batch of every tile (else empty: every tile is its own job)
    std::vector<CovSpan> cov_spans((size_t)nref);
    // the stores of the reports that are asked for; --print-params plans the tiles without them
    auto wanted = [&](ReportId r) { return !o.print_params && !o.report[r].path.empty(); };
    auto names_of = [](const char *(*name_of)(int32_t), int32_t n) { std::vector<const char *> v; for (int32_t i = 0; i < n; i++) v.push_back(name_of(i)); return v; };   // the library's names of a store's columns
    const std::vector<const char *> mnames = names_of(uvcgpu_coverage_measure_name, UVC_NCOV);   // the depths of --coverage-out and --callable-out
    if (wanted(R_COVERAGE) && uvcio_coverage_open(&o.cov, mnames.data(), UVC_NCOV, o.coverage_thr.data(), (int32_t)o.coverage_thr.size())) die(uvcio_last_error());
    if (wanted(R_ERRPROF) && uvcio_errprofile_open(&o.errprof, names_of(uvcgpu_error_level_name, UVC_NERRLEVEL).data(), UVC_NERRLEVEL, o.errprof_req.min_depth, o.errprof_req.max_alt_permille)) die(uvcio_last_error());
    if (wanted(R_CALLABLE) && uvcio_callable_open(&o.callable, mnames.data(), UVC_NCOV, o.call_req.min_depth, o.call_req.max_aDP, names_of(uvcgpu_callable_bit_name, UVC_NCALLBIT).data(), UVC_NCALLBIT)) die(uvcio_last_error());
    if (wanted(R_MSI) && uvcio_msi_open(&o.msi, o.msi_req.min_tracklen, o.msi_req.min_units, o.msi_req.max_unitlen, o.msi_min_depth, o.msi_unstable_permille)) die(uvcio_last_error());
    if (wanted(R_READPROF) && uvcio_readprofile_open(&o.readprof, names_of(uvcgpu_read_class_name, UVC_READPROF_NCLASS).data(), o.readprof_req.min_mapq, o.readprof_req.min_depth, o.readprof_req.max_alt_permille)) die(uvcio_last_error());
    std::vector<CovSpan> fam_spans((size_t)nref);
    if (wanted(R_FAMSTATS) && uvcio_famstats_open(&o.fam)) die(uvcio_last_error());
    if (wanted(R_FAMCONC) && uvcio_famconcord_open(&o.famconc)) die(uvcio_last_error());
    std::vector<CovSpan> frag_spans((size_t)nref);
    if (wanted(R_FRAGPROF) && uvcio_fragprofile_open(&o.fragprof, o.fragprof_req.min_mapq, o.fragprof_req.short_lo, o.fragprof_req.short_hi, o.fragprof_req.long_lo, o.fragprof_req.long_hi)) die(uvcio_last_error());
    if (wanted(R_CLIPSITES) && uvcio_clipsites_open(&o.clipsites, o.clipsites_req.min_mapq, o.clipsites_req.min_clip, o.clipsites_req.min_reads, o.clipsites_reads)) die(uvcio_last_error());
    if (o.clipsites && o.clipsites_junctions && uvcio_clipsites_set_junctions(o.clipsites, o.clipjunc_req.min_votes, o.clipjunc_req.min_len, o.clipjunc_req.max_mismatch, o.clipjunc_req.max_dist, o.clipjunc_req.mate_slop)) die(uvcio_last_error());
    if (o.clipsites && o.clipsites_mates && uvcio_clipsites_set_mates(o.clipsites, o.clipmates_req.window, o.clipmates_req.overhang, o.clipmates_req.min_dist, o.clipmates_req.max_gap, o.clipmates_req.min_pairs, G.cnames.data(), nref))
        die(uvcio_last_error());
    if (wanted(R_SITEREADS)) {   // the listed sites, each with its reference base: a site that no tile owns keeps its S line of zeros
        uvcio_sites_t *list = nullptr; uvcio_fasta_t *fa = nullptr;
        if (uvcio_sites_open(&list, o.sitereads_sites.c_str(), G.cnames.data(), nref)) die("--site-reads-sites: " + std::string(uvcio_last_error()));
        fprintf(stderr, "uvc1-mi355x: %lld sites from %s\n", (long long)uvcio_sites_count(list), o.sitereads_sites.c_str());
        if (uvcio_sitereads_open(&o.sitereads, names_of(uvcgpu_site_read_kind_name, UVC_SITEREAD_NKIND).data(), names_of(uvcgpu_read_class_name, UVC_READPROF_NCLASS).data(), o.sitereads_req.min_mapq, o.sitereads_req.alt_only)
            || uvcio_fasta_open(&fa, o.fasta.c_str())) die(uvcio_last_error());
        for (int32_t tid = 0; tid < nref; tid++) {
            const int32_t *s = nullptr; int64_t n = 0;
            if (uvcio_sites_fetch(list, tid, 0, (int64_t)INT32_MAX + 1, &s, &n)) die(uvcio_last_error());
            std::vector<int32_t> pos((size_t)n); std::string ref((size_t)n, '.');
            for (int64_t i = 0; i < n; i++) {
                pos[(size_t)i] = s[i] - 1;
                if (s[i] <= G.lens[(size_t)tid] && uvcio_fasta_fetch(fa, G.cnames[(size_t)tid], s[i] - 1, s[i], &ref[(size_t)i])) die(uvcio_last_error());
            }
            if (n > 0 && uvcio_sitereads_add(o.sitereads, tid, G.cnames[(size_t)tid], pos.data(), ref.data(), n, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) die(uvcio_last_error());
        }
        uvcio_fasta_close(fa);
        o.sitereads_list = list;
    }
    std::vector<Tile> tiles = plan_tiles(o, bam0, G, &batch_of, &cov_spans, &fam_spans, &frag_spans);
    std::vector<std::vector<FamPiece>> fam_plan, frag_plan;
    if (o.fam) fam_plan = plan_family_pieces(REPORTS[R_FAMSTATS].out, o.report[R_FAMSTATS].window, &Tile::fam_target, tiles, fam_spans, nref);
    if (o.fragprof) frag_plan = plan_family_pieces(REPORTS[R_FRAGPROF].out, o.report[R_FRAGPROF].window, &Tile::frag_target, tiles, frag_spans, nref);
    if (o.n_shards > 1) {
        std::vector<int32_t> shard_of = plan_shard_of(o, bam0, tiles);
        if (!batch_of.empty()) {   // balanced over batches: a batch is one region and goes to one shard, at the sum of its tiles' costs
            std::vector<int64_t> cost; std::vector<int32_t> of_batch;
            for (size_t q = 0; q < tiles.size(); q++) {
                const int64_t c = uvcio_bam_region_bytes(bam0, tiles[q].tid, tiles[q].beg, tiles[q].end) + (tiles[q].end - tiles[q].beg) / 8 + 1;
                if (q > 0 && batch_of[q] == batch_of[q - 1]) cost.back() += c; else cost.push_back(c);
            }
            of_batch.resize(cost.size());
            if (uvcio_plan_shards(cost.data(), (int64_t)cost.size(), o.n_shards, of_batch.data())) die(uvcio_last_error());
            for (size_t q = 0, bi = 0; q < tiles.size(); q++) { if (q > 0 && batch_of[q] != batch_of[q - 1]) bi++; shard_of[q] = of_batch[bi]; }
        }
        std::vector<Tile> mine; std::vector<int64_t> mine_batch;
        for (size_t q = 0; q < tiles.size(); q++) if (shard_of[q] == o.shard) { mine.push_back(tiles[q]); if (!batch_of.empty()) mine_batch.push_back(batch_of[q]); }
        fprintf(stderr, "uvc1-mi355x: shard %d of %d takes %zu of %zu tiles\n", o.shard, o.n_shards, mine.size(), tiles.size());
        tiles.swap(mine); batch_of.swap(mine_batch);
        if (o.shard > 0) o.no_header = true;
    }
    const size_t tiles_per_pass = tiles.size();
    for (int rep = 1; rep < o.repeat; rep++) for (size_t q = 0; q < tiles_per_pass; q++) { tiles.push_back(tiles[q]); if (!batch_of.empty()) batch_of.push_back(batch_of[q] + (int64_t)rep * ((int64_t)tiles_per_pass + 1)); }
    // a job = what one call_tile takes: a tile, or with --merge-regions the consecutive tiles of one batch
    std::vector<std::pair<size_t, size_t>> jobs;   // first tile, number of tiles
    for (size_t q = 0; q < tiles.size(); q++) {
        if (!batch_of.empty() && q > 0 && batch_of[q] == batch_of[q - 1]) jobs.back().second++; else jobs.emplace_back(q, 1);
    }
    const bool merging = !batch_of.empty();
    if (merging) fprintf(stderr, "uvc1-mi355x: --merge-regions %lld: %zu BED lines in %zu regions\n", (long long)o.merge, tiles_per_pass, jobs.size() / (size_t)o.repeat);
    if (!platform_given) infer_platform(o, bam0, tiles);
    uvcio_bam_close(bam0);
    if (o.print_params) { print_params(o); return 0; }
    uvcio_sites_t *sites = nullptr;
    if (!o.force_sites.empty()) {
        if (uvcio_sites_open(&sites, o.force_sites.c_str(), G.cnames.data(), nref)) die("--force-sites: " + std::string(uvcio_last_error()));
        fprintf(stderr, "uvc1-mi355x: %lld force-output sites from %s\n", (long long)uvcio_sites_count(sites), o.force_sites.c_str());
        o.sites = sites;
    }
    // a report path that cannot be written fails here -- before a device is opened -- not behind the last tile
    for (int r = 0; r < N_REPORTS; r++) if (!o.report[r].path.empty()) probe_create(REPORTS[r].out, o.report[r].path);
    if (uvcgpu_init(o.devices[0])) die(uvcgpu_last_error());
    reader_switches(o);
    // T/N: the tumor pass's records (rescue_variants_from_vcf, main.cpp:183-398)
    uvcio_tumor_vcf_t *tvcf = nullptr;
    if (!o.tumor_vcf.empty()) {
        if (uvcio_tumor_vcf_open(&tvcf, o.tumor_vcf.c_str(), G.cnames.data(), nref, o.tumor_format)) die(uvcio_last_error());
        fprintf(stderr, "uvc1-mi355x: %lld tumor records from %s\n", (long long)uvcio_tumor_vcf_n_records(tvcf), o.tumor_vcf.c_str());
    }

    // output: header, then the lines of every tile in tile order
    uvcio_bgzf_writer_t *zw = nullptr;
    if (uvcio_bgzf_write_open(&zw, o.out.c_str(), 6)) die(uvcio_last_error());
    if (!o.no_header) {
        const std::string h = vcf_header(o, cmd, (tvcf && o.tumor_format) ? uvcio_tumor_vcf_sample_name(tvcf) : nullptr, G.cnames.data(), G.lens.data(), nref);
        if (uvcio_bgzf_write(zw, h.data(), (int64_t)h.size())) die(uvcio_last_error());
    }
    const double t_start = now();
    std::vector<std::string> done(jobs.size()); std::vector<char> ready(jobs.size(), 0); std::vector<int64_t> tile_reads(tiles.size(), 0);
    std::mutex mu; std::condition_variable cv; std::atomic<size_t> next{ 0 };
    size_t written = 0;   // tiles the writer has taken (guarded by mu)
    const int nthreads = (int)std::min<size_t>((size_t)o.threads, std::max<size_t>(jobs.size(), 1));
    const size_t max_ahead = (size_t)4 * (size_t)nthreads;
    std::vector<Worker> workers((size_t)nthreads);
    std::vector<std::thread> th;
    for (int wi = 0; wi < nthreads; wi++) th.emplace_back([&, wi]() {
        Worker &w = workers[(size_t)wi];
        if (uvcgpu_init(o.devices[(size_t)wi % o.devices.size()])) die(uvcgpu_last_error());   // binds this host thread to its device
        if (uvcio_bam_open(&w.bam, o.bam.c_str()) || uvcio_fasta_open(&w.fa, o.fasta.c_str())) die(uvcio_last_error());
        for (;;) {
            const size_t ji = next.fetch_add(1);
            if (ji >= jobs.size()) break;
            const size_t ti = jobs[ji].first, nt = jobs[ji].second;
            // bounded run-ahead: finished tiles wait in `done` for the in-order writer; a worker does not start a tile more than
            // 4 * threads in front of it, so a slow early tile cannot make the rest of the genome pile up in memory
            { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return ji < written + max_ahead; }); }
            std::string lines; std::vector<int64_t> nk(nt, 0);
            call_tile(w, o, P, tiles[ti], G.lens[(size_t)tiles[ti].tid], tvcf, lines, nk.data(), nullptr, merging ? nt : 0, &cov_spans[(size_t)tiles[ti].tid], o.fam ? &fam_plan[ti] : nullptr, o.fragprof ? &frag_plan[ti] : nullptr);
            w.n_tiles++;
            { std::lock_guard<std::mutex> g(mu); done[ji].swap(lines); ready[ji] = 1; for (size_t q = 0; q < nt; q++) tile_reads[ti + q] = nk[q]; }
            cv.notify_all();
        }
        if (w.reg) uvcgpu_region_destroy(w.reg);
        uvcio_bam_close(w.bam); uvcio_fasta_close(w.fa);
    });
    int64_t n_lines = 0, n_pos = 0; double t_first_pass = 0; int64_t pos_first_pass = 0;
    for (size_t ji = 0; ji < jobs.size(); ji++) {
        if (jobs[ji].first == tiles_per_pass) { t_first_pass = now() - t_start; pos_first_pass = n_pos; }
        std::string lines;
        { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return ready[ji] != 0; }); lines.swap(done[ji]); written = ji + 1; }
        cv.notify_all();
        n_lines += std::count(lines.begin(), lines.end(), '\n');
        for (size_t q = 0; q < jobs[ji].second; q++) n_pos += tiles[jobs[ji].first + q].end - tiles[jobs[ji].first + q].beg;
        if (!lines.empty() && uvcio_bgzf_write(zw, lines.data(), (int64_t)lines.size())) die(uvcio_last_error());
    }
    for (auto &t : th) t.join();
    if (uvcio_bgzf_write_close(zw)) die(uvcio_last_error());
    // every tile has reported.  The stores write in target order whichever worker finished first (callable: sorted, filled and joined per
    // target); sums do not depend on the order
    auto path = [&](ReportId r) { return o.report[r].path.c_str(); };
    auto finish = [](ReportId r, int rc) { if (rc) die(std::string(REPORTS[r].out) + ": " + uvcio_last_error()); };
    if (o.cov) { finish(R_COVERAGE, uvcio_coverage_write(o.cov, path(R_COVERAGE))); uvcio_coverage_close(o.cov); }
    if (o.fam) { finish(R_FAMSTATS, uvcio_famstats_write(o.fam, path(R_FAMSTATS))); uvcio_famstats_close(o.fam); }
    if (o.callable) {
        if (o.timing) fprintf(stderr, "uvc1-mi355x: --callable-out holds %lld runs\n", (long long)uvcio_callable_n_runs(o.callable));
        finish(R_CALLABLE, uvcio_callable_write(o.callable, path(R_CALLABLE))); uvcio_callable_close(o.callable);
    }
    if (o.msi) {
        if (o.timing) fprintf(stderr, "uvc1-mi355x: --msi-out holds %lld loci\n", (long long)uvcio_msi_n_loci(o.msi));
        finish(R_MSI, uvcio_msi_write(o.msi, path(R_MSI))); uvcio_msi_close(o.msi);
    }
    if (o.errprof) { finish(R_ERRPROF, uvcio_errprofile_write(o.errprof, path(R_ERRPROF))); uvcio_errprofile_close(o.errprof); }
    if (o.famconc) { finish(R_FAMCONC, uvcio_famconcord_write(o.famconc, path(R_FAMCONC))); uvcio_famconcord_close(o.famconc); }
    if (o.readprof) { finish(R_READPROF, uvcio_readprofile_write(o.readprof, path(R_READPROF))); uvcio_readprofile_close(o.readprof); }
    if (o.fragprof) { finish(R_FRAGPROF, uvcio_fragprofile_write(o.fragprof, path(R_FRAGPROF))); uvcio_fragprofile_close(o.fragprof); }
    if (o.sitereads) { finish(R_SITEREADS, uvcio_sitereads_write(o.sitereads, path(R_SITEREADS))); uvcio_sitereads_close(o.sitereads); uvcio_sites_close(o.sitereads_list); }
    if (o.clipsites) { finish(R_CLIPSITES, uvcio_clipsites_write(o.clipsites, path(R_CLIPSITES))); uvcio_clipsites_close(o.clipsites); }
    if (tvcf) uvcio_tumor_vcf_close(tvcf);
    if (sites) uvcio_sites_close(sites);
    if (!o.bed_out.empty()) {
        std::vector<const Tile *> pass; for (size_t ti = 0; ti < tiles_per_pass; ti++) pass.push_back(&tiles[ti]);
        write_region_table(o, pass, tile_reads);
    }
    const double dt = now() - t_start;
    fprintf(stderr, "uvc1-mi355x: %lld record lines from %zu tiles (%lld positions) in %.2f s = %.2f M positions/s, %d tiles in flight on %zu device(s)\n",
            (long long)n_lines, tiles.size(), (long long)n_pos, dt, n_pos / dt / 1e6, nthreads, o.devices.size());
    if (o.repeat > 1) fprintf(stderr, "  passes 2..%d (steady state): %.2f M positions/s\n", o.repeat, (n_pos - pos_first_pass) / (dt - t_first_pass) / 1e6);
    if (o.timing) {
        double f = 0, g = 0, r = 0, s = 0, k = 0, x = 0;
        for (auto &w : workers) { f += w.t_fetch; g += w.t_group; r += w.t_region; s += w.t_reads; k += w.t_gpu; x += w.t_text; }
        fprintf(stderr, "  thread-seconds: fetch %.2f, digest+group %.2f, reference+region %.2f, set_reads %.2f, bq+accumulate+score %.2f, record text %.2f\n", f, g, r, s, k, x);
        for (size_t wi = 0; wi < workers.size(); wi++) fprintf(stderr, "  worker %zu on device %d: %lld tiles\n", wi, o.devices[wi % o.devices.size()], (long long)workers[wi].n_tiles);
        if (o.score_mem_mb > 0) {
            int64_t nc = 0, ns = 0; for (auto &w : workers) { nc += w.n_chunks; ns += w.n_streamed; }
            fprintf(stderr, "  --score-mem-mb %lld: %lld records per chunk, %lld chunks in %lld scored tiles = %.2f chunks per tile\n", (long long)o.score_mem_mb,
                    (long long)std::max<int64_t>(1, (o.score_mem_mb << 20) / uvcgpu_score_stream_bytes_per_record()), (long long)nc, (long long)ns, ns ? (double)nc / (double)ns : 0.0);
        }
    }
    return 0;
}
