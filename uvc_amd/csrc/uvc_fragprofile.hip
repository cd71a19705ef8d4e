// uvc_fragprofile.hip -- uvcgpu_region_fragment_profile: template lengths and reference end motifs of the fragments and families of ranges
// (the definitions are in uvcgpu.h).  Nothing here reads the planes: the inputs are the per-alignment columns (pos, endpos,
// frag, flag, mapq), RegionDev::frags / fss and RegionDev::refsym.
//
// Stage one, the spans of every fragment (k_fp_span).  As in k_famstat_span the work is split by alignment, never by fragment: a lane takes
// one alignment, the alignments of a fragment are consecutive, and a wave folds each run of equal fragment indices among its lanes with a
// segmented butterfly over { loF, hiF, loR, hiR } (an alignment that is not counted brings the empty span).  The head lane of a run merges
// it into the fragment's 16-byte record with atomicMin / atomicMax: a fragment of two alignments costs one merge, one of 130 three or four.
//
// Stage two, the fragments (k_fp_frag).  A lane takes a fragment: its kind from the record, its span into the template span of its
// family-strand unit where it is a pair (the fragments of a unit are consecutive: folded in the wave first), its first range by binary
// search on pos_end and the walk forward while it overlaps.  A block keeps a private copy of the profile row in LDS and the TARGET rows
// of a window of FP_WIN consecutive ranges, as k_famstat_bin does; adds outside the window go to the global rows.  An amplicon pile puts a
// whole wave on one LEN word: the lanes of a wave merge equal keys before the LDS add.
//
// Stage three, the families (k_fp_fam), a launch of its own because the unit templates must be complete.  A lane takes a unit; the unit
// that makes the family's record (k_famstat_bin's rule) joins its partner and bins by the same walk.
//
// Width of the LDS words.  The profile copy is 32 bits a word: a block bins at most 256 * FP_STEPS objects and every object adds at most 2
// (its two ends) to a word.  len_sum is a sum of lengths, not a count, so the block's len_sum and the window's TARGET rows are 64-bit
// words.  A block adds its non-zero words with 64-bit vector atomics: the profile into one of FP_SHARDS copies that k_fp_fold sums, the
// window into the result rows.  Integer adds only: their order does not show, the result is the same bits from call to call.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
enum {
#define UVC_FRAGPROF(name, first, words) FPROW_##name,
#include "uvc_fragprofile.def"
#undef UVC_FRAGPROF
    FPROW_N
};
static_assert(FPROW_N == UVC_NFRAGPROF, "include/uvc_fragprofile.def and UvcFragProfSection of uvcgpu.h list the same sections");
#define UVC_FRAGPROF(name, first, words) static_assert((int)FPROW_##name == (int)UVC_FRAGPROF_##name, "uvc_fragprofile.def order = UvcFragProfSection order");
#include "uvc_fragprofile.def"
#undef UVC_FRAGPROF
constexpr UvcSection FP_SECTIONS[UVC_NFRAGPROF] = {
#define UVC_FRAGPROF(name, first, words) { #name, first, words },
#include "uvc_fragprofile.def"
#undef UVC_FRAGPROF
};
static_assert(uvc_sections_tile(FP_SECTIONS, UVC_FRAGPROF_ROW), "the sections of uvc_fragprofile.def tile the row");
static_assert(FP_SECTIONS[UVC_FRAGPROF_LEN].first == UVC_FRAGPROF_LEN_BINS && FP_SECTIONS[UVC_FRAGPROF_LEN].words == UVC_FRAGPROF_NLEN
              && FP_SECTIONS[UVC_FRAGPROF_FAMLEN].first == UVC_FRAGPROF_FAMLEN_BINS && FP_SECTIONS[UVC_FRAGPROF_FAMLEN].words == UVC_FRAGPROF_NLEN
              && FP_SECTIONS[UVC_FRAGPROF_MOTIF].first == UVC_FRAGPROF_MOTIF_BINS && FP_SECTIONS[UVC_FRAGPROF_MOTIF].words == UVC_FRAGPROF_NMOTIF
              && FP_SECTIONS[UVC_FRAGPROF_LEN].first == UVC_FRAGPROF_NCOUNTER && FP_SECTIONS[UVC_FRAGPROF_reserved].first == UVC_FRAGPROF_TARGET_ROW - 1,
              "the block offsets of uvcgpu.h are those of uvc_fragprofile.def");
// a counter's section id is its word, in a TARGET row and in the profile row
static_assert(FP_SECTIONS[UVC_FRAGPROF_pairs].first == UVC_FRAGPROF_pairs && FP_SECTIONS[UVC_FRAGPROF_families].first == UVC_FRAGPROF_families
              && FP_SECTIONS[UVC_FRAGPROF_ends_no_ref].first == UVC_FRAGPROF_ends_no_ref && UVC_FRAGPROF_others == UVC_FRAGPROF_pairs + 1 && UVC_FRAGPROF_singles == UVC_FRAGPROF_pairs + 2,
              "the counters are one word each, the three kinds in a row");
static_assert(sizeof(UvcFamilyRange) == 16, "the host uploads the caller's ranges as 16-byte rows");
static_assert(UVC_BASE_A == 0 && UVC_BASE_C == 1 && UVC_BASE_G == 2 && UVC_BASE_T == 3, "the complement of a reference symbol is 3 - code");

#define FP_WIN 256      // ranges whose TARGET rows a block keeps in LDS: 256 * 8 * 8 = 16 384 B beside the 9 280 B of the profile copy
#define FP_STEPS 4      // objects per lane: a block of 256 lanes bins 1 024 fragments or units into one window before it flushes
#define FP_SHARDS 16    // copies of the profile row the blocks add into
#define FP_TROW UVC_FRAGPROF_TARGET_ROW
enum { FP_PAIR = 0, FP_OTHER = 1, FP_SINGLE = 2 };   // a fragment's kind = its counter; in k_fp_fam: a sized family without / with pairs on both strands

// every span starts empty, every word of the result and of the copies at 0
__global__ void __launch_bounds__(256) k_fp_init(UvcFragSpan *fspan, int n_frags, UvcUnitSpan *uspan, int n_fs, unsigned long long *out, long long n_out, unsigned long long *parts, long long n_parts) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_frags) fspan[i] = UvcFragSpan{ INT_MAX, INT_MIN, INT_MAX, INT_MIN };
    if (i < n_fs) uspan[i] = UvcUnitSpan{ INT_MAX, INT_MIN };
    if (i < n_out) out[i] = 0;
    if (i < n_parts) parts[i] = 0;
}

__global__ void __launch_bounds__(256) k_fp_span(const int32_t *pos, const int32_t *endpos, const int32_t *frag_of, const uint16_t *flag, const uint8_t *mapq, int n_alns, int n_frags, int min_mapq,
                                                 UvcFragSpan *fspan) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int g = -1, lo[2] = { INT_MAX, INT_MAX }, hi[2] = { INT_MIN, INT_MIN };   // [0] forward, [1] reverse
    if (i < n_alns) {
        g = frag_of[i];
        const int fl = (int)flag[i];
        if ((int)mapq[i] >= min_mapq && !(fl & 0x904)) {   // counted: not unmapped, secondary or supplementary
            const int rev = (fl & 0x10) ? 1 : 0;
            lo[rev] = pos[i]; hi[rev] = endpos[i];
        }
    }
    if (g < 0 || g >= n_frags) g = -1;   // (no such fragment: set_reads refuses these reads)
    seg_fold_minmax<2>(g, lo, hi);   // the run of a fragment among the lanes, over two (min, max) pairs
    if (seg_head(g) && g >= 0) {
        if (lo[0] != INT_MAX) { atomicMin(&fspan[g].loF, lo[0]); atomicMax(&fspan[g].hiF, hi[0]); }
        if (lo[1] != INT_MAX) { atomicMin(&fspan[g].loR, lo[1]); atomicMax(&fspan[g].hiR, hi[1]); }
    }
}

struct FpObj { int lo, hi, first, kind; };   // [lo, hi); first: the first range it overlaps, n_ranges where there is none; kind < 0: the lane has no object

// what a block keeps: the profile copy, the TARGET rows of its window and its len_sum
struct FpBlock { unsigned prof[UVC_FRAGPROF_ROW]; UvcRowWindow<unsigned long long, FP_WIN, FP_TROW> win; unsigned long long len_sum; };
DEV void fp_block_begin(FpBlock &B, int tid) {
    for (int j = tid; j < UVC_FRAGPROF_ROW; j += 256) B.prof[j] = 0;
    B.win.begin(tid);
    if (tid == 0) B.len_sum = 0;
    __syncthreads();
}
DEV void fp_block_end(FpBlock &B, int tid, int w0, int n_ranges, unsigned long long *rows, unsigned long long *part_row) {
    __syncthreads();
    for (int j = tid; j < UVC_FRAGPROF_ROW; j += 256) { const unsigned v = B.prof[j]; if (v) atomicAdd(part_row + j, (unsigned long long)v); }
    if (tid == 0 && B.len_sum) atomicAdd(part_row + UVC_FRAGPROF_len_sum, B.len_sum);
    B.win.flush(tid, w0, n_ranges, rows);
}
// one 5' end of a pair in the profile: x = the region offset of its first reference base (left end) or one behind its last (right end)
DEV void fp_end(const RegionDev &R, long long x, bool right, bool on, unsigned *prof, int lane) {
    const long long n = R.npos - 1;   // positions that hold a reference base
    const bool usable = right ? (x - 4 >= 0 && x <= n) : (x >= 0 && x + 4 <= n);
    int key = 0; bool acgt = true;
    if (on && usable) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = (int)R.refsym[right ? x - 1 - k : x + k];
            acgt = acgt && s <= UVC_BASE_T;
            key = key * 4 + ((right ? 3 - s : s) & 3);
        }
    }
    count_lanes(prof + UVC_FRAGPROF_ends_off_region, on && !usable, lane);
    count_lanes(prof + UVC_FRAGPROF_ends_no_ref, on && usable && !acgt, lane);
    count_lanes(prof + UVC_FRAGPROF_ends, on && usable && acgt, lane);
    merge_add(prof + UVC_FRAGPROF_MOTIF_BINS, key, on && usable && acgt, lane);
}

__global__ void __launch_bounds__(256) k_fp_frag(RegionDev R, const UvcFragSpan *fspan, UvcUnitSpan *uspan, const UvcFamilyRange *ranges, int n_ranges, UvcFragmentProfileRequest req,
                                                 unsigned long long *rows, unsigned long long *parts) {
    __shared__ FpBlock B;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    fp_block_begin(B, tid);
    FpObj ob[FP_STEPS];
    int first_min = INT_MAX;
#pragma unroll
    for (int c = 0; c < FP_STEPS; c++) {
        FpObj &o = ob[c];
        o = FpObj{ 0, 0, n_ranges, -1 };
        const long long g = ((long long)blockIdx.x * FP_STEPS + c) * 256 + tid;
        int u = -1, tlo[1] = { INT_MAX }, thi[1] = { INT_MIN };
        if (g < R.n_frags) {
            const UvcFragSpan s = fspan[g];
            const bool fwd = (s.loF != INT_MAX), rev = (s.loR != INT_MAX);
            u = R.frags[g].fs;
            if (u < 0 || u >= R.n_fs) u = -1;
            if (fwd || rev) {
                o.lo = imin(s.loF, s.loR); o.hi = imax(s.hiF, s.hiR);
                o.kind = (fwd && rev) ? ((s.loF <= s.loR && s.hiF <= s.hiR) ? FP_PAIR : FP_OTHER) : FP_SINGLE;
                if (o.kind == FP_PAIR) { tlo[0] = o.lo; thi[0] = o.hi; }
                o.first = first_range(ranges, n_ranges, o.lo, o.hi);
                if (o.first < n_ranges) first_min = imin(first_min, o.first);
            }
        }
        // the pairs of a unit into its template span: the fragments of a unit are consecutive, a fragment that is no pair brings the empty span
        seg_fold_minmax<1>(u, tlo, thi);
        if (seg_head(u) && u >= 0 && tlo[0] != INT_MAX) { atomicMin(&uspan[u].lo, tlo[0]); atomicMax(&uspan[u].hi, thi[0]); }
    }
    const int w0 = B.win.choose(first_min);
    if (w0 == INT_MAX) return;   // (block-uniform) none of the block's fragments meets a range
#pragma unroll
    for (int c = 0; c < FP_STEPS; c++) {
        const FpObj o = ob[c];
        const long long L = (long long)o.hi - o.lo;
        const bool is_short = (L >= req.short_lo && L <= req.short_hi), is_long = (L >= req.long_lo && L <= req.long_hi);
        bool in_first = false;
        if (o.kind >= 0) {
            // (k_famstat_bin's walk and k_fp_fam's, each spelled out: through one shared walk with a callback this kernel takes 56 VGPRs for 54 and
            // k_fp_fam is scheduled differently; profiles/report_kernels_registers.txt)
            for (int i = o.first; i < n_ranges; i++) {
                const UvcFamilyRange q = ranges[i];
                if (q.pos_beg >= o.hi) break;   // the ranges ascend: no later one overlaps (o.lo < q.pos_end holds from `first` on)
                if (!(q.flags & UVC_FAMRANGE_CONTINUES) || o.lo >= q.pos_beg) {
                    B.win.add(w0, rows, i, UVC_FRAGPROF_pairs + o.kind, 1ull);
                    if (o.kind == FP_PAIR) {
                        B.win.add(w0, rows, i, UVC_FRAGPROF_len_sum, (unsigned long long)L);
                        if (is_short) B.win.add(w0, rows, i, UVC_FRAGPROF_short, 1ull);
                        if (is_long) B.win.add(w0, rows, i, UVC_FRAGPROF_long, 1ull);
                    }
                }
                if (q.prev_end <= o.lo) in_first = true;
            }
        }
        // the profile: the whole wave, so that equal keys merge
        const bool pair = (in_first && o.kind == FP_PAIR);
        count_lanes(B.prof + UVC_FRAGPROF_pairs, pair, lane);
        count_lanes(B.prof + UVC_FRAGPROF_others, in_first && o.kind == FP_OTHER, lane);
        count_lanes(B.prof + UVC_FRAGPROF_singles, in_first && o.kind == FP_SINGLE, lane);
        count_lanes(B.prof + UVC_FRAGPROF_short, pair && is_short, lane);
        count_lanes(B.prof + UVC_FRAGPROF_long, pair && is_long, lane);
        const long long wave_len = wave_sum(pair ? L : 0ll);
        if (lane == 0 && wave_len) lds_add(&B.len_sum, (unsigned long long)wave_len);
        merge_add(B.prof + UVC_FRAGPROF_LEN_BINS, (int)(L < 0 ? 0 : L < UVC_FRAGPROF_NLEN - 1 ? L : UVC_FRAGPROF_NLEN - 1), pair, lane);
        fp_end(R, (long long)o.lo - R.beg, false, pair, B.prof, lane);
        fp_end(R, (long long)o.hi - R.beg, true, pair, B.prof, lane);
    }
    fp_block_end(B, tid, w0, n_ranges, rows, parts + (size_t)(blockIdx.x % FP_SHARDS) * UVC_FRAGPROF_ROW);
}

__global__ void __launch_bounds__(256) k_fp_fam(RegionDev R, const UvcUnitSpan *uspan, const UvcFamilyRange *ranges, int n_ranges, unsigned long long *rows, unsigned long long *parts) {
    __shared__ FpBlock B;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    fp_block_begin(B, tid);
    FpObj ob[FP_STEPS];
    int first_min = INT_MAX;
#pragma unroll
    for (int c = 0; c < FP_STEPS; c++) {
        FpObj &o = ob[c];
        o = FpObj{ 0, 0, n_ranges, -1 };
        const long long u = ((long long)blockIdx.x * FP_STEPS + c) * 256 + tid;
        if (u >= R.n_fs) continue;
        const FsRec me = R.fss[u];
        const bool partner = (me.other_fs >= 0 && me.other_fs < R.n_fs);
        if (me.strand != 0 && partner) continue;   // the strand-0 unit makes the family's record (k_famstat_bin)
        UvcUnitSpan s = uspan[u];
        bool both = false;
        if (partner) {
            const UvcUnitSpan t = uspan[me.other_fs];
            both = (s.lo != INT_MAX && t.lo != INT_MAX);
            s.lo = imin(s.lo, t.lo); s.hi = imax(s.hi, t.hi);
        }
        if (s.lo == INT_MAX) continue;   // not sized: no pair fragment
        o.lo = s.lo; o.hi = s.hi; o.kind = both ? 1 : 0;
        o.first = first_range(ranges, n_ranges, o.lo, o.hi);
        if (o.first < n_ranges) first_min = imin(first_min, o.first);
    }
    const int w0 = B.win.choose(first_min);
    if (w0 == INT_MAX) return;   // (block-uniform) none of the block's families meets a range
#pragma unroll
    for (int c = 0; c < FP_STEPS; c++) {
        const FpObj o = ob[c];
        const long long TL = (long long)o.hi - o.lo;
        bool in_first = false;
        if (o.kind >= 0) {
            for (int i = o.first; i < n_ranges; i++) {
                const UvcFamilyRange q = ranges[i];
                if (q.pos_beg >= o.hi) break;
                if (!(q.flags & UVC_FAMRANGE_CONTINUES) || o.lo >= q.pos_beg) B.win.add(w0, rows, i, UVC_FRAGPROF_families, 1ull);
                if (q.prev_end <= o.lo) in_first = true;
            }
        }
        count_lanes(B.prof + UVC_FRAGPROF_families, in_first, lane);
        count_lanes(B.prof + UVC_FRAGPROF_families_both_strands, in_first && o.kind == 1, lane);
        merge_add(B.prof + UVC_FRAGPROF_FAMLEN_BINS, (int)(TL < 0 ? 0 : TL < UVC_FRAGPROF_NLEN - 1 ? TL : UVC_FRAGPROF_NLEN - 1), in_first, lane);
    }
    fp_block_end(B, tid, w0, n_ranges, rows, parts + (size_t)(blockIdx.x % FP_SHARDS) * UVC_FRAGPROF_ROW);
}

// The copies of the row summed into the result: one lane per word.  Not uvc_launch_sum_fold: FP_SHARDS is a compile-time count, so the 16
// loads of a lane are in flight together, and through the shared kernel's loop over a run-time count they wait one for the other -- 3 to
// 8 us more per call on the 1 Mb x 300x tile (profiles/report_kernels_bench.json).
__global__ void __launch_bounds__(256) k_fp_fold(const unsigned long long *parts, unsigned long long *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= UVC_FRAGPROF_ROW) return;
    unsigned long long v = 0;
    for (int s = 0; s < FP_SHARDS; s++) v += parts[(size_t)s * UVC_FRAGPROF_ROW + i];
    out[i] = v;
}
}   // namespace

extern "C" const char *uvc_fragprofile_name(int id) { return (id >= 0 && id < UVC_NFRAGPROF) ? FP_SECTIONS[id].name : nullptr; }
// copies of the profile row a call adds into (the result itself is one more)
extern "C" int64_t uvc_fragprofile_copies(void) { return FP_SHARDS; }
// d_fspan: n_frags rows and d_uspan: n_fs rows of scratch; d_ranges: the caller's n_ranges rows as they are; d_out: n_ranges TARGET rows and
// the profile row behind them; d_parts: uvc_fragprofile_copies() rows.  The init writes all of them: the caller clears nothing.
extern "C" void uvc_launch_fragprofile(const RegionDev *R, const RawReads *W, const UvcFragmentProfileRequest *req, UvcFragSpan *d_fspan, UvcUnitSpan *d_uspan, const UvcFamilyRange *d_ranges, int n_ranges,
                                       long long *d_out, long long *d_parts, hipStream_t s) {
    if (n_ranges <= 0) return;
    const long long n_out = (long long)n_ranges * FP_TROW + UVC_FRAGPROF_ROW, n_parts = (long long)FP_SHARDS * UVC_FRAGPROF_ROW;
    const long long n_init = std::max(std::max(n_out, n_parts), (long long)std::max(R->n_frags, R->n_fs));
    unsigned long long *rows = (unsigned long long *)d_out, *prof = rows + (size_t)n_ranges * FP_TROW, *parts = (unsigned long long *)d_parts;
    hipLaunchKernelGGL(k_fp_init, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, s, d_fspan, R->n_frags, d_uspan, R->n_fs, rows, n_out, parts, n_parts);
    if (R->n_frags <= 0 || R->n_fs <= 0 || R->n_alns <= 0) return;   // (the result is zeros)
    hipLaunchKernelGGL(k_fp_span, dim3((unsigned)(((long long)R->n_alns + 255) / 256)), dim3(256), 0, s, W->pos, W->endpos, W->frag, W->flag, W->mapq, R->n_alns, R->n_frags, req->min_mapq, d_fspan);
    hipLaunchKernelGGL(k_fp_frag, dim3((unsigned)(((long long)R->n_frags + 256 * FP_STEPS - 1) / (256 * FP_STEPS))), dim3(256), 0, s, *R, (const UvcFragSpan *)d_fspan, d_uspan, d_ranges, n_ranges, *req, rows, parts);
    hipLaunchKernelGGL(k_fp_fam, dim3((unsigned)(((long long)R->n_fs + 256 * FP_STEPS - 1) / (256 * FP_STEPS))), dim3(256), 0, s, *R, (const UvcUnitSpan *)d_uspan, d_ranges, n_ranges, rows, parts);
    hipLaunchKernelGGL(k_fp_fold, dim3((unsigned)((UVC_FRAGPROF_ROW + 255) / 256)), dim3(256), 0, s, (const unsigned long long *)parts, prof);
}
