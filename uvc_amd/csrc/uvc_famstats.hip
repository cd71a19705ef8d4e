// uvc_famstats.hip -- uvcgpu_region_family_stats: family-size statistics of ranges from the unit records of set_reads (the
// definitions are in uvcgpu.h).  Nothing here reads the planes: the inputs are RegionDev::fss / frags and the alignments' pos / end columns.
//
// Stage one, the span of every family-strand unit (k_famstat_span).  a, b and n of a family need no walk: a unit's fragments are
// frag_end - frag_beg and its alignments run from its first fragment's aln_beg to its last one's aln_end.  Only lo and hi have to be reduced
// over the alignments, and a unit holds one alignment or tens of thousands (a non-UMI amplicon pile).  So the work is split by alignment,
// never by unit: a lane takes one alignment (pos, end and unit index are 4-byte columns: 64 consecutive alignments are one wave
// instruction each; AlnRec::pos / rend hold the same two numbers 200 bytes apart), the alignments of a unit are consecutive, and a wave reduces each
// run of equal unit indices among its lanes with a segmented butterfly (seg_fold_minmax).  The head lane of a run merges it into the unit's { lo, hi } with
// one atomicMin and one atomicMax: a unit of 30 000 alignments costs 470 pairs of atomics on its word, a unit of one alignment one pair.
//
// Stage two, the rows (k_famstat_bin).  A lane takes one unit; the strand-0 unit of a family -- or its strand-1 unit where there is no
// other -- joins its partner (FsRec::other_fs) into the family record { a, b, n, lo, hi, dflag }, finds its first range (first_range) and
// walks forward while the family overlaps.  A 365-word row per range does not fit LDS for hundreds of ranges, and one range must not put
// every lane of the machine on the same 365 global words.  So a block keeps a UvcRowWindow of FS_WIN consecutive ranges (the units of a
// tile come roughly in position order, so most adds of a block fall into its window; with at most FS_WIN ranges every add does).  LDS
// words are 32 bits: a block's families add each counter of a row at most once per family, and a region holds fewer than 2^30 alignments.
// Integer adds only: their order does not show, the rows are the same bits from call to call.
#include "uvc_report_dev.h"

namespace {
enum {
#define UVC_FAMSTAT(name, first, words) FSROW_##name,
#include "uvc_famstats.def"
#undef UVC_FAMSTAT
    FSROW_N
};
static_assert(FSROW_N == UVC_NFAMSTAT, "include/uvc_famstats.def and UvcFamStat of uvcgpu.h list the same sections");
#define UVC_FAMSTAT(name, first, words) static_assert((int)FSROW_##name == (int)UVC_FAMSTAT_##name, "uvc_famstats.def order = UvcFamStat order");
#include "uvc_famstats.def"
#undef UVC_FAMSTAT
constexpr UvcSection FS_SECTIONS[UVC_NFAMSTAT] = {
#define UVC_FAMSTAT(name, first, words) { #name, first, words },
#include "uvc_famstats.def"
#undef UVC_FAMSTAT
};
static_assert(uvc_sections_tile(FS_SECTIONS, UVC_FAMSTAT_ROW), "the sections of uvc_famstats.def tile the row");
static_assert(FS_SECTIONS[UVC_FAMSTAT_target_families].first == UVC_FAMSTAT_TARGET && FS_SECTIONS[UVC_FAMSTAT_families].first == UVC_FAMSTAT_FIRST
              && FS_SECTIONS[UVC_FAMSTAT_size].first == UVC_FAMSTAT_SIZE && FS_SECTIONS[UVC_FAMSTAT_size].words == UVC_FAMSTAT_NSIZE
              && FS_SECTIONS[UVC_FAMSTAT_strands].first == UVC_FAMSTAT_STRANDS && FS_SECTIONS[UVC_FAMSTAT_strands].words == (UVC_FAMSTAT_STRAND_CAP + 1) * (UVC_FAMSTAT_STRAND_CAP + 1),
              "the block offsets of uvcgpu.h are those of uvc_famstats.def");
static_assert(sizeof(UvcFamilyRange) == 16, "the host uploads the caller's ranges as 16-byte rows");

#define FS_WIN 16     // ranges whose partial rows a block keeps in LDS: 16 * 365 * 4 = 23 360 B, two blocks (8 waves) per CU and more
#define FS_STEPS 4    // units per lane: a block of 256 lanes bins 1 024 units into one window before it flushes

// every unit's span starts empty, every row at 0
__global__ void __launch_bounds__(256) k_famstat_init(UvcUnitSpan *span, int n_fs, unsigned long long *rows, long long n_words) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_fs) span[i] = UvcUnitSpan{ INT_MAX, INT_MIN };
    if (i < n_words) rows[i] = 0;
}

__global__ void __launch_bounds__(256) k_famstat_span(const int32_t *pos, const int32_t *endpos, const int32_t *fs_of, int n_alns, int n_fs, UvcUnitSpan *span) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int u = -1, p[1] = { INT_MAX }, e[1] = { INT_MIN };
    if (i < n_alns) { u = fs_of[i]; p[0] = pos[i]; e[0] = endpos[i]; }
    if (u < 0 || u >= n_fs) u = -1;   // (no such unit: set_reads refuses these reads)
    seg_fold_minmax<1>(u, p, e);   // the run of a unit among the lanes
    if (seg_head(u) && u >= 0) { atomicMin(&span[u].lo, p[0]); atomicMax(&span[u].hi, e[0]); }
}

struct FsFamily { int a, b, n, lo, hi, dflag, first; };   // first: the first range that ends behind lo; n_ranges: the lane has no family or no range

__global__ void __launch_bounds__(256) k_famstat_bin(RegionDev R, const UvcUnitSpan *span, const UvcFamilyRange *ranges, int n_ranges, unsigned long long *rows) {
    __shared__ UvcRowWindow<unsigned, FS_WIN, UVC_FAMSTAT_ROW> win;
    const int tid = (int)threadIdx.x;
    win.begin(tid);
    __syncthreads();
    FsFamily fam[FS_STEPS];
    int first_min = INT_MAX;
#pragma unroll
    for (int c = 0; c < FS_STEPS; c++) {
        FsFamily &f = fam[c];
        f = FsFamily{ 0, 0, 0, 0, 0, 0, n_ranges };
        const long long u = ((long long)blockIdx.x * FS_STEPS + c) * 256 + tid;
        if (u >= R.n_fs) continue;
        const FsRec me = R.fss[u];
        const bool partner = (me.other_fs >= 0 && me.other_fs < R.n_fs);
        if (me.strand != 0 && partner) continue;   // the strand-0 unit makes the family's record
        if (me.frag_end <= me.frag_beg) continue;
        int a = (me.strand != 0 ? 0 : me.frag_end - me.frag_beg), b = (me.strand != 0 ? me.frag_end - me.frag_beg : 0);
        f.n = R.frags[me.frag_end - 1].aln_end - R.frags[me.frag_beg].aln_beg;
        UvcUnitSpan s = span[u];
        if (partner) {
            const FsRec ot = R.fss[me.other_fs];
            if (ot.frag_end > ot.frag_beg) {
                b += ot.frag_end - ot.frag_beg;   // (me is the strand-0 unit here)
                f.n += R.frags[ot.frag_end - 1].aln_end - R.frags[ot.frag_beg].aln_beg;
                const UvcUnitSpan t = span[me.other_fs];
                s.lo = imin(s.lo, t.lo); s.hi = imax(s.hi, t.hi);
            }
        }
        f.a = a; f.b = b; f.lo = s.lo; f.hi = s.hi; f.dflag = me.dflag;
        if (f.hi <= f.lo) continue;   // (a unit without alignments)
        f.first = first_range(ranges, n_ranges, f.lo, f.hi);
        if (f.first < n_ranges) first_min = imin(first_min, f.first);
    }
    const int w0 = win.choose(first_min);
    if (w0 == INT_MAX) return;   // (block-uniform) none of the block's families meets a range
#pragma unroll
    for (int c = 0; c < FS_STEPS; c++) {
        const FsFamily &f = fam[c];
        const int frg = f.a + f.b;
        const bool both = (f.a >= 1 && f.b >= 1);
        for (int i = f.first; i < n_ranges; i++) {
            const UvcFamilyRange q = ranges[i];
            if (q.pos_beg >= f.hi) break;   // the ranges ascend: no later one overlaps (f.lo < q.pos_end holds from `first` on)
            const auto add = [&](int word, unsigned v) { win.add(w0, rows, i, word, v); };
            if (!(q.flags & UVC_FAMRANGE_CONTINUES) || f.lo >= q.pos_beg) {
                add(UVC_FAMSTAT_TARGET + 0, 1u);
                add(UVC_FAMSTAT_TARGET + 1, (unsigned)frg);
                add(UVC_FAMSTAT_TARGET + 2, (unsigned)f.n);
                if (both) add(UVC_FAMSTAT_TARGET + 3, 1u);
            }
            if (q.prev_end <= f.lo) {
                add(UVC_FAMSTAT_FIRST + 0, 1u);
                add(UVC_FAMSTAT_FIRST + 1, (unsigned)frg);
                add(UVC_FAMSTAT_FIRST + 2, (unsigned)f.n);
                if (both) add(UVC_FAMSTAT_FIRST + 3, 1u);
                if (f.dflag & 1) add(UVC_FAMSTAT_FIRST + 4, 1u);
                if (f.dflag & 2) add(UVC_FAMSTAT_FIRST + 5, 1u);
                if (f.dflag & 4) add(UVC_FAMSTAT_FIRST + 6, 1u);
                add(UVC_FAMSTAT_SIZE + imin(frg, UVC_FAMSTAT_NSIZE) - 1, 1u);
                add(UVC_FAMSTAT_STRANDS + imin(f.a, UVC_FAMSTAT_STRAND_CAP) * (UVC_FAMSTAT_STRAND_CAP + 1) + imin(f.b, UVC_FAMSTAT_STRAND_CAP), 1u);
            }
        }
    }
    __syncthreads();
    win.flush(tid, w0, n_ranges, rows);
}
static_assert(UVC_FAMSTAT_families_umi == UVC_FAMSTAT_families + 4 && UVC_FAMSTAT_families_duplex_tag == UVC_FAMSTAT_families + 5 && UVC_FAMSTAT_families_amplicon == UVC_FAMSTAT_families + 6
              && UVC_FAMSTAT_target_families_both_strands == 3 && UVC_FAMSTAT_families_both_strands == UVC_FAMSTAT_families + 3, "k_famstat_bin's counter order");
}   // namespace

extern "C" const char *uvc_famstats_name(int id) { return (id >= 0 && id < UVC_NFAMSTAT) ? FS_SECTIONS[id].name : nullptr; }
// d_span: n_fs rows of scratch; d_ranges: the caller's n_ranges rows as they are; d_rows: n_ranges rows of UVC_FAMSTAT_ROW words
extern "C" void uvc_launch_famstats(const RegionDev *R, const int32_t *pos, const int32_t *endpos, const int32_t *fs_of, UvcUnitSpan *d_span, const UvcFamilyRange *d_ranges, int n_ranges, long long *d_rows, hipStream_t s) {
    if (n_ranges <= 0) return;
    const long long n_words = (long long)n_ranges * UVC_FAMSTAT_ROW, n_init = n_words > R->n_fs ? n_words : (long long)R->n_fs;
    hipLaunchKernelGGL(k_famstat_init, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, s, d_span, R->n_fs, (unsigned long long *)d_rows, n_words);
    if (R->n_fs <= 0 || R->n_alns <= 0) return;
    hipLaunchKernelGGL(k_famstat_span, dim3((unsigned)(((long long)R->n_alns + 255) / 256)), dim3(256), 0, s, pos, endpos, fs_of, R->n_alns, R->n_fs, d_span);
    hipLaunchKernelGGL(k_famstat_bin, dim3((unsigned)(((long long)R->n_fs + 256 * FS_STEPS - 1) / (256 * FS_STEPS))), dim3(256), 0, s, *R, d_span, d_ranges, n_ranges, (unsigned long long *)d_rows);
}
