// uvc_coverage.hip -- uvcgpu_region_coverage: depth statistics of many ranges of the accumulated planes in one pass.
//
// The ranges are laid end to end (compact position i = exclusive prefix of the range lengths + offset in the range, as k_range_map and
// k_block_stats_windows lay theirs) and the work is split by compact position, never by range: a 100 bp exon and a whole 1 Mb tile load the
// machine alike.  A lane owns one compact position per step, finds its range by a search in the prefix (and keeps it while its positions stay
// inside), reads the cells of the six measures -- every cell once per call, 64 consecutive positions of a plane per wave instruction -- and
// keeps sum / min / max / counts in registers.  While all lanes of a wave stay in one range nothing crosses lanes; a wave reduces (butterfly
// over the 64 lanes) and merges into the range's row only when the range changes or its positions end.  The merge is one 64-bit vector atomic
// per (wave, range segment, statistic), issued by one lane each.  The arithmetic is integer: the order of the merges does not show.
#include "uvc_launch.h"

#include <algorithm>
#include <limits.h>

namespace {
enum {
#define UVC_COV(name, group, plane) COVROW_##name,
#include "uvc_coverage.def"
#undef UVC_COV
    COVROW_N
};
static_assert(COVROW_N == UVC_NCOV, "include/uvc_coverage.def and UvcCoverageMeasure of uvcgpu.h list the same measures");
#define UVC_COV(name, group, plane) static_assert((int)COVROW_##name == (int)UVC_COV_##name, "uvc_coverage.def order = UvcCoverageMeasure order");
#include "uvc_coverage.def"
#undef UVC_COV
static_assert(UVC_COV_ROW == UVC_COV_GE + UVC_COV_MAX_THRESHOLDS, "a row is sum, min, max and the threshold counts");

const char *const COV_NAMES[UVC_NCOV] = {
#define UVC_COV(name, group, plane) #name,
#include "uvc_coverage.def"
#undef UVC_COV
};

struct CovThr { int t[UVC_COV_MAX_THRESHOLDS]; };   // unused slots hold INT_MAX
// A lane's statistics of one range.  The threshold counts are packed two to a register (threshold k in the low half, k + 4 in the high half):
// a lane counts at most COV_MAX_STEPS positions and a wave 64 times that, far below 2^16.
#define COV_MAX_STEPS 16
#define COV_NGE2 (UVC_COV_MAX_THRESHOLDS / 2)
struct CovAcc { long long sum[UVC_NCOV]; int mn[UVC_NCOV], mx[UVC_NCOV]; unsigned ge2[UVC_NCOV][COV_NGE2]; };
static_assert(64 * COV_MAX_STEPS < 65536, "the packed counts of a wave fit 16 bits");

DEV void acc_clear(CovAcc &a) {
#pragma unroll
    for (int m = 0; m < UVC_NCOV; m++) {
        a.sum[m] = 0; a.mn[m] = INT_MAX; a.mx[m] = INT_MIN;
#pragma unroll
        for (int k = 0; k < COV_NGE2; k++) a.ge2[m][k] = 0;
    }
}
DEV void acc_add(CovAcc &a, const int (&v)[UVC_NCOV], const CovThr &T) {   // (unused thresholds are INT_MAX: never reached, their counts stay 0)
#pragma unroll
    for (int m = 0; m < UVC_NCOV; m++) {
        a.sum[m] += v[m]; a.mn[m] = imin(a.mn[m], v[m]); a.mx[m] = imax(a.mx[m], v[m]);
#pragma unroll
        for (int k = 0; k < COV_NGE2; k++) a.ge2[m][k] += (v[m] >= T.t[k] ? 1u : 0u) + (v[m] >= T.t[k + COV_NGE2] ? 0x10000u : 0u);
    }
}
// The wave's lanes hold partial statistics of one range (neutral values in lanes that have none): butterfly over the 64 lanes, then lane j
// merges statistic j of the row (66 statistics: two rounds).  A zero is not added; min and max always go out (every range has a position).
// The butterfly is written out here, all statistics per distance, and not as wave_sum / wave_min / wave_max of uvc_collectives.h per
// statistic: with those k_coverage takes 167 VGPRs instead of 161 (171 and 177 in two other orders of the calls), at or past the 168 that
// three waves per SIMD allow (profiles/collectives_registers.txt).
DEV void wave_merge(CovAcc a, long long rid, long long *out) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int m = 0; m < UVC_NCOV; m++) {
            a.sum[m] += __shfl_xor(a.sum[m], d, 64);
            a.mn[m] = imin(a.mn[m], __shfl_xor(a.mn[m], d, 64));
            a.mx[m] = imax(a.mx[m], __shfl_xor(a.mx[m], d, 64));
#pragma unroll
            for (int k = 0; k < COV_NGE2; k++) a.ge2[m][k] += __shfl_xor(a.ge2[m][k], d, 64);
        }
    }
    const int lane = (int)(threadIdx.x & 63);
    long long *row = out + (size_t)rid * (UVC_NCOV * UVC_COV_ROW);
#pragma unroll
    for (int j0 = 0; j0 < UVC_NCOV * UVC_COV_ROW; j0 += 64) {
        const int j = j0 + lane;
        long long val = 0;
#pragma unroll
        for (int m = 0; m < UVC_NCOV; m++) {
            if (j == m * UVC_COV_ROW + UVC_COV_SUM) val = a.sum[m];
            if (j == m * UVC_COV_ROW + UVC_COV_MIN) val = a.mn[m];
            if (j == m * UVC_COV_ROW + UVC_COV_MAX) val = a.mx[m];
#pragma unroll
            for (int k = 0; k < COV_NGE2; k++) {
                if (j == m * UVC_COV_ROW + UVC_COV_GE + k) val = a.ge2[m][k] & 0xFFFFu;
                if (j == m * UVC_COV_ROW + UVC_COV_GE + k + COV_NGE2) val = a.ge2[m][k] >> 16;
            }
        }
        if (j >= UVC_NCOV * UVC_COV_ROW) continue;
        const int k = j % UVC_COV_ROW;
        if (k == UVC_COV_MIN) atomicMin(row + j, val);
        else if (k == UVC_COV_MAX) atomicMax(row + j, val);
        else if (val != 0) atomicAdd((unsigned long long *)(row + j), (unsigned long long)val);
    }
}

// rows before the merges: sum and counts 0, min / max at the neutral values of the 64-bit atomics
__global__ void __launch_bounds__(256) k_coverage_init(long long *out, long long n_cells) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cells) return;
    const int k = (int)(i % UVC_COV_ROW);
    out[i] = (k == UVC_COV_MIN ? LLONG_MAX : (k == UVC_COV_MAX ? LLONG_MIN : 0));
}

// Few long ranges: every wave's merges meet on the same 66 words per range, and atomics on one word run one after the other (measured:
// 61 ns per merge and word, DESIGN.md 4i and profiles/r07_coverage_timings.txt).  The waves then merge into `shards` copies of each row (wave
// index modulo shards) and this kernel folds the copies into the caller's row: one lane per statistic.
__global__ void __launch_bounds__(256) k_coverage_fold(const long long *parts, int shards, long long *out, long long n_cells) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cells) return;
    const long long rid = i / (UVC_NCOV * UVC_COV_ROW); const int j = (int)(i % (UVC_NCOV * UVC_COV_ROW)), k = j % UVC_COV_ROW;
    long long v = (k == UVC_COV_MIN ? LLONG_MAX : (k == UVC_COV_MAX ? LLONG_MIN : 0));
    for (int s = 0; s < shards; s++) {
        const long long p = parts[(rid * shards + s) * (UVC_NCOV * UVC_COV_ROW) + j];
        v = (k == UVC_COV_MIN ? lmin(v, p) : (k == UVC_COV_MAX ? lmax(v, p) : v + p));
    }
    out[i] = v;
}

// One wave takes `steps` consecutive groups of 64 compact positions.  Its registers hold the statistics of one range at a time (`cur`); the
// positions of a step are taken range by range in ascending order, and a change of range sends what was kept to that range's row.  One
// more round behind the last step sends the rest, so the merge exists once in the code.
__global__ void __launch_bounds__(256) k_coverage(RegionDev R, const UvcRangeRow *tab, int n_ranges, int n_total, int steps, int shards, CovThr T, long long *out) {
    const int lane = (int)(threadIdx.x & 63);
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long base = wave * 64 * steps;
    if (base >= n_total) return;
    const int shard = (int)(wave % shards);   // the copy of every row this wave merges into (row index = range * shards + shard)
    CovAcc acc; acc_clear(acc);
    int cur = -1;                                      // wave-uniform: the range the accumulators belong to, -1 = none
    UvcRangeCursor g;                                  // this lane's range
    for (int c = 0; ; c++) {
        const bool last = (c >= steps || base + (long long)c * 64 >= n_total);   // wave-uniform
        const long long i = base + (long long)c * 64 + lane;
        bool act = (!last && i < n_total);
        int v[UVC_NCOV];
#pragma unroll
        for (int m = 0; m < UVC_NCOV; m++) v[m] = 0;
        if (act) {
            uvc_range_find(g, tab, n_ranges, i);
            const int64_t x = (int64_t)g.x0 + (i - g.first);
            act = (x >= 0 && x < R.npos);   // (the host has checked every range against the region)
            if (act) {
                int q = 0;
#define UVC_COV(name, group, plane) v[q++] = cov_##group(R, plane, x);
#include "uvc_coverage.def"
#undef UVC_COV
            }
        }
        const int my = act ? g.rid : -1;
        unsigned long long todo = last ? 1ull : __ballot(act);
        while (todo) {
            const int seg = last ? -1 : __shfl(my, __ffsll((long long)todo) - 1, 64);
            const bool in = (act && my == seg);
            if (seg != cur) {
                if (cur >= 0) wave_merge(acc, (long long)cur * shards + shard, out);
                acc_clear(acc);
                cur = seg;
            }
            if (in) acc_add(acc, v, T);
            todo = last ? 0ull : (todo & ~__ballot(in));
        }
        if (last) break;
    }
}
}   // namespace

extern "C" const char *uvc_coverage_name(int id) { return (id >= 0 && id < UVC_NCOV) ? COV_NAMES[id] : nullptr; }
static void cov_geometry(int n_ranges, int64_t n_total, int &steps, long long &n_waves, int &shards) {
    // a wave keeps its statistics in registers over `steps` groups of 64 positions: fewer merges into a long range's row, as long as 2 048
    // waves (two per SIMD) stay to fill the machine.  Where the waves still outnumber the ranges 256 to 1 the rows are sharded (k_coverage_fold):
    // 256 merges per word are 16 us of chain, under what the reads take; at most 16 copies of a row
    steps = (int)std::max<int64_t>(1, std::min<int64_t>(COV_MAX_STEPS, n_total / (64 * 2048)));
    n_waves = (n_total + 64LL * steps - 1) / (64LL * steps);
    shards = (int)std::max<long long>(1, std::min<long long>(16, n_waves / (256LL * n_ranges)));
}
// rows of scratch (beside the n_ranges rows of the result) a call needs: the shard copies, 0 when the rows are not sharded
extern "C" int64_t uvc_coverage_scratch_rows(int n_ranges, int64_t n_total) {
    int steps, shards; long long n_waves;
    cov_geometry(n_ranges, n_total, steps, n_waves, shards);
    return shards > 1 ? (int64_t)n_ranges * shards : 0;
}
// d_tab: n_ranges + 1 entries of { plane index of the first position, first compact position }, the last one { 0, n_total }; d_out: n_ranges rows;
// d_scratch: the scratch_rows = uvc_coverage_scratch_rows(n_ranges, n_total) rows the caller allocated (a call with fewer launches nothing)
extern "C" void uvc_launch_coverage(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const int32_t *thr, int n_thr, long long *d_out, long long *d_scratch, int64_t scratch_rows, hipStream_t s) {
    if (n_ranges <= 0 || n_total <= 0 || scratch_rows < uvc_coverage_scratch_rows(n_ranges, n_total)) return;
    int steps, shards; long long n_waves;
    cov_geometry(n_ranges, n_total, steps, n_waves, shards);
    const long long n_final = (long long)n_ranges * UVC_NCOV * UVC_COV_ROW, n_cells = n_final * shards;
    long long *d_parts = (shards > 1 ? d_scratch : d_out);
    hipLaunchKernelGGL(k_coverage_init, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, s, d_parts, n_cells);
    CovThr T;
    for (int k = 0; k < UVC_COV_MAX_THRESHOLDS; k++) T.t[k] = (k < n_thr ? thr[k] : INT_MAX);
    hipLaunchKernelGGL(k_coverage, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, s, *R, d_tab, n_ranges, (int)n_total, steps, shards, T, d_parts);
    if (shards > 1) hipLaunchKernelGGL(k_coverage_fold, dim3((unsigned)((n_final + 255) / 256)), dim3(256), 0, s, d_parts, shards, d_out, n_final);
}
