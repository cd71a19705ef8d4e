// uvc_errprofile.hip -- uvcgpu_region_error_profile: the background error profile of ranges of the accumulated planes in one pass
// (the definitions are in uvcgpu.h).
//
// The ranges are laid end to end as k_coverage lays them (compact position i = exclusive prefix of the range lengths + offset in the range)
// and the work is split by compact position: a block takes 256 * steps consecutive ones, a lane one per step, so that 64 consecutive positions
// of a plane are one wave instruction.  A lane forms the context of its position from three reference symbols, reads the 99 cells of the
// position once (4 levels x 2 strands x 11 symbols, 11 of dDP1), applies the two gates per level and kind and adds the cells that pass to a
// block-private copy of the profile in LDS: a data-dependent scatter, [level][ctx][symbol], with LDS atomics.  Neighbouring lanes mostly
// differ in ctx, so the adds of one wave instruction spread over the table; zero cells (most non-reference ones) are not added.  The six
// counters per level and no_context are the same word for every lane: a wave counts them with a ballot and one lane adds the count.
// The LDS words are 64 bits wide: a cell is below 2^31 and a block may feed thousands of positions to one bin, so 32-bit partials have no
// bound that holds for every input; at 28 KB a CU holds five blocks (20 waves).  Whether that occupancy or the LDS adds limit the kernel is
// a question for the measurements of DESIGN.md 4j, not settled here.
// At the end a block adds its non-zero words to the result with 64-bit vector atomics.  Integer arithmetic only: the order of the adds does
// not show, the result is the same bits from call to call.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
enum {
#define UVC_ERRLEVEL(name, group, plane) ERRROW_##name,
#include "uvc_errprofile.def"
#undef UVC_ERRLEVEL
    ERRROW_N
};
static_assert(ERRROW_N == UVC_NERRLEVEL, "include/uvc_errprofile.def and UvcErrLevel of uvcgpu.h list the same levels");
#define UVC_ERRLEVEL(name, group, plane) static_assert((int)ERRROW_##name == (int)UVC_ERRLEVEL_##name, "uvc_errprofile.def order = UvcErrLevel order");
#include "uvc_errprofile.def"
#undef UVC_ERRLEVEL
static_assert(UVC_ERR_LINK_BINS == UVC_ERR_BASE_BINS + UVC_ERR_NCTX * UVC_ERR_NBASE && UVC_ERR_COUNTERS == UVC_ERR_LINK_BINS + UVC_ERR_NCTX * UVC_ERR_NLINK
              && UVC_ERR_ROW == UVC_ERR_COUNTERS + UVC_NERRC, "a row is the BASE bins, the LINK bins and the counters");
static_assert(UVC_BASE_T == UVC_ERR_NBASE - 1 && UVC_LINK_I1 - UVC_LINK_M == UVC_ERR_NLINK - 1, "the symbols of the two kinds are A..T and LINK_M..LINK_I1");

const char *const ERR_NAMES[UVC_NERRLEVEL] = {
#define UVC_ERRLEVEL(name, group, plane) #name,
#include "uvc_errprofile.def"
#undef UVC_ERRLEVEL
};

#define ERR_CELLS (UVC_NERRLEVEL * UVC_ERR_ROW)   // 3 560 words of a profile
#define ERR_MAX_STEPS 16
#define ERR_MAX_SHARDS 16

// c_L(s, x): the level's cell, both strands summed where the group has them.  Symbol slot j: 0..3 = A..T, 4..10 = LINK_M..LINK_I1
DEV int err_sym(int j) { return j < UVC_ERR_NBASE ? j : UVC_LINK_M + (j - UVC_ERR_NBASE); }
DEV long long err_FRAG(const RegionDev &R, int plane, int s, int64_t x) { return (long long)FRP(R, 0, plane, s, x) + FRP(R, 1, plane, s, x); }
DEV long long err_FAM(const RegionDev &R, int plane, int s, int64_t x) { return (long long)FAP(R, 0, plane, s, x) + FAP(R, 1, plane, s, x); }
DEV long long err_DUPLEX(const RegionDev &R, int plane, int s, int64_t x) { return (long long)DUP(R, plane, s, x); }

// One kind of one level at one position: v[0] is the reference symbol's cell when ref == 0 (LINK: LINK_M is slot 0), else ref names the slot
// (BASE: m).  `ctx` < 0: the position has no context (or the lane has no position) and adds nothing.
template <int N> DEV void err_kind(const long long (&v)[N], int ref, int ctx, int min_depth, int permille, unsigned long long *bins, unsigned long long *counters, int lane) {
    long long d = 0, a = 0;
#pragma unroll
    for (int j = 0; j < N; j++) { d += v[j]; if (j != ref) a = lmax(a, v[j]); }
    const bool on = (ctx >= 0);
    const bool low = on && d < (long long)min_depth;
    const bool high = on && !low && a * 1000 > (long long)permille * d;
    const bool counted = on && !low && !high;
    if (counted) {
#pragma unroll
        for (int j = 0; j < N; j++) if (v[j] != 0) lds_add(bins + ctx * N + j, (unsigned long long)v[j]);
    }
    count_lanes(counters + 0, counted, lane);   // UVC_ERRC_<kind>_counted, _low_depth, _high_alt
    count_lanes(counters + 1, low, lane);
    count_lanes(counters + 2, high, lane);
}
static_assert(UVC_ERRC_BASE_low_depth == UVC_ERRC_BASE_counted + 1 && UVC_ERRC_BASE_high_alt == UVC_ERRC_BASE_counted + 2
              && UVC_ERRC_LINK_low_depth == UVC_ERRC_LINK_counted + 1 && UVC_ERRC_LINK_high_alt == UVC_ERRC_LINK_counted + 2, "err_kind's counter order");

// every copy of the profile starts at 0
__global__ void __launch_bounds__(256) k_errprofile_init(unsigned long long *out, int n_cells) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_cells) out[i] = 0;
}

__global__ void __launch_bounds__(256) k_errprofile(RegionDev R, const UvcRangeRow *tab, int n_ranges, int n_total, int steps, int shards, int min_depth, int permille, unsigned long long *out) {
    __shared__ unsigned long long prof[ERR_CELLS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int j = tid; j < ERR_CELLS; j += 256) prof[j] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * 256 * steps;
    UvcRangeCursor g;   // this lane's range
    for (int c = 0; c < steps; c++) {
        const long long i0 = base + (long long)c * 256 + (tid & ~63);   // the wave's first compact position of this step: wave-uniform
        if (i0 >= n_total) break;
        const long long i = i0 + lane;
        bool act = (i < n_total);
        int64_t x = 0;
        if (act) {
            uvc_range_find(g, tab, n_ranges, i);
            x = (int64_t)g.x0 + (i - g.first);
            act = (x >= 0 && x < R.npos);   // (the host has checked every range against the region)
        }
        // the context: reference symbols exist for plane indices 0 .. npos - 2 (the region's last position, `end`, has no reference base)
        int ctx = -1, m = 0;
        if (act) {
            const int64_t n_ref = R.npos - 1;
            const int sl = (x - 1 >= 0 && x - 1 < n_ref) ? (int)R.refsym[x - 1] : UVC_BASE_N;
            const int sm = (x < n_ref) ? (int)R.refsym[x] : UVC_BASE_N;
            const int sr = (x + 1 < n_ref) ? (int)R.refsym[x + 1] : UVC_BASE_N;
            if (sl <= UVC_BASE_T && sm <= UVC_BASE_T && sr <= UVC_BASE_T) { ctx = 16 * sl + 4 * sm + sr; m = sm; }
        }
        {   // no_context: once per position, the same count in every level's row
            const unsigned long long none = __ballot(act && ctx < 0);
            if (lane < UVC_NERRLEVEL && none) lds_add(prof + lane * UVC_ERR_ROW + UVC_ERR_COUNTERS + UVC_ERRC_no_context, (unsigned long long)__popcll(none));
        }
        if (__ballot(ctx >= 0) == 0) continue;   // wave-uniform: nothing but no_context here
        const int64_t xs = (ctx >= 0 ? x : 0);   // lanes without a context read nothing
        int level = 0;
#define UVC_ERRLEVEL(name, group, plane) { \
            long long vb[UVC_ERR_NBASE], vl[UVC_ERR_NLINK]; \
            _Pragma("unroll") for (int j = 0; j < UVC_ERR_NBASE; j++) vb[j] = (ctx >= 0 ? err_##group(R, plane, err_sym(j), xs) : 0); \
            _Pragma("unroll") for (int j = 0; j < UVC_ERR_NLINK; j++) vl[j] = (ctx >= 0 ? err_##group(R, plane, err_sym(UVC_ERR_NBASE + j), xs) : 0); \
            unsigned long long *row = prof + level * UVC_ERR_ROW; \
            err_kind<UVC_ERR_NBASE>(vb, m, ctx, min_depth, permille, row + UVC_ERR_BASE_BINS, row + UVC_ERR_COUNTERS + UVC_ERRC_BASE_counted, lane); \
            err_kind<UVC_ERR_NLINK>(vl, 0, ctx, min_depth, permille, row + UVC_ERR_LINK_BINS, row + UVC_ERR_COUNTERS + UVC_ERRC_LINK_counted, lane); \
            level++; }
#include "uvc_errprofile.def"
#undef UVC_ERRLEVEL
    }
    __syncthreads();
    unsigned long long *dst = out + (size_t)(blockIdx.x % (unsigned)shards) * ERR_CELLS;
    for (int j = tid; j < ERR_CELLS; j += 256) { const unsigned long long v = prof[j]; if (v) atomicAdd(dst + j, v); }
}

void err_geometry(int64_t n_total, int &steps, long long &n_blocks, int &shards) {
    // a block keeps its profile in LDS over `steps` groups of 256 positions: fewer flushes, as long as 1 024 blocks (four per CU) stay to fill
    // the machine.  From 128 blocks on the profile is sharded (its flushes meet on the same 3 560 words; uvc_launch_sum_fold sums the copies), at most 16 copies: up to 1 024 blocks (4 M positions at 16
    // steps) fewer than 128 flushes meet on one word; beyond that the chain on a word grows with the positions, blocks / 16 flushes
    steps = (int)std::max<int64_t>(1, std::min<int64_t>(ERR_MAX_STEPS, n_total / (256 * 1024)));
    n_blocks = (n_total + 256LL * steps - 1) / (256LL * steps);
    shards = (int)std::max<long long>(1, std::min<long long>(ERR_MAX_SHARDS, n_blocks / 64));
}
}   // namespace

extern "C" const char *uvc_errprofile_level_name(int id) { return (id >= 0 && id < UVC_NERRLEVEL) ? ERR_NAMES[id] : nullptr; }
// profiles of scratch (beside the one of the result) a call may need: the shard copies
extern "C" int64_t uvc_errprofile_scratch_cells(void) { return (int64_t)ERR_MAX_SHARDS * ERR_CELLS; }
// d_tab: n_ranges + 1 entries of { plane index of the first position, first compact position }, the last one { 0, n_total }; d_out: one profile;
// d_scratch: uvc_errprofile_scratch_cells() words
extern "C" void uvc_launch_errprofile(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, int min_depth, int max_alt_permille, long long *d_out, long long *d_scratch, hipStream_t s) {
    if (n_ranges <= 0 || n_total <= 0) return;
    int steps, shards; long long n_blocks;
    err_geometry(n_total, steps, n_blocks, shards);
    unsigned long long *d_parts = (unsigned long long *)(shards > 1 ? d_scratch : d_out);
    const int n_cells = ERR_CELLS * shards;
    hipLaunchKernelGGL(k_errprofile_init, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, s, d_parts, n_cells);
    hipLaunchKernelGGL(k_errprofile, dim3((unsigned)n_blocks), dim3(256), 0, s, *R, d_tab, n_ranges, (int)n_total, steps, shards, min_depth, max_alt_permille, d_parts);
    if (shards > 1) uvc_launch_sum_fold(d_scratch, shards, ERR_CELLS, d_out, s);
}
