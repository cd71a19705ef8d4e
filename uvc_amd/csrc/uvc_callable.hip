// uvc_callable.hip -- uvcgpu_region_callable: the runs of equal callability masks of many ranges of the accumulated planes (DESIGN.md 4l;
// the definitions are in uvcgpu.h, the bits in include/uvc_callable.def).  The output's length depends on the data, so this is a
// classification, a count, a scan and an ordered compaction, not a reduction into fixed rows.
//
// The ranges are laid end to end and the work is split by compact position, never by range, as k_coverage splits it: a lane owns one
// compact position per step, finds its range by a search in the prefix table (and keeps it while its positions stay inside), and a wave
// instruction reads 64 consecutive positions of a plane.  A block takes CALL_TILE consecutive compact positions.
//   k_callable_count  reads the cells of the measures the request tests (aDP always: NO_COVERAGE needs it), forms the mask, stores it as one
//                     byte per compact position and counts the block's run heads.  A position is a head when it is the first of its range or
//                     its mask differs from the mask of the position before it; that mask comes from the lane to the left, and a lane 0
//                     that does not start a range RECOMPUTES the mask of the position before the wave's first (one lane in 64 reads twice).
//   (scan)            uvc_launch_block_scan, one block: the exclusive prefix of the block counts in place, their total (the number of runs) behind them.
//   k_callable_emit   reads the mask bytes (its own, both neighbours'), ranks the heads -- ballot and popcount in a wave, LDS across the four
//                     waves, a running base across the steps, the scanned count across blocks -- and writes the runs in order: a head
//                     writes { range, pos_beg, mask } of its run, the last position of a run writes its pos_end.
// No workgroup waits on another, nothing is atomic, every store is a plain vector store; the bytes are the same from call to call.  The host
// reads the number of runs between scan and emit, so a call whose caller has too little room launches no emit.
#include "uvc_report_dev.h"

namespace {
enum {
#define UVC_CALLBIT(name) CALLBIT_##name,
#include "uvc_callable.def"
#undef UVC_CALLBIT
    CALLBIT_N
};
static_assert(CALLBIT_N == UVC_NCALLBIT, "include/uvc_callable.def and UvcCallableBit of uvcgpu.h list the same bits");
#define UVC_CALLBIT(name) static_assert((int)CALLBIT_##name == (int)UVC_CALL_##name, "uvc_callable.def order = UvcCallableBit order");
#include "uvc_callable.def"
#undef UVC_CALLBIT
#define UVC_COV(name, group, plane) static_assert((int)UVC_CALL_LOW_##name == (int)UVC_COV_##name, "bit k of a mask is LOW_<measure k of uvc_coverage.def>");
#include "uvc_coverage.def"
#undef UVC_COV
static_assert((int)UVC_CALL_EXCESS_aDP == (int)UVC_NCOV && (int)UVC_CALL_NO_COVERAGE == (int)UVC_NCOV + 1 && (int)UVC_NCALLBIT == (int)UVC_NCOV + 2, "the two aDP bits follow the LOW bits of all measures");
static_assert(UVC_NCALLBIT <= 8, "a mask is stored as one byte per position");
static_assert(sizeof(UvcCallableRun) == 16 && sizeof(UvcCallableRequest) == 4 * (UVC_NCOV + 1), "runs leave as 16-byte rows; the request goes into the kernel by value");

const char *const CALL_NAMES[UVC_NCALLBIT] = {
#define UVC_CALLBIT(name) #name,
#include "uvc_callable.def"
#undef UVC_CALLBIT
};

#define CALL_STEPS 4
#define CALL_TILE (256 * CALL_STEPS)   // compact positions of one block: 1 024 blocks (4 096 waves) on a 1 Mb tile

// The mask of plane index x.  Which measures are tested is uniform for the launch: the branches are scalar, and an untested measure
// costs no plane read.
DEV int call_mask(const RegionDev &R, const UvcCallableRequest &q, int64_t x) {
    int mask = 0;
#define UVC_COV(name, group, plane) \
    if (UVC_COV_##name == UVC_COV_aDP || q.min_depth[UVC_COV_##name] > 0) { \
        const int v = cov_##group(R, plane, x); \
        if (q.min_depth[UVC_COV_##name] > 0 && v < q.min_depth[UVC_COV_##name]) mask |= 1 << UVC_CALL_LOW_##name; \
        if (UVC_COV_##name == UVC_COV_aDP) mask |= (q.max_aDP > 0 && v > q.max_aDP ? 1 << UVC_CALL_EXCESS_aDP : 0) | (v == 0 ? 1 << UVC_CALL_NO_COVERAGE : 0); \
    }
#include "uvc_coverage.def"
#undef UVC_COV
    return mask;
}

__global__ void __launch_bounds__(256) k_callable_count(RegionDev R, const UvcRangeRow *tab, int n_ranges, int n_total, UvcCallableRequest q, unsigned char *mask_out, int *block_count) {
    __shared__ int wave_heads[4];
    const int lane = (int)(threadIdx.x & 63);
    const long long base = (long long)blockIdx.x * CALL_TILE;
    UvcRangeCursor g;
    int heads = 0;   // wave-uniform
#pragma unroll
    for (int c = 0; c < CALL_STEPS; c++) {
        const long long i = base + c * 256 + threadIdx.x;
        const bool act = (i < n_total);
        int m = 0; bool first = false; int64_t x = 0;
        if (act) {
            uvc_range_find(g, tab, n_ranges, i);
            x = (int64_t)g.x0 + (i - g.first);   // (inside [0, npos): the host has checked every range against the region)
            first = (i == g.first);
            m = call_mask(R, q, x);
        }
        int left = __shfl_up(m, 1, 64);   // (the previous lane's mask: a neighbour fetch, not a scan step)
        if (act && lane == 0 && !first) left = call_mask(R, q, x - 1);   // the position before the wave's first, of the same range
        const bool head = act && (first || left != m);
        if (act) mask_out[i] = (unsigned char)m;
        heads += __popcll(__ballot(head));
    }
    const int block_heads = waves_sum<4>(heads, wave_heads);
    if (threadIdx.x == 0) block_count[blockIdx.x] = block_heads;
}

__global__ void __launch_bounds__(256) k_callable_emit(const UvcRangeRow *tab, int n_ranges, int n_total, int region_beg, const unsigned char *mask, const int *block_off, UvcCallableRun *runs) {
    __shared__ int wave_heads[4];
    const long long base = (long long)blockIdx.x * CALL_TILE;
    UvcRangeCursor g;
    int run_base = block_off[blockIdx.x];   // the heads in front of this step's first position
#pragma unroll
    for (int c = 0; c < CALL_STEPS; c++) {
        const long long i = base + c * 256 + threadIdx.x;
        const bool act = (i < n_total);
        int m = 0, pos = 0; bool head = false, tail = false;
        if (act) {
            uvc_range_find(g, tab, n_ranges, i);
            pos = region_beg + g.x0 + (int)(i - g.first);
            m = mask[i];
            head = (i == g.first || mask[i - 1] != m);
            tail = (i + 1 == g.next || mask[i + 1] != m);   // (g.next <= n_total: i + 1 is read only inside the range)
        }
        int step_heads;
        // the run this position lies in: the heads up to and including it, less one (position 0 of the call is a head, so never below 0)
        const int idx = run_base + head_rank(head, wave_heads, step_heads) - 1;
        if (head) { runs[idx].range = g.rid; runs[idx].pos_beg = pos; runs[idx].mask = m; }
        if (tail) runs[idx].pos_end = pos + 1;
        run_base += step_heads;
        __syncthreads();   // wave_heads is written again in the next step
    }
}
}   // namespace

extern "C" const char *uvc_callable_name(int bit) { return (bit >= 0 && bit < UVC_NCALLBIT) ? CALL_NAMES[bit] : nullptr; }
extern "C" int64_t uvc_callable_blocks(int64_t n_total) { return (n_total + CALL_TILE - 1) / CALL_TILE; }
// d_tab: n_ranges + 1 rows; d_mask: n_total bytes; d_blocks: uvc_callable_blocks(n_total) + 1 ints, the last one receives the number of runs
extern "C" void uvc_launch_callable_count(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const UvcCallableRequest *req, unsigned char *d_mask, int *d_blocks, hipStream_t s) {
    if (n_ranges <= 0 || n_total <= 0) return;
    const int n_blocks = (int)uvc_callable_blocks(n_total);
    hipLaunchKernelGGL(k_callable_count, dim3((unsigned)n_blocks), dim3(256), 0, s, *R, d_tab, n_ranges, (int)n_total, *req, d_mask, d_blocks);
    uvc_launch_block_scan(d_blocks, n_blocks, s);
}
// after uvc_launch_callable_count with the same arguments; d_runs: room for d_blocks[n_blocks] runs
extern "C" void uvc_launch_callable_emit(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const unsigned char *d_mask, const int *d_blocks, UvcCallableRun *d_runs, hipStream_t s) {
    if (n_ranges <= 0 || n_total <= 0) return;
    hipLaunchKernelGGL(k_callable_emit, dim3((unsigned)uvc_callable_blocks(n_total)), dim3(256), 0, s, d_tab, n_ranges, (int)n_total, R->beg, d_mask, d_blocks, d_runs);
}
