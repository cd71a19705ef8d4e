// uvc_msi.hip -- uvcgpu_region_msi: the microsatellite loci of many ranges of the accumulated region, as the STR planes of UVC_F_RTR name
// them, with the smallest depths along each tract and a length-shift histogram per evidence level from the device InDel allele rows
// (the definitions are in uvcgpu.h, the row layout in include/uvc_msi.def).  The number of loci depends on the data: a count,
// a scan and an ordered compaction as in uvc_callable.hip, then two passes over what was compacted.
//   k_msi_heads   lanes walk the ranges laid end to end by compact position, read the three STR planes and count the block's locus heads.
//   (scan)        uvc_launch_block_scan: the exclusive prefix of the block counts, the number of loci behind them.
//   k_msi_emit    the same walk; a head ranks itself (ballot and popcount in a wave, LDS across the four waves, a running base across the
//                 steps, the scanned count across blocks) and writes its region-relative position into the head list and the five header
//                 words of its row; the rest of the rows was zeroed by the host's fill.  Loci come out sorted by head.
//   k_msi_depth   one wave per locus without EDGE: the lanes stride over the tract, 64 consecutive positions of every plane of the four
//                 measures per step, a wave minimum, lane 0 stores.  The loop is as long as the tract.
//   k_msi_bin     one lane per device allele row (the row count is read here, from RegionDev::gap.n_rows: the host never learns it): one or
//                 two STR reads name the head, a binary search in the head list finds the row, an insertion compares its bases with the
//                 reference, and up to four 32-bit vector atomics add the counters.  Rows are per distinct allele, not per read: a locus
//                 sees tens of adds, so there is no LDS stage.
// The kernels behind the scan read the number of loci from the device and leave what lies beyond `room` alone: the host learns the number
// after everything has run, and a call whose buffer was too small runs again with a larger one.  Integer arithmetic only; the adds commute.
#include "uvc_report_dev.h"

namespace {
enum {
#define UVC_MSI(name, first, words) MSI_##name,
#include "uvc_msi.def"
#undef UVC_MSI
    MSI_N
};
static_assert(MSI_N == UVC_NMSI, "include/uvc_msi.def and UvcMsiSection of uvcgpu.h list the same sections");
#define UVC_MSI(name, first, words) static_assert((int)MSI_##name == (int)UVC_MSI_##name, "uvc_msi.def order = UvcMsiSection order");
#include "uvc_msi.def"
#undef UVC_MSI
constexpr UvcSection MSI_SECTIONS[UVC_NMSI] = {
#define UVC_MSI(name, first, words) { #name, first, words },
#include "uvc_msi.def"
#undef UVC_MSI
};
static_assert(uvc_sections_tile(MSI_SECTIONS, UVC_MSI_ROW), "the sections of uvc_msi.def follow each other and fill UVC_MSI_ROW words");
#define MSI_W(section) (MSI_SECTIONS[MSI_##section].first)   // the first word of a section
static_assert(MSI_W(range) == 0 && MSI_W(pos_beg) == 1 && MSI_W(tracklen) == 2 && MSI_W(unitlen) == 3 && MSI_W(flags) == 4, "the header words k_msi_emit writes");
static_assert(MSI_W(depth) == UVC_MSI_DEPTH && MSI_SECTIONS[MSI_depth].words == UVC_MSI_NLEVEL && MSI_W(hist) == UVC_MSI_HIST && MSI_SECTIONS[MSI_hist].words == UVC_MSI_NLEVEL * UVC_MSI_NBIN, "depth[4] and hist[4][13]");
static_assert(UVC_MSI_NBIN == 2 * UVC_MSI_MAXSHIFT + 1 && UVC_MSI_OTHER == 2 * UVC_MSI_MAXSHIFT, "twelve shift bins and OTHER");
static_assert(sizeof(UvcMsiRequest) == 12, "the request goes into the kernel by value");

#define MSI_STEPS 4
#define MSI_TILE (256 * MSI_STEPS)   // compact positions of one block, as in uvc_callable.hip

// is plane index x the head of a locus of the request?  (x in [0, npos))
DEV bool msi_head(const RegionDev &R, const UvcMsiRequest &q, int64_t x, int &tl, int &ul) {
    tl = 0; ul = 0;
    if (RTRP(R, UVC_RTR_begpos, x) != (int)x) return false;
    tl = RTRP(R, UVC_RTR_tracklen, x); ul = RTRP(R, UVC_RTR_unitlen, x);
    return ul >= 1 && ul <= q.max_unitlen && tl >= q.min_tracklen && tl / ul >= q.min_units;
}

__global__ void __launch_bounds__(256) k_msi_heads(RegionDev R, const UvcRangeRow *tab, int n_ranges, int n_total, UvcMsiRequest q, int *block_count) {
    __shared__ int wave_heads[4];
    const long long base = (long long)blockIdx.x * MSI_TILE;
    UvcRangeCursor g;
    int heads = 0;   // wave-uniform
#pragma unroll
    for (int c = 0; c < MSI_STEPS; c++) {
        const long long i = base + c * 256 + threadIdx.x;
        bool head = false;
        if (i < n_total) {
            uvc_range_find(g, tab, n_ranges, i);
            int tl, ul;
            head = msi_head(R, q, (int64_t)g.x0 + (i - g.first), tl, ul);   // (inside [0, npos): the host has checked every range against the region)
        }
        heads += __popcll(__ballot(head));
    }
    const int block_heads = waves_sum<4>(heads, wave_heads);
    if (threadIdx.x == 0) block_count[blockIdx.x] = block_heads;
}

__global__ void __launch_bounds__(256) k_msi_emit(RegionDev R, const UvcRangeRow *tab, int n_ranges, int n_total, UvcMsiRequest q, const int *block_off, int32_t *heads_out, int32_t *rows, int room) {
    __shared__ int wave_heads[4];
    const long long base = (long long)blockIdx.x * MSI_TILE;
    UvcRangeCursor g;
    int locus_base = block_off[blockIdx.x];   // the heads in front of this step's first position
#pragma unroll
    for (int c = 0; c < MSI_STEPS; c++) {
        const long long i = base + c * 256 + threadIdx.x;
        bool head = false; int x = 0, tl = 0, ul = 0;
        if (i < n_total) {
            uvc_range_find(g, tab, n_ranges, i);
            x = g.x0 + (int)(i - g.first);
            head = msi_head(R, q, x, tl, ul);
        }
        int step_heads;
        const int idx = locus_base + head_rank(head, wave_heads, step_heads) - 1;   // (of a head) the heads in front of this one
        if (head && idx < room) {
            heads_out[idx] = x;
            int32_t *row = rows + (size_t)idx * UVC_MSI_ROW;
            // the tract holds the first or the last reference base of the region (position npos - 1 has none): the cut may have truncated it
            const bool edge = (x == 0 || (int64_t)x + tl >= R.npos - 1);
            row[MSI_W(range)] = g.rid; row[MSI_W(pos_beg)] = R.beg + x; row[MSI_W(tracklen)] = tl; row[MSI_W(unitlen)] = ul;
            row[MSI_W(flags)] = edge ? UVC_MSI_EDGE : 0;
        }
        locus_base += step_heads;
        __syncthreads();   // wave_heads is written again in the next step
    }
}

// grid-stride over the loci, one wave each; n_loci_dev: the scanned total
__global__ void __launch_bounds__(256) k_msi_depth(RegionDev R, const int *n_loci_dev, int32_t *rows, int room) {
    const int lane = (int)(threadIdx.x & 63);
    const int n = imin(*n_loci_dev, room);
    const int waves = (int)gridDim.x * 4;
    for (int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); i < n; i += waves) {   // (i is wave-uniform)
        int32_t *row = rows + (size_t)i * UVC_MSI_ROW;
        if (row[MSI_W(flags)] & UVC_MSI_EDGE) continue;
        const int64_t h = row[MSI_W(pos_beg)] - R.beg, end = lmin(h + row[MSI_W(tracklen)], R.npos);   // (a track ends at the last reference base at the latest)
        int d0 = INT32_MAX, d1 = INT32_MAX, d2 = INT32_MAX, d3 = INT32_MAX;
        for (int64_t x = h + lane; x < end; x += 64) {
            d0 = imin(d0, cov_FRAG(R, UVC_FRAG_bDP, x));
            d1 = imin(d1, cov_FAM(R, UVC_FAM_cDP12, x));
            d2 = imin(d2, cov_FAM(R, UVC_FAM_cDP2, x));
            d3 = imin(d3, cov_DUPLEX(R, UVC_DUPLEX_dDP1, x));
        }
        d0 = wave_min(d0); d1 = wave_min(d1); d2 = wave_min(d2); d3 = wave_min(d3);
        if (lane == 0) { int32_t *d = row + UVC_MSI_DEPTH; d[0] = d0; d[1] = d1; d[2] = d2; d[3] = d3; }   // (tracklen >= 1: every minimum has seen a position)
    }
}

// the index of head h in the ascending list, -1 when it is not there
DEV int msi_find(const int32_t *heads, int n, int h) {
    const int lo = first_ge(heads, n, h);
    return (lo < n && heads[lo] == h) ? lo : -1;
}

__global__ void __launch_bounds__(256) k_msi_bin(RegionDev R, const int *n_loci_dev, const int32_t *heads, int32_t *rows, int room) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= imin(*R.gap.n_rows, R.gap.n_ev)) return;
    const int n = imin(*n_loci_dev, room);
    const GapRow g = R.gap.rows[i];
    int c[UVC_MSI_NLEVEL] = { 0, 0, 0, 0 };
#pragma unroll
    for (int sd = 0; sd < 2; sd++)
        if (g.cnt[sd * 4] > 0) {   // a strand without fragment support has no row in the public tables (gap_tables of uvc_host.cpp)
#pragma unroll
            for (int l = 0; l < UVC_MSI_NLEVEL; l++) c[l] += g.cnt[sd * 4 + l];
        }
    const bool ins = is_ins(g.sym), del = is_del(g.sym);
    if ((c[0] | c[1] | c[2] | c[3]) == 0 || !(ins || del) || g.len < 1 || g.x < 0 || (int64_t)g.x >= R.npos) return;
    int h = RTRP(R, UVC_RTR_begpos, g.x);
    int idx = msi_find(heads, n, h);
    if (ins && idx < 0 && g.x > 0) {   // behind the last unit of the locus in front
        h = RTRP(R, UVC_RTR_begpos, g.x - 1);
        idx = msi_find(heads, n, h);
        if (idx >= 0 && h + rows[(size_t)idx * UVC_MSI_ROW + MSI_W(tracklen)] != g.x) idx = -1;
    }
    if (idx < 0) return;
    int32_t *row = rows + (size_t)idx * UVC_MSI_ROW;
    if (row[MSI_W(flags)] & UVC_MSI_EDGE) return;
    const int tl = row[MSI_W(tracklen)], ul = row[MSI_W(unitlen)];
    bool unit_shift = (g.len % ul == 0);
    if (del) unit_shift = unit_shift && ((int64_t)g.x + g.len <= (int64_t)h + tl);
    else {
        unit_shift = unit_shift && g.seq_off >= 0;
        const int phase = g.x - h;   // (>= 0 on both paths; h + (..) % ul < h + tl: a reference base of the region)
        for (int k = 0; unit_shift && k < g.len; k++) unit_shift = (R.gap.seq[g.seq_off + k] == R.refsym[h + (phase + k) % ul]);
    }
    const int units = imin(g.len / ul, UVC_MSI_MAXSHIFT);
    const int bin = !unit_shift ? UVC_MSI_OTHER : (del ? UVC_MSI_MAXSHIFT - units : UVC_MSI_MAXSHIFT - 1 + units);
#pragma unroll
    for (int l = 0; l < UVC_MSI_NLEVEL; l++) if (c[l] != 0) atomicAdd(row + UVC_MSI_HIST + l * UVC_MSI_NBIN + bin, c[l]);
}
}   // namespace

extern "C" const char *uvc_msi_name(int id) { return (id >= 0 && id < UVC_NMSI) ? MSI_SECTIONS[id].name : nullptr; }
extern "C" int64_t uvc_msi_blocks(int64_t n_total) { return (n_total + MSI_TILE - 1) / MSI_TILE; }
extern "C" void uvc_launch_msi(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int64_t n_total, const UvcMsiRequest *req, int *d_blocks, int32_t *d_heads, int32_t *d_rows, int64_t room, hipStream_t s) {
    if (n_ranges <= 0 || n_total <= 0) return;
    const int n_blocks = (int)uvc_msi_blocks(n_total);
    hipLaunchKernelGGL(k_msi_heads, dim3((unsigned)n_blocks), dim3(256), 0, s, *R, d_tab, n_ranges, (int)n_total, *req, d_blocks);
    uvc_launch_block_scan(d_blocks, n_blocks, s);
    if (room <= 0) return;
    const int rm = (int)(room < INT32_MAX ? room : INT32_MAX);
    hipLaunchKernelGGL(k_msi_emit, dim3((unsigned)n_blocks), dim3(256), 0, s, *R, d_tab, n_ranges, (int)n_total, *req, d_blocks, d_heads, d_rows, rm);
    const int64_t depth_blocks = (room + 3) / 4;
    hipLaunchKernelGGL(k_msi_depth, dim3((unsigned)(depth_blocks < 16384 ? depth_blocks : 16384)), dim3(256), 0, s, *R, d_blocks + n_blocks, d_rows, rm);
    if (R->gap.n_ev > 0 && R->gap.n_rows) hipLaunchKernelGGL(k_msi_bin, dim3((unsigned)((R->gap.n_ev + 255) / 256)), dim3(256), 0, s, *R, d_blocks + n_blocks, d_heads, d_rows, rm);
}
