// uvc_sitereads.hip -- uvcgpu_region_site_reads: the alignments of the handle that show something at a short list of sites, one 32-byte row
// per kept (alignment, site) observation and eight counts per site (the definitions are in uvcgpu.h).  Nothing here reads the
// planes: the inputs are the read columns of set_reads (RawReads), RegionDev::cigars / bq / refsym and the sorted site list.
//
// The work is proportional to the (alignment, site) ITEMS -- the listed sites inside [pos, endpos) of a counted alignment -- and is split by
// item, never by alignment or by site: a dense list over one 20 kb read and a hundred sites over two million short reads both fill the
// machine.
//   k_sr_span    one lane per alignment: two binary searches in the site list (staged in LDS when it has at most SR_LDS_SITES entries)
//                give the first candidate site and the number of candidates, 0 for an alignment that is not counted; the block's sum is
//                the tile sum of the scan, and one 64-bit add per tile keeps the true total (the 32-bit scan is refused above 2^31 - 1).
//   (uvc_launch_block_scan over the tile sums)
//   (uvc_launch_tile_prefix, in place: ipre[a] = the first item of alignment a, ipre[n_alns] = the number of items)
//   k_sr_items<false>  the COUNT pass.  A wave takes a run of consecutive items, whole 64-item steps; two wave-uniform binary searches in
//                ipre give the alignments of its first and last item, and a lane finds the alignment of its own item between the two.  A
//                lane walks its alignment's CIGAR to the op that holds the site and looks one step further for the events anchored there.
//                A lane's items of one alignment ascend, so the walk goes on where the lane's last item of that alignment left it: a lane
//                walks a CIGAR once, a 20 kb read costs 64 walks and not one per site.  The pass adds to counts[site][8] (integer atomics
//                whose results nobody reads) and leaves the number of kept rows of the wave's run.
//   (uvc_launch_block_scan over the waves' numbers; the host reads the total: sizes first)
//   k_sr_items<true>   the WRITE pass, launched only when the caller has room: the same walk; a kept row's rank is the wave's scanned base,
//                the kept rows of the earlier steps and a ballot over the lower lanes -- item order, which is (read, site) order.  A row
//                leaves as two 16-byte vector stores.
// Integer adds only, no LDS atomics, no scratch memory; the order of the rows depends on no atomic, two calls return the same bytes.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
#define SR_TILE UVC_SCAN_TILE   // alignments of one scan tile = threads of a block
#define SR_LDS_SITES 4096       // a list this long or shorter is searched in LDS (16 KiB)
#define SR_SPAN_BLOCKS 1024     // k_sr_span's blocks at most: each stages the list once and takes every SR_SPAN_BLOCKS-th tile
#define SR_MAX_BLOCKS 1024      // k_sr_items' blocks at most, four waves each

const char *const SR_KIND_NAMES[UVC_SITEREAD_NKIND] = { "A", "C", "G", "T", "N", "DEL" };
static_assert(sizeof(UvcSiteRead) == 32 && UVC_SITEREAD_NCOL == 8, "a row is eight int32, a site has eight counts");

// first[a], cnt[a]: the first candidate site of alignment a and the number of candidates; tile_sums[t]: the candidates of tile t; total:
// their 64-bit sum over all tiles (zero when the kernel starts)
template <bool LDS> __global__ void __launch_bounds__(SR_TILE) k_sr_span(RawReads W, int n_alns, const int32_t *sites, int n_sites, int min_mapq, int32_t *first, int32_t *cnt, int32_t *tile_sums,
                                                                           unsigned long long *total) {
    __shared__ int32_t sh_sites[LDS ? SR_LDS_SITES : 1];
    __shared__ long long sh_wave[SR_TILE / 64];
    const int tid = (int)threadIdx.x;
    if (LDS) { for (int j = tid; j < n_sites; j += SR_TILE) sh_sites[j] = sites[j]; __syncthreads(); }
    const int32_t *list = LDS ? sh_sites : sites;
    const int n_tiles = (n_alns + SR_TILE - 1) / SR_TILE;
    for (int t = (int)blockIdx.x; t < n_tiles; t += (int)gridDim.x) {
        const int a = t * SR_TILE + tid;
        int lo = 0, c = 0;
        if (a < n_alns && (int)W.mapq[a] >= min_mapq && W.l_qseq[a] > 0) {
            lo = first_ge(list, n_sites, W.pos[a]);
            c = first_ge(list, n_sites, W.endpos[a]) - lo;   // (endpos is behind the last reference position of the alignment: c >= 0)
        }
        if (a < n_alns) { first[a] = lo; cnt[a] = c; }
        const long long sum = waves_sum<SR_TILE / 64>(wave_sum((long long)c), sh_wave);
        if (tid == 0) { tile_sums[t] = (int32_t)sum; if (sum) atomicAdd(total, (unsigned long long)sum); }
        __syncthreads();   // sh_wave is written again in the next round
    }
}

// WRITE = false: counts and wave_rows[wave] = the kept rows of the wave's run; WRITE = true: wave_rows holds the exclusive prefix, the rows
// go to rows[]
template <bool WRITE> __global__ void __launch_bounds__(256) k_sr_items(RegionDev R, RawReads W, const int32_t *sites, const int32_t *first, const int32_t *ipre, int alt_only,
                                                                         const unsigned long long *total64, int32_t *counts, int32_t *wave_rows, UvcSiteRead *rows) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int n_alns = R.n_alns;
    const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (tid >> 6));
    const int n_waves = (int)gridDim.x * 4;
    const bool fits = (*total64 <= 0x7FFFFFFFull);   // (else the 32-bit scan wrapped: nothing of it is read, the host refuses the call)
    const int total = fits ? ipre[n_alns] : 0;
    const int per = (int)((((long long)total + n_waves - 1) / n_waves + 63) & ~63ll);   // whole steps of 64 items
    const long long i0 = (long long)wv * per, i1 = (i0 + per < total ? i0 + per : total);
    int kept = WRITE ? wave_rows[wv] : 0;   // WRITE: the rank of the next kept row
    if (i0 < i1) {
        // the last alignment whose first item is <= i holds item i (an alignment without items shares its entry with its successor)
        const int a_lo = last_le(ipre, 0, n_alns, (int)i0), a_hi = last_le(ipre, a_lo, n_alns, (int)(i1 - 1));
        // the walk of this lane: the alignment it is in, the op it stands in front of, that op's first query index and reference coordinate
        int cur = -1, j = 0, q = 0, p = 0, nc = 0, L = 0;
        long long so = 0, co = 0;
        for (long long ib = i0; ib < i1; ib += 64) {
            const bool have = (ib + lane < i1);
            const int i = have ? (int)(ib + lane) : 0;
            bool obs = false, keep = false;
            int a = 0, si = 0, kind = 0, qi = 0, qual = 0, ins_q = -1, ins_len = 0, del_len = 0;
            if (have) {
                a = last_le(ipre, a_lo, a_hi + 1, i);
                si = first[a] + (i - ipre[a]);
                const int s = sites[si];
                if (a != cur) { cur = a; j = 0; q = 0; p = W.pos[a]; nc = W.n_cigar[a]; L = W.l_qseq[a]; so = W.seq_off[a]; co = W.cigar_off[a]; }
                int op = C_PAD, len = 0;
                for (; j < nc; j++) {   // to the op that holds s: s >= p here, the sites of an alignment ascend
                    const uint32_t cg = R.cigars[co + j];
                    op = cig_op(cg); len = cig_len(cg);
                    const int rl = cig_ref(op) ? len : 0;
                    if (s - p < rl) break;
                    p += rl; q += cig_query(op) ? len : 0;
                }
                if (j < nc && op != C_REF_SKIP) {
                    obs = true;
                    const bool del = (op == C_DEL);
                    qi = del ? (q > 0 ? q - 1 : 0) : q + (s - p);
                    qi = qi < L ? qi : L - 1;   // (set_reads refuses a CIGAR whose query length is not l_qseq: never taken, and no load leaves the read)
                    const int v = (int)R.bq[so + qi], base = v & 0xFF;
                    qual = v >> 8;
                    kind = del ? UVC_SITEREAD_DEL : (base <= UVC_BASE_T ? base : UVC_SITEREAD_N);
                    if (s - p == len - 1) {   // the op ends at s: the events anchored here follow, up to the next op that moves p
                        int qn = q + (del ? 0 : len);
                        for (int jj = j + 1; jj < nc; jj++) {
                            const uint32_t cg = R.cigars[co + jj];
                            const int o = cig_op(cg), n = cig_len(cg);
                            if (o == C_INS) { if (ins_len == 0 && n > 0) ins_q = qn; ins_len += n; qn += n; }
                            else if (o == C_SOFT_CLIP) qn += n;
                            else if (o == C_DEL) { del_len += n; if (n > 0) break; }
                            else if (o == C_HARD_CLIP || o == C_PAD || n == 0) continue;
                            else break;
                        }
                    }
                    const long long x = (long long)s - R.beg;
                    const int ref = (x >= 0 && x < R.npos - 1) ? (int)R.refsym[x] : (int)UVC_BASE_N;   // (the region's last position holds no reference base)
                    keep = !alt_only || del || ins_len > 0 || del_len > 0 || (kind <= UVC_BASE_T && ref <= UVC_BASE_T && ref != kind);
                }
            }
            if (!WRITE) {
                if (obs) {
                    int32_t *c = counts + (size_t)si * UVC_SITEREAD_NCOL;
                    atomicAdd(c + kind, 1);
                    if (ins_len > 0) atomicAdd(c + UVC_SITEREAD_COL_INS, 1);
                    if (del_len > 0) atomicAdd(c + UVC_SITEREAD_COL_DEL_AFTER, 1);
                }
                kept += (int)__popcll(__ballot(keep));
            } else {
                const unsigned long long m = __ballot(keep);
                if (keep) {
                    int4 *dst = (int4 *)(rows + (size_t)kept + (size_t)__popcll(m & ((1ull << lane) - 1ull)));
                    dst[0] = make_int4(si, a, qi, kind | (qual << 8));
                    dst[1] = make_int4(ins_q, ins_len, del_len, 0);
                }
                kept += (int)__popcll(m);
            }
        }
    }
    if (!WRITE && lane == 0) wave_rows[wv] = kept;
}

// the blocks of the item passes: no more waves than 64-item steps of the most items the call can have
int sr_item_blocks(int64_t n_alns, int64_t n_sites) {
    const double most = (double)n_alns * (double)n_sites;
    return (int)std::max<double>(1, std::min<double>(SR_MAX_BLOCKS, (most + 255) / 256));
}
}   // namespace

extern "C" const char *uvc_sitereads_kind_name(int k) { return (k >= 0 && k < UVC_SITEREAD_NKIND) ? SR_KIND_NAMES[k] : nullptr; }
// ints of scratch of a call: [first candidate site per alignment] [first item per alignment, their number] [tile sums, their total]
// [kept rows per wave, their total]; two more for the 64-bit number of items in front of them all
extern "C" int64_t uvc_sitereads_scratch_ints(int64_t n_alns, int64_t n_sites) {
    return 2 + n_alns + (n_alns + 1) + (uvc_scan_tiles(n_alns) + 1) + ((int64_t)sr_item_blocks(n_alns, n_sites) * 4 + 1);
}
// where the host reads: the 64-bit number of items (scratch[0..1]) and the number of kept rows
extern "C" int64_t uvc_sitereads_rows_at(int64_t n_alns, int64_t n_sites) { return uvc_sitereads_scratch_ints(n_alns, n_sites) - 1; }

// The count: d_counts ([n_sites][8]) and the first two ints of d_scratch are zero at the start.  R->n_alns >= 1, n_sites >= 1.
extern "C" void uvc_launch_sitereads_count(const RegionDev *R, const RawReads *W, const int32_t *d_sites, int n_sites, const UvcSiteReadsRequest *req, int32_t *d_counts, int32_t *d_scratch, hipStream_t s) {
    const int n = R->n_alns;
    if (n <= 0 || n_sites <= 0) return;
    const int nt = (int)uvc_scan_tiles(n), nb = sr_item_blocks(n, n_sites);
    unsigned long long *total = (unsigned long long *)d_scratch;
    int32_t *first = d_scratch + 2, *ipre = first + n, *tsum = ipre + n + 1, *wrows = tsum + nt + 1;
    const unsigned sb = (unsigned)std::min(nt, SR_SPAN_BLOCKS);
    if (n_sites <= SR_LDS_SITES) hipLaunchKernelGGL(k_sr_span<true>, dim3(sb), dim3(SR_TILE), 0, s, *W, n, d_sites, n_sites, req->min_mapq, first, ipre, tsum, total);
    else hipLaunchKernelGGL(k_sr_span<false>, dim3(sb), dim3(SR_TILE), 0, s, *W, n, d_sites, n_sites, req->min_mapq, first, ipre, tsum, total);
    uvc_launch_block_scan(tsum, nt, s);
    uvc_launch_tile_prefix(ipre, n, 0, tsum, ipre, s);
    hipLaunchKernelGGL(k_sr_items<false>, dim3((unsigned)nb), dim3(256), 0, s, *R, *W, d_sites, first, ipre, req->alt_only, total, d_counts, wrows, (UvcSiteRead *)nullptr);
    uvc_launch_block_scan(wrows, nb * 4, s);
}
// after uvc_launch_sitereads_count with the same arguments; d_rows: room for the rows it counted
extern "C" void uvc_launch_sitereads_write(const RegionDev *R, const RawReads *W, const int32_t *d_sites, int n_sites, const UvcSiteReadsRequest *req, int32_t *d_scratch, UvcSiteRead *d_rows, hipStream_t s) {
    const int n = R->n_alns;
    if (n <= 0 || n_sites <= 0) return;
    const int nt = (int)uvc_scan_tiles(n), nb = sr_item_blocks(n, n_sites);
    int32_t *first = d_scratch + 2, *ipre = first + n, *wrows = ipre + n + 1 + nt + 1;   // (the layout of uvc_launch_sitereads_count)
    hipLaunchKernelGGL(k_sr_items<true>, dim3((unsigned)nb), dim3(256), 0, s, *R, *W, d_sites, first, ipre, req->alt_only, (const unsigned long long *)d_scratch, (int32_t *)nullptr, wrows, d_rows);
}
