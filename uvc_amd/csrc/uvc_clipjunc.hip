// uvc_clipjunc.hip -- uvcgpu_region_clip_junctions: where the clipped consensus of each clip site lies on the region's reference, on which
// strand, how unique that is, and which other site is the far end of the event (the definitions are in uvcgpu.h).  The inputs
// are RegionDev::refsym and the caller's site rows (pos, side, VOTE); no read and no plane is touched.
//   k_cj_pack     once per call: the reference as 2-bit codes, 32 positions per 64-bit word, and beside it the "not a base" mask (bit 2 i of
//                 a word: position i of the word is no A/C/G/T or lies behind the reference).  Two words of "not a base" follow the last.
//   k_cj_queries  one lane per site: winner, total and the compare rule per vote index, then for each of the two strands a 64-bit query
//                 word and compare mask laid out so that the placement is "query against the forward window that starts at w": the query
//                 is reversed where d k runs downward and complemented for the reverse strand; toff / poff map w back to t and to the
//                 partner.  The lane also sets the site's best key to all ones and its hist to zero.
//   k_cj_search   the hot kernel.  A lane owns one window start: it builds its window and its invalid mask once from two packed words and
//                 loops over the sites that have a window to compare (a ballot per 64 sites names them), whose query rows are wave-uniform loads.  Per (window, site, strand): XOR, fold the two bits of a
//                 base, OR the invalid mask, AND the compare mask, popcount.  Only a count <= max_mismatch leaves that path: the max_dist
//                 test on the mapped partner, one hist add, one 64-bit atomicMin over (mismatches, strand, t).
//   k_cj_finish   one lane per site: the row from the best key and hist; the mate by first_ge over the positions of the expected side.
// With UVC_CLIPJUNC_NAIVE the search is the form the packed one is measured against and tested with: one byte per base, a loop over k
// straight from refsym for every (t, site, strand).  Integer adds and one min per counted placement, whose results nobody reads back before
// the kernel ends: two calls return the same bytes.  No scratch memory.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
enum {
#define UVC_CLIPJUNC(name, first, words) CJROW_##name,
#include "uvc_clipjunc.def"
#undef UVC_CLIPJUNC
    CJROW_N
};
static_assert(CJROW_N == UVC_NCLIPJUNC, "include/uvc_clipjunc.def and UvcClipJuncSection of uvcgpu.h list the same sections");
#define UVC_CLIPJUNC(name, first, words) static_assert((int)CJROW_##name == (int)UVC_CLIPJUNC_##name, "uvc_clipjunc.def order = UvcClipJuncSection order");
#include "uvc_clipjunc.def"
#undef UVC_CLIPJUNC
constexpr UvcSection CJ_SECTIONS[UVC_NCLIPJUNC] = {
#define UVC_CLIPJUNC(name, first, words) { #name, first, words },
#include "uvc_clipjunc.def"
#undef UVC_CLIPJUNC
};
static_assert(uvc_sections_tile(CJ_SECTIONS, UVC_CLIPJUNC_ROW), "the sections of uvc_clipjunc.def tile the row");
static_assert(CJ_SECTIONS[UVC_CLIPJUNC_hist].words == UVC_CLIPJUNC_NHIST && UVC_CLIPSITE_NCONS == 32, "hist has a bin per mismatch count 0..7; a query fits one 64-bit word of 2-bit codes");
enum {
#define UVC_CLIPSITE(name, first, words) CJ_SITE_##name = first,
#include "uvc_clipsites.def"
#undef UVC_CLIPSITE
};
const char *const CJ_CLASSES[UVC_NCLIPCLASS] = { "NONE", "DEL", "DUP", "INV", "ADJACENT" };

#define CJ_WORD(section) (CJ_SECTIONS[UVC_CLIPJUNC_##section].first)
#define CJ_BLOCK 256
#define CJ_MAX_BLOCKS 4096       // blocks over the window starts at most (a lane strides over the rest)
typedef unsigned long long u64;

// what the search knows of a site.  Variant v = strand: q[v] / c[v] are the query and compare mask against the forward window at w (bits
// 2 i, 2 i + 1: the code that faces window position i; bit 2 i of c: position i is compared), t = w + toff[v], partner = w + poff[v].
// wmax: the last window start whose query_len positions lie inside the reference, negative when there is none or the site is not searched.
struct CjSite {
    u64 q[2], c[2];
    int wmax, len, cmp, x, side, toff[2], poff[2];
    unsigned char b[UVC_CLIPSITE_NCONS];   // the naive form's query: winner per k, 255 where k is not compared
    int searched;
};
static_assert(sizeof(CjSite) % 8 == 0, "a site's query row is read as 64-bit words");

// the 2-bit groups of v in reverse order
DEV u64 cj_reverse2(u64 v) {
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(v);
}
DEV u64 cj_key(int mm, int strand, int t) { return ((u64)mm << 40) | ((u64)strand << 32) | (u64)(unsigned)t; }
// the partner's plane index from t: + 1 where side and strand agree in number (LEFT forward, RIGHT reverse)
DEV int cj_partner_add(int side, int strand) { return 1 - (side ^ strand); }

// ref2 / inv: nw words each (uvc_clipjunc_ref_words); a lane makes one word of both
__global__ void __launch_bounds__(CJ_BLOCK) k_cj_pack(const uint8_t *refsym, int n, int nw, u64 *ref2, u64 *inv) {
    const int j = (int)(blockIdx.x * CJ_BLOCK + threadIdx.x);
    if (j >= nw) return;
    u64 codes = 0, bad = 0;
    for (int i = 0; i < 32; i++) {
        const long long x = 32ll * j + i;
        const int c = (x < n) ? (int)refsym[x] : (int)UVC_BASE_N;
        if (c <= UVC_BASE_T) codes |= (u64)c << (2 * i); else bad |= 1ull << (2 * i);
    }
    ref2[j] = codes; inv[j] = bad;
}

// rows: the caller's site rows; n: reference positions.  S, best and hist are written for every site
__global__ void __launch_bounds__(CJ_BLOCK) k_cj_queries(const long long *rows, int n_sites, int n, long long beg, int min_votes, int min_len, CjSite *S, u64 *best, unsigned *hist) {
    const int s = (int)(blockIdx.x * CJ_BLOCK + threadIdx.x);
    if (s >= n_sites) return;
    const long long *row = rows + (size_t)s * UVC_CLIPSITE_ROW;
    const int side = (int)row[CJ_SITE_side];
    u64 qa = 0, ca = 0;   // ascending: bits of k at 2 k
    int len = 0, cmp = 0;
    CjSite &o = S[s];
    for (int k = 0; k < UVC_CLIPSITE_NCONS; k++) {
        const long long *v = row + CJ_SITE_VOTE + k * UVC_CLIPSITE_NCODE;
        long long total = 0, top = v[0]; int win = 0;
#pragma unroll
        for (int c = 0; c < UVC_CLIPSITE_NCODE; c++) { total += v[c]; if (v[c] > top) { top = v[c]; win = c; } }
        if (total >= 1) len = k + 1;
        const bool on = (total >= min_votes && win <= UVC_BASE_T && top * 3 >= total * 2);
        if (on) { qa |= (u64)win << (2 * k); ca |= 1ull << (2 * k); cmp++; }
        o.b[k] = on ? (unsigned char)win : (unsigned char)255;
    }
    const bool searched = (cmp >= min_len);
    // descending: the code of k at window position len - 1 - k
    const u64 qd = len > 0 ? cj_reverse2(qa) >> (64 - 2 * len) : 0, cd = len > 0 ? cj_reverse2(ca) >> (64 - 2 * len) : 0;
    // forward runs upward for a RIGHT site (d = +1) and downward for a LEFT site; the reverse strand the other way round, complemented
    const bool fwd_up = (side == UVC_CLIPSITE_RIGHT);
    o.q[0] = fwd_up ? qa : qd;                o.c[0] = fwd_up ? ca : cd;
    o.q[1] = (fwd_up ? qd : qa) ^ (3 * (fwd_up ? cd : ca)); o.c[1] = fwd_up ? cd : ca;
    o.toff[0] = fwd_up ? 0 : len - 1;         o.toff[1] = fwd_up ? len - 1 : 0;
    o.poff[0] = o.toff[0] + cj_partner_add(side, 0); o.poff[1] = o.toff[1] + cj_partner_add(side, 1);
    o.wmax = searched ? n - len : -1;
    o.len = len; o.cmp = cmp; o.x = (int)(row[CJ_SITE_pos] - beg); o.side = side; o.searched = searched;
    best[s] = ~0ull;
#pragma unroll
    for (int m = 0; m < UVC_CLIPJUNC_NHIST; m++) hist[(size_t)s * UVC_CLIPJUNC_NHIST + m] = 0;
}

// a placement of site s with mm <= max_mismatch mismatches: counted unless its partner lies further than max_dist from the site
DEV void cj_count(const CjSite &S, int s, int mm, int strand, int t, int partner, int max_dist, u64 *best, unsigned *hist) {
    const int dist = partner > S.x ? partner - S.x : S.x - partner;
    if (max_dist > 0 && dist > max_dist) return;
    atomicAdd(hist + (size_t)s * UVC_CLIPJUNC_NHIST + mm, 1u);
    atomicMin(best + s, cj_key(mm, strand, t));
}

// blockIdx.y takes the sites [y per, (y + 1) per): a short reference with many sites still fills the device.  Both forms walk the sites
// 64 at a time: every lane looks at one site of the group, a ballot names those with a window to compare, and the wave loops over these
// alone -- a list of a hundred thousand single-read sites, none of them searched, costs a load and a ballot per 64.  The loops over the
// window starts and over the groups are block-uniform, so whole waves make the ballots.
#ifndef UVC_CLIPJUNC_NAIVE
__global__ void __launch_bounds__(CJ_BLOCK) k_cj_search(const u64 *__restrict__ ref2, const u64 *__restrict__ inv, int n, const CjSite *__restrict__ S, int n_sites, int per, int max_mm, int max_dist, u64 *__restrict__ best,
                                                        unsigned *__restrict__ hist) {
    const int s0 = (int)blockIdx.y * per, s1 = imin(n_sites, s0 + per), lane = (int)(threadIdx.x & 63);
    for (long long b = (long long)blockIdx.x * CJ_BLOCK; b < n; b += (long long)gridDim.x * CJ_BLOCK) {
        const long long w = b + threadIdx.x;   // (a lane behind the reference has w > wmax of every site)
        u64 win = 0, bad = ~0ull;
        if (w < n) {
            const int j = (int)(w >> 5), sh = 2 * (int)(w & 31);
            win = ref2[j]; bad = inv[j];   // (words j and j + 1 exist: two words follow the last position's)
            if (sh) { win = (win >> sh) | (ref2[j + 1] << (64 - sh)); bad = (bad >> sh) | (inv[j + 1] << (64 - sh)); }
        }
        for (int sb = s0; sb < s1; sb += 64) {
            u64 live = __ballot(sb + lane < s1 && S[sb + lane].wmax >= 0);
            while (live) {   // (s is wave-uniform: the site's row comes through the scalar cache)
                const int s = sb + __ffsll((long long)live) - 1;
                live &= live - 1;
                const CjSite &Q = S[s];
                if (w > Q.wmax) continue;
#pragma unroll
                for (int v = 0; v < 2; v++) {
                    const u64 x = win ^ Q.q[v];
                    const int mm = __popcll(((x | (x >> 1)) | bad) & Q.c[v]);
                    if (mm <= max_mm) cj_count(Q, s, mm, v, (int)w + Q.toff[v], (int)w + Q.poff[v], max_dist, best, hist);
                }
            }
        }
    }
}
#else
// the naive form: a lane owns one t and compares byte by byte, straight from the definition
__global__ void __launch_bounds__(CJ_BLOCK) k_cj_search(const uint8_t *__restrict__ refsym, int n, const CjSite *__restrict__ S, int n_sites, int per, int max_mm, int max_dist, u64 *__restrict__ best, unsigned *__restrict__ hist) {
    const int s0 = (int)blockIdx.y * per, s1 = imin(n_sites, s0 + per), lane = (int)(threadIdx.x & 63);
    for (long long b = (long long)blockIdx.x * CJ_BLOCK; b < n; b += (long long)gridDim.x * CJ_BLOCK) {
        const long long t = b + threadIdx.x;
        for (int sb = s0; sb < s1; sb += 64) {
            u64 live = __ballot(sb + lane < s1 && S[sb + lane].searched != 0);
            while (live) {
                const int s = sb + __ffsll((long long)live) - 1;
                live &= live - 1;
                const CjSite &Q = S[s];
                if (t >= n) continue;
                const int d = (Q.side == UVC_CLIPSITE_RIGHT) ? 1 : -1;
                for (int strand = 0; strand < 2; strand++) {
                    const int e = strand ? -d : d;
                    const long long last = t + (long long)e * (Q.len - 1);
                    if (last < 0 || last >= n) continue;
                    int mm = 0;
                    for (int k = 0; k < Q.len; k++) {
                        if (Q.b[k] == 255) continue;
                        const int r = (int)refsym[t + e * k];
                        if (r > UVC_BASE_T || (strand ? 3 - r : r) != (int)Q.b[k]) mm++;
                    }
                    if (mm <= max_mm) cj_count(Q, s, mm, strand, (int)t, (int)t + cj_partner_add(Q.side, strand), max_dist, best, hist);
                }
            }
        }
    }
}
#endif

// mpos: the plane indices of the LEFT sites ascending, behind them ([n_left, n_sites)) those of the RIGHT sites; midx: their rows
__global__ void __launch_bounds__(CJ_BLOCK) k_cj_finish(const CjSite *S, int n_sites, long long beg, int mate_slop, const u64 *best, const unsigned *hist, const int32_t *mpos, const int32_t *midx, int n_left,
                                                        long long *rows) {
    const int s = (int)(blockIdx.x * CJ_BLOCK + threadIdx.x);
    if (s >= n_sites) return;
    const CjSite &Q = S[s];
    long long *row = rows + (size_t)s * UVC_CLIPJUNC_ROW;
    const u64 key = best[s];
    const bool searched = (Q.searched != 0), placed = searched && key != ~0ull;
    row[CJ_WORD(site)] = s; row[CJ_WORD(query_len)] = Q.len; row[CJ_WORD(cmp_len)] = Q.cmp;
    row[CJ_WORD(status)] = placed ? UVC_CLIPJUNC_PLACED : searched ? UVC_CLIPJUNC_NOT_PLACED : UVC_CLIPJUNC_NOT_SEARCHED;
    long long best_mm = -1, n_best = 0, second = -1, partner = -1, strand = -1, klass = UVC_CLIPCLASS_NONE, len = -1, mate = -1;
    if (placed) {
        best_mm = (long long)(key >> 40); strand = (long long)((key >> 32) & 1);
        const int t = (int)(unsigned)key, px = t + cj_partner_add(Q.side, (int)strand);
        n_best = hist[(size_t)s * UVC_CLIPJUNC_NHIST + best_mm];
        if (n_best >= 2) second = best_mm;
        else for (int m = (int)best_mm + 1; m < UVC_CLIPJUNC_NHIST && second < 0; m++) if (hist[(size_t)s * UVC_CLIPJUNC_NHIST + m]) second = m;
        partner = (long long)px + beg;
        len = px > Q.x ? px - Q.x : Q.x - px;
        if (strand) klass = UVC_CLIPCLASS_INV;
        else if (px == Q.x) klass = UVC_CLIPCLASS_ADJACENT;
        else klass = ((px > Q.x) == (Q.side == UVC_CLIPSITE_RIGHT)) ? UVC_CLIPCLASS_DEL : UVC_CLIPCLASS_DUP;
        // the mate: the nearest site of the expected side (forward: the other side, reverse: the same), the smaller pos of two equally near
        const int want = strand ? Q.side : 1 - Q.side;
        const int lo = want == UVC_CLIPSITE_LEFT ? 0 : n_left, hi = want == UVC_CLIPSITE_LEFT ? n_left : n_sites;
        const int i = lo + first_ge(mpos + lo, hi - lo, px);
        long long dist = (long long)mate_slop + 1;
        if (i < hi && (long long)mpos[i] - px < dist) { dist = (long long)mpos[i] - px; mate = midx[i]; }
        if (i > lo && (long long)px - mpos[i - 1] <= dist && (long long)px - mpos[i - 1] <= mate_slop) mate = midx[i - 1];
    }
    row[CJ_WORD(best_mm)] = best_mm; row[CJ_WORD(n_best)] = n_best; row[CJ_WORD(second_mm)] = second; row[CJ_WORD(partner)] = partner;
    row[CJ_WORD(strand)] = strand; row[CJ_WORD(klass)] = klass; row[CJ_WORD(len)] = len; row[CJ_WORD(mate)] = mate;
#pragma unroll
    for (int m = 0; m < UVC_CLIPJUNC_NHIST; m++) row[CJ_WORD(hist) + m] = searched ? (long long)hist[(size_t)s * UVC_CLIPJUNC_NHIST + m] : 0;
#pragma unroll
    for (int m = 0; m < CJ_SECTIONS[UVC_CLIPJUNC_reserved].words; m++) row[CJ_WORD(reserved) + m] = 0;
}

unsigned cj_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + CJ_BLOCK - 1) / CJ_BLOCK); }
}   // namespace

extern "C" const char *uvc_clipjunc_name(int id) { return (id >= 0 && id < UVC_NCLIPJUNC) ? CJ_SECTIONS[id].name : nullptr; }
extern "C" const char *uvc_clipjunc_class_name(int k) { return (k >= 0 && k < UVC_NCLIPCLASS) ? CJ_CLASSES[k] : nullptr; }
extern "C" int uvc_clipjunc_naive(void) {
#ifdef UVC_CLIPJUNC_NAIVE
    return 1;
#else
    return 0;
#endif
}
// 64-bit words of each of the two packed arrays: one per 32 reference positions and two more, so that the window of every start has a
// second word
extern "C" int64_t uvc_clipjunc_ref_words(int64_t npos) { return (npos - 1 + 31) / 32 + 2; }
extern "C" int64_t uvc_clipjunc_query_bytes(int64_t n_sites) { return (int64_t)sizeof(CjSite) * n_sites; }

extern "C" void uvc_launch_clipjunc_pack(const RegionDev *R, unsigned long long *d_ref2, unsigned long long *d_inv, hipStream_t s) {
#ifndef UVC_CLIPJUNC_NAIVE   // (the naive form reads refsym itself)
    const int nw = (int)uvc_clipjunc_ref_words(R->npos);
    hipLaunchKernelGGL(k_cj_pack, dim3(cj_blocks(nw)), dim3(CJ_BLOCK), 0, s, R->refsym, (int)(R->npos - 1), nw, d_ref2, d_inv);
#endif
}
extern "C" void uvc_launch_clipjunc_queries(const RegionDev *R, const long long *d_sites, int n_sites, const UvcClipJunctionsRequest *req, void *d_query, unsigned long long *d_best, unsigned *d_hist, hipStream_t s) {
    hipLaunchKernelGGL(k_cj_queries, dim3(cj_blocks(n_sites)), dim3(CJ_BLOCK), 0, s, d_sites, n_sites, (int)(R->npos - 1), (long long)R->beg, req->min_votes, req->min_len, (CjSite *)d_query, d_best, d_hist);
}
extern "C" void uvc_launch_clipjunc_search(const RegionDev *R, const unsigned long long *d_ref2, const unsigned long long *d_inv, const void *d_query, int n_sites, const UvcClipJunctionsRequest *req,
                                           unsigned long long *d_best, unsigned *d_hist, hipStream_t s) {
    const int n = (int)(R->npos - 1);
    if (n <= 0 || n_sites <= 0) return;
    const unsigned bx = std::min<unsigned>(cj_blocks(n), CJ_MAX_BLOCKS);
    // enough blocks for the device where the reference is short: the sites in up to 2048 / bx groups
    const int groups = (int)std::max<int64_t>(1, std::min<int64_t>(n_sites, 2048 / bx)), per = (n_sites + groups - 1) / groups;
    const dim3 grid(bx, (unsigned)((n_sites + per - 1) / per));
#ifndef UVC_CLIPJUNC_NAIVE
    hipLaunchKernelGGL(k_cj_search, grid, dim3(CJ_BLOCK), 0, s, d_ref2, d_inv, n, (const CjSite *)d_query, n_sites, per, req->max_mismatch, req->max_dist, d_best, d_hist);
#else
    hipLaunchKernelGGL(k_cj_search, grid, dim3(CJ_BLOCK), 0, s, R->refsym, n, (const CjSite *)d_query, n_sites, per, req->max_mismatch, req->max_dist, d_best, d_hist);
#endif
}
extern "C" void uvc_launch_clipjunc_finish(const RegionDev *R, const void *d_query, int n_sites, const UvcClipJunctionsRequest *req, const unsigned long long *d_best, const unsigned *d_hist,
                                           const int32_t *d_mpos, const int32_t *d_midx, int n_left, long long *d_rows, hipStream_t s) {
    hipLaunchKernelGGL(k_cj_finish, dim3(cj_blocks(n_sites)), dim3(CJ_BLOCK), 0, s, (const CjSite *)d_query, n_sites, (long long)R->beg, req->mate_slop, d_best, d_hist, d_mpos, d_midx, n_left, d_rows);
}
