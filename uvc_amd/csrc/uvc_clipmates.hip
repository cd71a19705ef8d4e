// uvc_clipmates.hip -- uvcgpu_region_clip_mates: the read pairs that face each given clip site, their classes, and the clusters the mates of
// the discordant ones form (the definitions are in uvcgpu.h).  The inputs are the read columns of set_reads (RawReads: pos,
// endpos, mpos, flag, mapq, l_qseq), the caller's mtid column and the site lists the host lays out (the positions of the LEFT sites
// ascending, behind them those of the RIGHT sites, and the row each belongs to); no CIGAR, no base and no plane is touched.
//   k_cm_count    one lane per alignment: the sites it faces are a stretch of one of the two lists (cm_stretch); per item +1 into the
//                 site row's class counter and, for a witness, +1 into the site's witness count; the four totals per block in LDS.  The
//                 alignments come sorted by position, so the lanes of a wave mostly face the same sites: the wave takes the t-th item
//                 of every lane per round, groups the lanes by site and class with ballots and makes one add per group (cm_count_add).
//   k_cm_blocks   one lane per site: the 256-witness blocks the rank kernel gives the site.
//   (uvc_launch_tile_sums / _block_scan / _tile_prefix over the witness counts and over the block counts: every site's segment of the
//   witness array, the number of witnesses, every site's first rank block, their number)
// The host reads the four totals and the two numbers; a call with fewer than 2^31 facing items and at least one witness goes on:
//   k_cm_scatter  the walk again: a witness goes into its site's segment at a slot taken with an atomic cursor (one add per group of lanes
//                 with the same site, cm_take_slots), as its 64-bit key
//                 mt << 33 | strand << 32 | (mpos with the sign bit flipped: signed order as unsigned order) and its read index.  This order
//                 is arbitrary and nobody outside the call reads it.
//   k_cm_rank     a block takes up to 256 witnesses of ONE site (a site with more takes several blocks), loops over the site's segment in
//                 tiles of 256 staged in LDS and counts, per witness, those with a smaller (key, read): its final slot.  Quadratic per site.
//   k_cm_cut      one lane per ranked witness: its site, and "begins a cluster".
//   (the tile scan over the flags numbers the clusters)
//   k_cm_reduce   one lane per ranked witness: integer adds into its cluster's counters, one per group of lanes with the same cluster
//                 (neighbours in witness order share theirs); the head of a cluster writes site, mtid, strand,
//                 mpos_min and first, its last witness mpos_max (the witnesses of a cluster ascend by mpos: no min or max is computed), and
//                 +1 into the site's `clusters`.
//   k_cm_keep     one lane per cluster: kept iff pairs >= min_pairs.
//   (the tile scan over the kept flags: the index of every kept cluster among the returned rows, their number)
//   k_cm_emit     one lane per cluster: a kept one copies its row behind its scanned index and adds 1 to its site's `clusters_kept`.
//   k_cm_reads    one lane per witness: its UvcClipMate row (want_reads).
// Integer adds whose results nobody reads before the kernel ends, no scratch memory; the order of witnesses, clusters and rows is decided
// by the keys alone: two calls return the same bytes.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
enum {
#define UVC_CLIPMATE_SITE(name, first, words) CMSITE_##name,
#define UVC_CLIPMATE_CLUSTER(name, first, words)
#include "uvc_clipmates.def"
#undef UVC_CLIPMATE_SITE
#undef UVC_CLIPMATE_CLUSTER
    CMSITE_N
};
enum {
#define UVC_CLIPMATE_SITE(name, first, words)
#define UVC_CLIPMATE_CLUSTER(name, first, words) CMCLUS_##name,
#include "uvc_clipmates.def"
#undef UVC_CLIPMATE_SITE
#undef UVC_CLIPMATE_CLUSTER
    CMCLUS_N
};
static_assert(CMSITE_N == UVC_NCLIPMSITE && CMCLUS_N == UVC_NCLIPMCLUS, "include/uvc_clipmates.def and the two word enums of uvcgpu.h list the same words");
#define UVC_CLIPMATE_SITE(name, first, words) static_assert((int)CMSITE_##name == (int)UVC_CLIPMSITE_##name, "uvc_clipmates.def order = UvcClipMateSiteWord order");
#define UVC_CLIPMATE_CLUSTER(name, first, words) static_assert((int)CMCLUS_##name == (int)UVC_CLIPMCLUS_##name, "uvc_clipmates.def order = UvcClipMateClusterWord order");
#include "uvc_clipmates.def"
#undef UVC_CLIPMATE_SITE
#undef UVC_CLIPMATE_CLUSTER
constexpr UvcSection CM_SITE_WORDS[UVC_NCLIPMSITE] = {
#define UVC_CLIPMATE_SITE(name, first, words) { #name, first, words },
#define UVC_CLIPMATE_CLUSTER(name, first, words)
#include "uvc_clipmates.def"
#undef UVC_CLIPMATE_SITE
#undef UVC_CLIPMATE_CLUSTER
};
constexpr UvcSection CM_CLUSTER_WORDS[UVC_NCLIPMCLUS] = {
#define UVC_CLIPMATE_SITE(name, first, words)
#define UVC_CLIPMATE_CLUSTER(name, first, words) { #name, first, words },
#include "uvc_clipmates.def"
#undef UVC_CLIPMATE_SITE
#undef UVC_CLIPMATE_CLUSTER
};
static_assert(uvc_sections_tile(CM_SITE_WORDS, UVC_CLIPMATE_SITE_ROW) && uvc_sections_tile(CM_CLUSTER_WORDS, UVC_CLIPMATE_ROW), "the words of uvc_clipmates.def tile the two rows");
static_assert(UVC_CLIPMSITE_concordant + UVC_CLIPMATE_OTHER_CONTIG == UVC_CLIPMSITE_other_contig && UVC_CLIPMSITE_concordant + UVC_CLIPMATE_FAR == UVC_CLIPMSITE_far
              && UVC_CLIPMCLUS_pairs + UVC_CLIPMATE_OTHER_CONTIG == UVC_CLIPMCLUS_other_contig && UVC_CLIPMCLUS_pairs + UVC_CLIPMATE_FAR == UVC_CLIPMCLUS_far,
              "the class counters of both rows follow each other in class order");
static_assert(sizeof(UvcClipMate) == 16 && sizeof(UvcClipMatesRequest) == 32 && UVC_CLIPMATE_NTOTAL == 8, "a witness row is four int32, the request eight");
const char *const CM_CLASSES[UVC_NCLIPMATECLASS] = { "CONCORDANT", "OTHER_CONTIG", "SAME_STRAND", "FAR" };

#define CM_BLOCK 256            // threads of every block; witnesses of one rank block and of one LDS tile
#define CM_MAX_BLOCKS 1024      // blocks of the passes over the alignments at most
typedef unsigned long long u64;

// what the kernels know of a call: the request and the two site lists (spos: the absolute positions of the n_left LEFT sites ascending, then
// those of the RIGHT sites; sidx: their rows)
struct CmCall { const int32_t *spos, *sidx, *mtid; int n_sites, n_left, tid, min_mapq, window, overhang, min_dist, max_gap, min_pairs; };

// the alignment as the definitions read it
struct CmRead { bool pair; int pos, rend, mpos, flag, mapq, mt; };
DEV CmRead cm_read(const RawReads &W, const CmCall &Q, int a) {
    CmRead v;
    v.flag = (int)W.flag[a]; v.mapq = (int)W.mapq[a]; v.pos = W.pos[a]; v.rend = W.endpos[a]; v.mpos = W.mpos[a];
    v.mt = Q.mtid ? Q.mtid[a] : Q.tid;
    v.pair = (v.mapq >= Q.min_mapq && (v.flag & 0x4) == 0 && W.l_qseq[a] > 0 && (v.flag & 0x1) && !(v.flag & 0x8) && !(v.flag & 0x900) && v.mt >= 0);
    return v;
}
DEV int cm_class(const CmRead &v, const CmCall &Q) {
    if (v.mt != Q.tid) return UVC_CLIPMATE_OTHER_CONTIG;
    if (((v.flag >> 5) & 1) == ((v.flag >> 4) & 1)) return UVC_CLIPMATE_SAME_STRAND;
    const long long d = (long long)v.mpos - v.pos;
    return (d < 0 ? -d : d) >= Q.min_dist ? UVC_CLIPMATE_FAR : UVC_CLIPMATE_CONCORDANT;
}
// The sites a pair read faces: entries [j0, j1) of the list.  A forward read faces the RIGHT sites p with pos < p and rend - overhang <= p
// < rend + window; a reverse read the LEFT sites p with pos - window < p <= pos + overhang and p < rend.  64-bit bounds: window and
// overhang are any int32.
DEV void cm_stretch(const CmRead &v, const CmCall &Q, int &j0, int &j1) {
    const bool rev = (v.flag & 0x10) != 0;
    long long lo, hi;   // p in [lo, hi)
    if (!rev) { const long long a = (long long)v.pos + 1, b = (long long)v.rend - Q.overhang; lo = a > b ? a : b; hi = (long long)v.rend + Q.window; }
    else { const long long a = (long long)v.pos + Q.overhang + 1, b = (long long)v.rend; lo = (long long)v.pos - Q.window + 1; hi = a < b ? a : b; }
    const int base = rev ? 0 : Q.n_left, n = rev ? Q.n_left : Q.n_sites - Q.n_left;
    j0 = j1 = base;
    if (lo >= hi || n == 0 || lo > INT_MAX || hi <= INT_MIN) return;
    j0 = base + first_ge(Q.spos + base, n, lo < INT_MIN ? INT_MIN : (int)lo);
    j1 = hi > INT_MAX ? base + n : base + first_ge(Q.spos + base, n, (int)hi);
    if (j1 < j0) j1 = j0;
}
DEV u64 cm_key(const CmRead &v) { return ((u64)(unsigned)v.mt << 33) | ((u64)((v.flag >> 5) & 1) << 32) | (u64)((unsigned)v.mpos ^ 0x80000000u); }
DEV int cm_key_mpos(u64 key) { return (int)((unsigned)key ^ 0x80000000u); }

// ---- adds into global words that many lanes of a wave meet on: the alignments come sorted by position and the witnesses by key, so the
// lanes of a wave mostly name the same site or cluster.  The lanes with `on` are grouped by key (one ballot round per distinct key among
// them) and the group's first lane makes one add for all of it.  Every lane of the wave makes the call.
// tab[key] += 1 per lane; T = u64 or int
template <class T> DEV void cm_count_add(T *tab, long long key, bool on, int lane) {
    u64 left = __ballot(on);
    while (left) {
        const int lead = __ffsll((long long)left) - 1;
        const long long k = __shfl(key, lead);
        const u64 same = __ballot(on && key == k);
        if (lane == lead) atomicAdd(tab + k, (T)__popcll(same));
        left &= ~same;
    }
}
// tab[key] += v per lane
DEV void cm_sum_add(u64 *tab, long long key, u64 v, bool on, int lane) {
    u64 left = __ballot(on);
    while (left) {
        const int lead = __ffsll((long long)left) - 1;
        const long long k = __shfl(key, lead);
        const bool mine = on && key == k;
        const u64 sum = wave_sum(mine ? v : 0ull);
        if (lane == lead) atomicAdd(tab + k, sum);
        left &= ~__ballot(mine);
    }
}
// the slot of every lane with `on` in the segment its cursor counts: the group's first lane takes the group's slots with one add, a lane's
// slot is the base + the group's lanes in front of it (-1 without `on`)
DEV int cm_take_slots(int32_t *cursor, int key, bool on, int lane) {
    u64 left = __ballot(on);
    int slot = -1;
    while (left) {
        const int lead = __ffsll((long long)left) - 1;
        const int k = __shfl(key, lead);
        const u64 same = __ballot(on && key == k);
        int base = 0;
        if (lane == lead) base = atomicAdd(cursor + k, __popcll(same));
        base = __shfl(base, lead);
        if (on && key == k) slot = base + __popcll(same & ((1ull << lane) - 1ull));
        left &= ~same;
    }
    return slot;
}

// rows: n_sites rows of UVC_CLIPMATE_SITE_ROW words (the class counters are added here, `facing` is their sum: the host's) and wcnt: n_sites ints, zero at the start; totals[0..3] (zero at the start)
__global__ void __launch_bounds__(CM_BLOCK) k_cm_count(RawReads W, long long n_alns, CmCall Q, u64 *rows, int32_t *wcnt, u64 *totals) {
    __shared__ u64 tot[4];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < 4) tot[tid] = 0;
    __syncthreads();
    for (long long a0 = (long long)blockIdx.x * CM_BLOCK; a0 < n_alns; a0 += (long long)gridDim.x * CM_BLOCK) {
        const long long a = a0 + tid;
        bool pair = false;
        u64 n_face = 0, n_conc = 0;
        int j0 = 0, j1 = 0, k = UVC_CLIPMATE_CONCORDANT;
        if (a < n_alns) {
            const CmRead v = cm_read(W, Q, (int)a);
            pair = v.pair;
            if (pair) {
                cm_stretch(v, Q, j0, j1);
                if (j1 > j0) {   // (the class of an item does not depend on the site)
                    k = cm_class(v, Q);
                    n_face = (u64)(j1 - j0); n_conc = (k == UVC_CLIPMATE_CONCORDANT) ? n_face : 0;
                }
            }
        }
        // the items of the wave's lanes, one per lane and round: the t-th site of every lane's stretch (the rounds are wave-uniform)
        const int rounds = wave_max(j1 - j0);
        for (int t = 0; t < rounds; t++) {
            const bool on = (j0 + t < j1);
            const int s = on ? Q.sidx[j0 + t] : 0;
            cm_count_add(rows, (long long)s * UVC_CLIPMATE_SITE_ROW + UVC_CLIPMSITE_concordant + k, on, lane);
            cm_count_add(wcnt, (long long)s, on && k != UVC_CLIPMATE_CONCORDANT, lane);
        }
        count_lanes(tot + UVC_CLIPMTOTAL_pair_reads, pair, lane);
        const u64 s_face = wave_sum(n_face), s_conc = wave_sum(n_conc);
        if (lane == 0 && s_face) {
            lds_add(tot + UVC_CLIPMTOTAL_facing, s_face);
            if (s_conc) lds_add(tot + UVC_CLIPMTOTAL_concordant, s_conc);
            if (s_face > s_conc) lds_add(tot + UVC_CLIPMTOTAL_discordant, s_face - s_conc);
        }
    }
    __syncthreads();
    if (tid < 4 && tot[tid]) atomicAdd(totals + tid, tot[tid]);
}

__global__ void __launch_bounds__(CM_BLOCK) k_cm_blocks(const int32_t *wcnt, int n_sites, int32_t *bcnt) {
    const int s = (int)(blockIdx.x * CM_BLOCK + threadIdx.x);
    if (s < n_sites) bcnt[s] = (int)(((long long)wcnt[s] + CM_BLOCK - 1) / CM_BLOCK);
}

// woff: the scanned witness counts; cursor: n_sites ints, zero at the start; key / read: the witness array in scatter order
__global__ void __launch_bounds__(CM_BLOCK) k_cm_scatter(RawReads W, long long n_alns, CmCall Q, const int32_t *woff, int32_t *cursor, u64 *key, int32_t *read) {
    const int lane = (int)(threadIdx.x & 63);
    for (long long a0 = (long long)blockIdx.x * CM_BLOCK; a0 < n_alns; a0 += (long long)gridDim.x * CM_BLOCK) {   // (whole waves make the rounds)
        const long long a = a0 + threadIdx.x;
        int j0 = 0, j1 = 0;
        u64 k = 0;
        if (a < n_alns) {
            const CmRead v = cm_read(W, Q, (int)a);
            if (v.pair && cm_class(v, Q) != UVC_CLIPMATE_CONCORDANT) { cm_stretch(v, Q, j0, j1); k = cm_key(v); }
        }
        const int rounds = wave_max(j1 - j0);
        for (int t = 0; t < rounds; t++) {
            const bool on = (j0 + t < j1);
            const int s = on ? Q.sidx[j0 + t] : 0;
            const int at = cm_take_slots(cursor, s, on, lane);
            if (on) { const int slot = woff[s] + at; key[slot] = k; read[slot] = (int)a; }   // (slot < woff[s + 1]: the count pass counted this item)
        }
    }
}

// boff: the scanned block counts of the sites (n_sites + 1 entries); block b takes witnesses [256 c, 256 c + 256) of the site s with
// boff[s] <= b < boff[s + 1], c = b - boff[s].  key / read: scatter order; okey / oread: witness order
__global__ void __launch_bounds__(CM_BLOCK) k_cm_rank(const int32_t *woff, const int32_t *boff, int n_sites, const u64 *key, const int32_t *read, u64 *okey, int32_t *oread) {
    __shared__ u64 sh_key[CM_BLOCK];
    __shared__ int32_t sh_read[CM_BLOCK];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int s = last_le(boff, 0, n_sites, b);   // (block-uniform; the sites without a witness have no block)
    const int w0 = woff[s], w1 = woff[s + 1], mine = w0 + (b - boff[s]) * CM_BLOCK + tid;
    const bool have = (mine < w1);
    const u64 k = have ? key[mine] : 0;
    const int rd = have ? read[mine] : 0;
    int rank = 0;
    for (int t0 = w0; t0 < w1; t0 += CM_BLOCK) {
        const int n = imin(CM_BLOCK, w1 - t0);
        if (tid < n) { sh_key[tid] = key[t0 + tid]; sh_read[tid] = read[t0 + tid]; }
        __syncthreads();
        if (have) {
            for (int j = 0; j < n; j++) {   // (j is block-uniform: the LDS reads are broadcasts)
                const u64 kj = sh_key[j];
                rank += (kj < k || (kj == k && sh_read[j] < rd)) ? 1 : 0;
            }
        }
        __syncthreads();   // the tile is written again in the next round
    }
    if (have) { okey[w0 + rank] = k; oread[w0 + rank] = rd; }   // (a permutation of the segment: (key, read) is total inside a site)
}

// okey: witness order.  wsite[i]: the site of witness i; head[i]: 1 where it begins a cluster
__global__ void __launch_bounds__(CM_BLOCK) k_cm_cut(const int32_t *woff, int n_sites, int n_wit, const u64 *okey, int max_gap, int32_t *wsite, int32_t *head) {
    const int i = (int)(blockIdx.x * CM_BLOCK + threadIdx.x);
    if (i >= n_wit) return;
    const int s = last_le(woff, 0, n_sites, i);
    bool h = (i == woff[s]);
    if (!h) {
        const u64 k = okey[i], p = okey[i - 1];
        h = ((k >> 32) != (p >> 32)) || ((long long)cm_key_mpos(k) - cm_key_mpos(p) > max_gap);
    }
    wsite[i] = s; head[i] = h ? 1 : 0;
}

// cnum: the scanned heads (n_wit + 1 entries): witness i lies in cluster cnum[i] + head[i] - 1.  crow: n_clus rows of UVC_CLIPMATE_ROW
// words, zero at the start; rows: the site rows
__global__ void __launch_bounds__(CM_BLOCK) k_cm_reduce(RawReads W, CmCall Q, int n_wit, const u64 *okey, const int32_t *oread, const int32_t *wsite, const int32_t *head, const int32_t *cnum,
                                                        u64 *crow, u64 *rows, int32_t *wclus, int32_t *wklass) {
    const int i = (int)(blockIdx.x * CM_BLOCK + threadIdx.x), lane = (int)(threadIdx.x & 63);
    const bool on = (i < n_wit);
    const int c = on ? cnum[i] + head[i] - 1 : 0, a = on ? oread[i] : 0;
    CmRead v; v.mapq = 0;
    int k = UVC_CLIPMATE_OTHER_CONTIG;
    if (on) { v = cm_read(W, Q, a); k = cm_class(v, Q); }
    const long long at = (long long)c * UVC_CLIPMATE_ROW;
    cm_count_add(crow, at + UVC_CLIPMCLUS_pairs, on, lane);
    cm_count_add(crow, at + UVC_CLIPMCLUS_pairs + k, on, lane);
    cm_sum_add(crow, at + UVC_CLIPMCLUS_mapq_sum, (u64)v.mapq, on, lane);
    if (!on) return;
    const int s = wsite[i];
    u64 *row = crow + at;
    const u64 key = okey[i];
    if (head[i]) {
        row[UVC_CLIPMCLUS_site] = (u64)s; row[UVC_CLIPMCLUS_mtid] = key >> 33; row[UVC_CLIPMCLUS_mate_strand] = (key >> 32) & 1;
        row[UVC_CLIPMCLUS_mpos_min] = (u64)(long long)cm_key_mpos(key); row[UVC_CLIPMCLUS_first] = (u64)i;
        atomicAdd(rows + (size_t)s * UVC_CLIPMATE_SITE_ROW + UVC_CLIPMSITE_clusters, 1ull);
    }
    if (i == n_wit - 1 || head[i + 1]) row[UVC_CLIPMCLUS_mpos_max] = (u64)(long long)cm_key_mpos(key);
    wclus[i] = c; wklass[i] = k;
}

__global__ void __launch_bounds__(CM_BLOCK) k_cm_keep(const u64 *crow, int n_clus, int min_pairs, int32_t *kept) {
    const int c = (int)(blockIdx.x * CM_BLOCK + threadIdx.x);
    if (c < n_clus) kept[c] = (crow[(size_t)c * UVC_CLIPMATE_ROW + UVC_CLIPMCLUS_pairs] >= (u64)min_pairs) ? 1 : 0;
}

// knum: the scanned kept flags; out: room for the kept rows
__global__ void __launch_bounds__(CM_BLOCK) k_cm_emit(const u64 *crow, int n_clus, const int32_t *kept, const int32_t *knum, u64 *out, u64 *rows) {
    const int c = (int)(blockIdx.x * CM_BLOCK + threadIdx.x);
    if (c >= n_clus || !kept[c]) return;
    const u64 *row = crow + (size_t)c * UVC_CLIPMATE_ROW;
    u64 *o = out + (size_t)knum[c] * UVC_CLIPMATE_ROW;
#pragma unroll
    for (int w = 0; w < UVC_CLIPMATE_ROW; w++) o[w] = row[w];
    atomicAdd(rows + (size_t)row[UVC_CLIPMCLUS_site] * UVC_CLIPMATE_SITE_ROW + UVC_CLIPMSITE_clusters_kept, 1ull);
}

__global__ void __launch_bounds__(CM_BLOCK) k_cm_reads(int n_wit, const int32_t *oread, const int32_t *wsite, const int32_t *wclus, const int32_t *wklass, const int32_t *kept, const int32_t *knum, UvcClipMate *out) {
    const int i = (int)(blockIdx.x * CM_BLOCK + threadIdx.x);
    if (i >= n_wit) return;
    const int c = wclus[i];
    out[i] = UvcClipMate{ wsite[i], oread[i], kept[c] ? knum[c] : -1, wklass[i] };
}

unsigned cm_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + CM_BLOCK - 1) / CM_BLOCK); }
CmCall cm_call(const UvcClipMateLists *L, const UvcClipMatesRequest *req) {
    return CmCall{ L->spos, L->sidx, L->mtid, L->n_sites, L->n_left, req->tid, req->min_mapq, req->window, req->overhang, req->min_dist, req->max_gap, req->min_pairs };
}
// the tile scan of the shared header over n ints: d_out[i] = the sum in front of i, d_out[n] the total (d_tiles: uvc_scan_tiles(n) + 1 ints)
void cm_scan(const int32_t *d_in, int n, int32_t *d_tiles, int32_t *d_out, hipStream_t s) {
    uvc_launch_tile_sums(d_in, n, 0, d_tiles, s);
    uvc_launch_block_scan(d_tiles, (int)uvc_scan_tiles(n), s);
    uvc_launch_tile_prefix(d_in, n, 0, d_tiles, d_out, s);
}
}   // namespace

extern "C" const char *uvc_clipmates_site_name(int id) { return (id >= 0 && id < UVC_NCLIPMSITE) ? CM_SITE_WORDS[id].name : nullptr; }
extern "C" const char *uvc_clipmates_cluster_name(int id) { return (id >= 0 && id < UVC_NCLIPMCLUS) ? CM_CLUSTER_WORDS[id].name : nullptr; }
extern "C" const char *uvc_clipmates_class_name(int k) { return (k >= 0 && k < UVC_NCLIPMATECLASS) ? CM_CLASSES[k] : nullptr; }
extern "C" int64_t uvc_clipmates_site_ints(int64_t n_sites) { return 4 * (n_sites + 1) + 2 * (uvc_scan_tiles(n_sites) + 1); }
extern "C" int64_t uvc_clipmates_witness_ints(int64_t n_wit) { return 6 * (n_wit + 1) + uvc_scan_tiles(n_wit) + 1; }

extern "C" void uvc_launch_clipmates_count(const RawReads *W, int64_t n_alns, const UvcClipMateLists *L, const UvcClipMatesRequest *req, long long *d_rows, long long *d_totals, int32_t *d_site_ints, hipStream_t s) {
    const int n = L->n_sites;
    int32_t *wcnt = d_site_ints, *woff = wcnt + (n + 1), *bcnt = woff + (n + 1), *boff = bcnt + (n + 1), *tiles = boff + (n + 1);
    const unsigned blocks = std::min<unsigned>(cm_blocks(n_alns), CM_MAX_BLOCKS);
    hipLaunchKernelGGL(k_cm_count, dim3(blocks), dim3(CM_BLOCK), 0, s, *W, (long long)n_alns, cm_call(L, req), (u64 *)d_rows, wcnt, (u64 *)d_totals);
    hipLaunchKernelGGL(k_cm_blocks, dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, s, wcnt, n, bcnt);
    cm_scan(wcnt, n, tiles, woff, s);
    cm_scan(bcnt, n, tiles + uvc_scan_tiles(n) + 1, boff, s);
}
extern "C" const int32_t *uvc_clipmates_n_witnesses_at(const int32_t *d_site_ints, int64_t n_sites) { return d_site_ints + (n_sites + 1) + n_sites; }
extern "C" const int32_t *uvc_clipmates_n_rank_blocks_at(const int32_t *d_site_ints, int64_t n_sites) { return d_site_ints + 3 * (n_sites + 1) + n_sites; }

extern "C" void uvc_launch_clipmates_scatter(const RawReads *W, int64_t n_alns, const UvcClipMateLists *L, const UvcClipMatesRequest *req, int32_t *d_site_ints, int n_wit,
                                             unsigned long long *d_key, int32_t *d_wit_ints, hipStream_t s) {
    const int n = L->n_sites;
    int32_t *woff = d_site_ints + (n + 1), *cursor = woff + (n + 1);   // (the block counts are read no more: their array is the cursor)
    hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)n, s);
    const unsigned blocks = std::min<unsigned>(cm_blocks(n_alns), CM_MAX_BLOCKS);
    hipLaunchKernelGGL(k_cm_scatter, dim3(blocks), dim3(CM_BLOCK), 0, s, *W, (long long)n_alns, cm_call(L, req), woff, cursor, d_key, d_wit_ints);
}
extern "C" void uvc_launch_clipmates_rank(const UvcClipMateLists *L, const int32_t *d_site_ints, int n_wit, int n_rank_blocks, const unsigned long long *d_key, unsigned long long *d_okey,
                                          int32_t *d_wit_ints, hipStream_t s) {
    const int n = L->n_sites;
    hipLaunchKernelGGL(k_cm_rank, dim3((unsigned)n_rank_blocks), dim3(CM_BLOCK), 0, s, d_site_ints + (n + 1), d_site_ints + 3 * (n + 1), n, (const u64 *)d_key, d_wit_ints, (u64 *)d_okey, d_wit_ints + (n_wit + 1));
}
extern "C" void uvc_launch_clipmates_cut(const UvcClipMateLists *L, const UvcClipMatesRequest *req, const int32_t *d_site_ints, int n_wit, const unsigned long long *d_okey, int32_t *d_wit_ints, hipStream_t s) {
    const int n = L->n_sites;
    int32_t *wsite = d_wit_ints + 2 * (n_wit + 1), *head = wsite + (n_wit + 1), *cnum = head + (n_wit + 1), *tiles = d_wit_ints + 6 * (n_wit + 1);
    hipLaunchKernelGGL(k_cm_cut, dim3(cm_blocks(n_wit)), dim3(CM_BLOCK), 0, s, d_site_ints + (n + 1), n, n_wit, d_okey, req->max_gap, wsite, head);
    cm_scan(head, n_wit, tiles, cnum, s);
}
extern "C" const int32_t *uvc_clipmates_n_clusters_at(const int32_t *d_wit_ints, int64_t n_wit) { return d_wit_ints + 4 * (n_wit + 1) + n_wit; }

// d_crow: n_clus rows, zero at the start; behind the call entry uvc_clipmates_n_kept_at of d_clus_ints (uvc_clipmates_cluster_ints(n_clus)
// ints) holds the number of kept clusters, d_out (room for n_clus rows) the kept rows and d_reads (or NULL) the witness rows
extern "C" void uvc_launch_clipmates_reduce(const RawReads *W, const UvcClipMateLists *L, const UvcClipMatesRequest *req, int n_wit, int n_clus, const unsigned long long *d_okey, int32_t *d_wit_ints,
                                            long long *d_crow, long long *d_rows, long long *d_out, UvcClipMate *d_reads, int32_t *d_clus_ints, hipStream_t s) {
    int32_t *oread = d_wit_ints + (n_wit + 1), *wsite = oread + (n_wit + 1), *head = wsite + (n_wit + 1), *cnum = head + (n_wit + 1), *wclus = cnum + (n_wit + 1);
    int32_t *wklass = d_wit_ints;   // (the read indices in scatter order are read no more)
    int32_t *kept = d_clus_ints, *knum = kept + (n_clus + 1), *tiles = knum + (n_clus + 1);
    hipLaunchKernelGGL(k_cm_reduce, dim3(cm_blocks(n_wit)), dim3(CM_BLOCK), 0, s, *W, cm_call(L, req), n_wit, (const u64 *)d_okey, oread, wsite, head, cnum, (u64 *)d_crow, (u64 *)d_rows, wclus, wklass);
    hipLaunchKernelGGL(k_cm_keep, dim3(cm_blocks(n_clus)), dim3(CM_BLOCK), 0, s, (const u64 *)d_crow, n_clus, req->min_pairs, kept);
    cm_scan(kept, n_clus, tiles, knum, s);
    hipLaunchKernelGGL(k_cm_emit, dim3(cm_blocks(n_clus)), dim3(CM_BLOCK), 0, s, (const u64 *)d_crow, n_clus, kept, knum, (u64 *)d_out, (u64 *)d_rows);
    if (d_reads) hipLaunchKernelGGL(k_cm_reads, dim3(cm_blocks(n_wit)), dim3(CM_BLOCK), 0, s, n_wit, oread, wsite, wclus, wklass, kept, knum, d_reads);
}
extern "C" int64_t uvc_clipmates_cluster_ints(int64_t n_clus) { return 2 * (n_clus + 1) + uvc_scan_tiles(n_clus) + 1; }
extern "C" const int32_t *uvc_clipmates_n_kept_at(const int32_t *d_clus_ints, int64_t n_clus) { return d_clus_ints + (n_clus + 1) + n_clus; }
