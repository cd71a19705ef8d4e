// uvc_clipsites.hip -- uvcgpu_region_clip_sites: the (position, side) sites inside a list of ranges at which the soft and hard clips of the
// handle's alignments pile up, one row of counters and base votes per site and one 16-byte row per event behind a site (the
// definitions are in uvcgpu.h).  Nothing here reads the planes: the inputs are the read columns of set_reads (RawReads), RegionDev::cigars
// and ::bases.  Unlike the other reports the sites are found, not given.
//
// A lane takes one alignment and walks its CIGAR alone (cs_walk): an alignment has at most two events, whatever its length, so the work is
// proportional to the alignments and their ops.
//   k_cs_find    the FIND pass: per counted alignment +1 / -1 into the difference array of spanning(p) and, per qualifying in-range event,
//                +1 into cnt[x][side]; the four totals of the pass are summed per block in LDS.
//   (uvc_launch_tile_sums over the differences, uvc_launch_block_scan over the tile sums)
//   k_cs_span    per tile of positions: the differences become spanning(p) in place; the tile's sites (cnt >= min_reads) are counted.
//   (uvc_launch_block_scan over the tiles' site counts: the number of sites)
//   k_cs_keys    the same tiles write their sites' keys 2 x + side behind the scanned base: ascending, which is (p, side) order.
//   k_cs_kept    per alignment the number of its events at kept sites, 0..2
//   (uvc_launch_tile_sums / _block_scan / _tile_prefix over them: the first event row of every alignment and the number of rows)
// The host reads the totals, the number of sites and the number of event rows; a call with room goes on:
//   k_cs_rowinit one lane per site: range, pos, side, reads and spanning of the row (the rows are zero before)
//   k_cs_fill    the FILL pass: the walk again; an event's site is looked up in the key list (first_ge), its event row is written at the
//                alignment's scanned base, and the row words and votes are added with 64-bit integer atomics whose results nobody reads.
//                A real breakpoint puts thousands of events on one row, so the lanes of a wave are grouped by site first (one ballot
//                round per distinct site among the lanes) and every counter and vote cell takes one add per group: the first lane of
//                the group's lanes with that vote adds their popcount.  len_sum, mapq_sum and len_max are reduced over the wave when all
//                of its events meet at one site, and go lane by lane otherwise.
// Integer adds only, no scratch memory; the order of sites and event rows depends on no atomic, two calls return the same bytes.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
enum {
#define UVC_CLIPSITE(name, first, words) CSROW_##name,
#include "uvc_clipsites.def"
#undef UVC_CLIPSITE
    CSROW_N
};
static_assert(CSROW_N == UVC_NCLIPSITE, "include/uvc_clipsites.def and UvcClipSiteSection of uvcgpu.h list the same sections");
#define UVC_CLIPSITE(name, first, words) static_assert((int)CSROW_##name == (int)UVC_CLIPSITE_##name, "uvc_clipsites.def order = UvcClipSiteSection order");
#include "uvc_clipsites.def"
#undef UVC_CLIPSITE
constexpr UvcSection CS_SECTIONS[UVC_NCLIPSITE] = {
#define UVC_CLIPSITE(name, first, words) { #name, first, words },
#include "uvc_clipsites.def"
#undef UVC_CLIPSITE
};
static_assert(uvc_sections_tile(CS_SECTIONS, UVC_CLIPSITE_ROW), "the sections of uvc_clipsites.def tile the row");
static_assert(CS_SECTIONS[UVC_CLIPSITE_VOTE].first == UVC_CLIPSITE_VOTE_BINS && CS_SECTIONS[UVC_CLIPSITE_VOTE].words == UVC_CLIPSITE_NCONS * UVC_CLIPSITE_NCODE
              && UVC_CLIPSITE_VOTE_BINS == UVC_CLIPSITE_NCOUNTER, "the vote block of uvcgpu.h is that of uvc_clipsites.def");
static_assert(sizeof(UvcClipRead) == 16 && UVC_CLIPSITE_NCONS == 32 && UVC_CLIPSITE_NTOTAL == 8, "an event row is four int32; the votes of an event fit two 64-bit words of 4-bit codes");

#define CS_TILE UVC_SCAN_TILE   // positions of one scan tile = threads of a block
#define CS_STEP 256             // alignments a block of the passes over the alignments takes per step
#define CS_MAX_BLOCKS 1024      // their blocks at most
#define CS_WORD(section) (CS_SECTIONS[UVC_CLIPSITE_##section].first)

// what the walk of one alignment leaves: the events of both sides (their boundary, soft and hard length; len 0: no event)
struct CsWalk { bool counted; int pos, rend, flag, mapq, jf, jl, p0, p1, soft0, soft1, hard0, hard1; };
DEV CsWalk cs_walk(const RegionDev &R, const RawReads &W, int a, int min_mapq) {
    CsWalk w;
    w.flag = (int)W.flag[a]; w.mapq = (int)W.mapq[a]; w.pos = W.pos[a]; w.rend = w.pos;
    w.counted = (w.mapq >= min_mapq && (w.flag & 0x4) == 0 && W.l_qseq[a] > 0);
    w.jf = w.jl = -1; w.p0 = w.p1 = 0; w.soft0 = w.soft1 = w.hard0 = w.hard1 = 0;
    if (!w.counted) return w;
    const int nc = W.n_cigar[a];
    const long long co = W.cigar_off[a];
    int p = w.pos, s = 0, h = 0;   // s, h: the clipped lengths since the last aligned op (in front of the first: the LEFT event)
    for (int j = 0; j < nc; j++) {
        const uint32_t cg = R.cigars[co + j];
        const int op = cig_op(cg), len = cig_len(cg);
        if (cig_aligned(op)) {
            if (w.jf < 0) { w.jf = j; w.p0 = p; w.soft0 = s; w.hard0 = h; }
            w.jl = j; p += len; w.p1 = p; s = 0; h = 0;
        } else if (op == C_SOFT_CLIP) s += len;
        else if (op == C_HARD_CLIP) h += len;
        else if (cig_ref(op)) p += len;
    }
    if (w.jf >= 0) { w.soft1 = s; w.hard1 = h; }
    w.rend = p;
    return w;
}
// the range that holds plane index x, -1 when none does (rows { x0, first compact position }, n_ranges + 1 of them)
DEV int cs_range_of(const UvcRangeRow *tab, int n_ranges, int x) {
    int lo = 0, hi = n_ranges;
    if (tab[0].x0 > x) return -1;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tab[mid].x0 <= x) lo = mid; else hi = mid; }
    return (x - tab[lo].x0 < tab[lo + 1].first - tab[lo].first) ? lo : -1;
}
// the key 2 x + side of a qualifying event whose boundary lies on the region's positions, -1 for every other event
DEV long long cs_key(const RegionDev &R, int jf, int p, int soft, int hard, int side, int min_clip) {
    const long long x = (long long)p - R.beg;
    return (jf >= 0 && soft + hard >= min_clip && x >= 0 && x < R.npos) ? 2 * x + side : -1;
}

// cnt[2 x + side]: qualifying in-range events; dx[x]: the differences of spanning; totals[0..3] (zero at the start)
__global__ void __launch_bounds__(CS_STEP) k_cs_find(RegionDev R, RawReads W, const UvcRangeRow *tab, int n_ranges, int min_mapq, int min_clip, int32_t *cnt, int32_t *dx, unsigned long long *totals) {
    __shared__ unsigned tot[4];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < 4) tot[tid] = 0;
    __syncthreads();
    const long long n_alns = R.n_alns, npos = R.npos;
    for (long long a0 = (long long)blockIdx.x * CS_STEP; a0 < n_alns; a0 += (long long)gridDim.x * CS_STEP) {
        const long long a = a0 + tid;
        bool counted = false;
        int n_in = 0, n_off = 0, n_short = 0;
        if (a < n_alns) {
            const CsWalk w = cs_walk(R, W, (int)a, min_mapq);
            counted = w.counted;
            if (counted) {
                const long long b = (long long)w.pos + 1 - R.beg, e = (long long)w.rend - R.beg, lo = (b > 0 ? b : 0), hi = (e < npos ? e : npos);   // pos < p < rend
                if (lo < hi) { atomicAdd(dx + lo, 1); if (hi < npos) atomicAdd(dx + hi, -1); }
#pragma unroll
                for (int side = 0; side < 2; side++) {
                    const int len = side ? w.soft1 + w.hard1 : w.soft0 + w.hard0;
                    if (w.jf < 0 || len < 1) continue;
                    if (len < min_clip) { n_short++; continue; }
                    const long long key = cs_key(R, w.jf, side ? w.p1 : w.p0, side ? w.soft1 : w.soft0, side ? w.hard1 : w.hard0, side, min_clip);
                    if (key >= 0 && cs_range_of(tab, n_ranges, (int)(key >> 1)) >= 0) { atomicAdd(cnt + key, 1); n_in++; }
                    else n_off++;
                }
            }
        }
        count_lanes(tot + UVC_CLIPTOTAL_alignments, counted, lane);
        const int s_in = wave_sum(n_in), s_off = wave_sum(n_off), s_short = wave_sum(n_short);
        if (lane == 0) {
            if (s_in) lds_add(tot + UVC_CLIPTOTAL_events_in_range, (unsigned)s_in);
            if (s_off) lds_add(tot + UVC_CLIPTOTAL_events_off_range, (unsigned)s_off);
            if (s_short) lds_add(tot + UVC_CLIPTOTAL_events_short, (unsigned)s_short);
        }
    }
    __syncthreads();
    if (tid < 4 && tot[tid]) atomicAdd(totals + tid, (unsigned long long)tot[tid]);
}

// dx: the differences, on return spanning; tile_pref: their scanned tile sums; blocks[t]: the sites of tile t; totals[4] += the events at them
__global__ void __launch_bounds__(CS_TILE) k_cs_span(long long npos, int32_t *dx, const int32_t *tile_pref, const int32_t *cnt, int min_reads, int32_t *blocks, unsigned long long *totals) {
    __shared__ int sh_wave[CS_TILE / 64];
    __shared__ int sh_sum[2][CS_TILE / 64];
    const long long x = (long long)blockIdx.x * CS_TILE + threadIdx.x;
    const bool have = (x < npos);
    const int d = have ? dx[x] : 0;
    const int D = tile_pref[blockIdx.x] + block_excl<CS_TILE / 64>(d, sh_wave) + d;
    int v[2] = { 0, 0 };   // sites, events at them
    if (have) {
        dx[x] = D;
        const int c0 = cnt[2 * x], c1 = cnt[2 * x + 1];
        if (c0 >= min_reads) { v[0]++; v[1] += c0; }
        if (c1 >= min_reads) { v[0]++; v[1] += c1; }
    }
    block_sums<CS_TILE / 64, 2>(v, sh_sum);
    if (threadIdx.x == 0) { blocks[blockIdx.x] = v[0]; if (v[1]) atomicAdd(totals + UVC_CLIPTOTAL_events_at_sites, (unsigned long long)v[1]); }
}
// blocks: scanned; keys[rank] = 2 x + side of every site, ascending (room: the entries keys has)
__global__ void __launch_bounds__(CS_TILE) k_cs_keys(long long npos, const int32_t *cnt, int min_reads, const int32_t *blocks, int32_t *keys, long long room) {
    __shared__ int sh_wave[CS_TILE / 64];
    const long long x = (long long)blockIdx.x * CS_TILE + threadIdx.x;
    const bool k0 = (x < npos && cnt[2 * x] >= min_reads), k1 = (x < npos && cnt[2 * x + 1] >= min_reads);
    const long long at = (long long)blocks[blockIdx.x] + block_excl<CS_TILE / 64>((int)k0 + (int)k1, sh_wave);
    if (k0 && at < room) keys[at] = (int32_t)(2 * x);
    if (k1 && at + k0 < room) keys[at + k0] = (int32_t)(2 * x + 1);
}
// kept[a]: the events of alignment a at kept sites (cnt is only ever positive for an in-range key)
__global__ void __launch_bounds__(CS_STEP) k_cs_kept(RegionDev R, RawReads W, int min_mapq, int min_clip, int min_reads, const int32_t *cnt, int32_t *kept) {
    const long long a = (long long)blockIdx.x * CS_STEP + threadIdx.x;
    if (a >= R.n_alns) return;
    const CsWalk w = cs_walk(R, W, (int)a, min_mapq);
    const long long k0 = cs_key(R, w.jf, w.p0, w.soft0, w.hard0, 0, min_clip), k1 = cs_key(R, w.jf, w.p1, w.soft1, w.hard1, 1, min_clip);
    kept[a] = (int)(w.counted && k0 >= 0 && cnt[k0] >= min_reads) + (int)(w.counted && k1 >= 0 && cnt[k1] >= min_reads);
}

// the words of a row that are known per site; the rows are zero
__global__ void __launch_bounds__(256) k_cs_rowinit(RegionDev R, const UvcRangeRow *tab, int n_ranges, const int32_t *keys, int n_sites, const int32_t *cnt, const int32_t *span, unsigned long long *rows) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n_sites) return;
    const int key = keys[i], x = key >> 1;
    unsigned long long *row = rows + (size_t)i * UVC_CLIPSITE_ROW;
    row[CS_WORD(range)] = (unsigned long long)(long long)cs_range_of(tab, n_ranges, x);
    row[CS_WORD(pos)] = (unsigned long long)((long long)x + R.beg);
    row[CS_WORD(side)] = (unsigned long long)(key & 1);
    row[CS_WORD(reads)] = (unsigned long long)cnt[key];
    row[CS_WORD(spanning)] = (unsigned long long)(long long)span[x];
}

// the vote codes of one event, 4 bits each: vote k in bits [4 k, 4 k + 4) of lo (k < 16) / of hi.  The S ops of the event are those in front
// of op jf (LEFT) or behind op jl (RIGHT); c[i] is the i-th of their query bases, vote k = c[soft - 1 - k] (LEFT) / c[k] (RIGHT)
DEV void cs_votes(const RegionDev &R, const RawReads &W, int a, int j0, int j1, int soft, bool left, unsigned long long &lo, unsigned long long &hi) {
    lo = hi = 0;
    const long long co = W.cigar_off[a], so = W.seq_off[a];
    int q = 0, i = 0;
    for (int j = 0; j < j1; j++) {
        const uint32_t cg = R.cigars[co + j];
        const int op = cig_op(cg), len = cig_len(cg);
        if (j >= j0 && op == C_SOFT_CLIP) {
            // the bases of this op that have a vote: k = soft - 1 - (i + t) < NCONS (LEFT), k = i + t < NCONS (RIGHT)
            const int t0 = left ? imax(0, soft - UVC_CLIPSITE_NCONS - i) : 0, t1 = left ? len : imin(len, UVC_CLIPSITE_NCONS - i);
            for (int t = t0; t < t1; t++) {
                const int base = (int)R.bases[so + q + t], k = left ? soft - 1 - (i + t) : i + t;
                const unsigned long long code = (unsigned long long)(base <= UVC_BASE_T ? base : UVC_CLIPSITE_NCODE - 1);
                if (k < 16) lo |= code << (4 * k); else hi |= code << (4 * (k - 16));
            }
            i += len;
        }
        if (cig_query(op)) q += len;
    }
}
// one side of the alignments of a wave; every lane of the wave makes the call.  key: this lane's event key or -1; returns whether the
// lane's event is at a kept site
DEV bool cs_fill_side(const RegionDev &R, const RawReads &W, int a, const CsWalk &w, bool left, long long key, int soft, int hard, int min_reads, const int32_t *cnt, const int32_t *keys, int n_sites,
                      unsigned long long *rows, UvcClipRead *out, int lane) {
    int site = -1;
    if (key >= 0 && cnt[key] >= min_reads) site = first_ge(keys, n_sites, (int)key);
    const bool on = (site >= 0);
    if (on && out) *(int4 *)out = make_int4(site, a, soft, hard);
    const unsigned long long act = __ballot(on);
    if (!act) return false;
    // the lanes of this lane's site
    unsigned long long grp = 0, left_m = act;
#ifdef UVC_CLIPSITES_NO_PREMERGE   // the variant the pre-merge was measured against: every lane a group of its own, one add per event and word
    grp = on ? 1ull << lane : 0ull; left_m = 0;
#endif
    while (left_m) {
        const int lead = __ffsll((long long)left_m) - 1;
        const int s = __shfl(site, lead);
        const unsigned long long same = __ballot(on && site == s);
        if (on && site == s) grp = same;
        left_m &= ~same;
    }
    unsigned long long *row = rows + (size_t)(on ? site : 0) * UVC_CLIPSITE_ROW;
    const bool leader = on && lane == __ffsll((long long)grp) - 1;
    unsigned long long m;
    m = __ballot(on && !(w.flag & 0x10)) & grp;  if (leader && m) atomicAdd(row + CS_WORD(reads_fwd), (unsigned long long)__popcll(m));
    m = __ballot(on && (w.flag & 0x800)) & grp;  if (leader && m) atomicAdd(row + CS_WORD(reads_supp), (unsigned long long)__popcll(m));
    m = __ballot(on && (w.flag & 0x100)) & grp;  if (leader && m) atomicAdd(row + CS_WORD(reads_secondary), (unsigned long long)__popcll(m));
    m = __ballot(on && hard > 0) & grp;          if (leader && m) atomicAdd(row + CS_WORD(reads_hard), (unsigned long long)__popcll(m));
    const int len = soft + hard;
    if (__ballot(on && grp != act) == 0) {   // (wave-uniform) one site in this wave: the sums over the wave, one add each
        const long long ls = wave_sum(on ? (long long)len : 0ll), ms = wave_sum(on ? (long long)w.mapq : 0ll);
        const int lm = wave_max(on ? len : 0);
        if (leader) { atomicAdd(row + CS_WORD(len_sum), (unsigned long long)ls); atomicAdd(row + CS_WORD(mapq_sum), (unsigned long long)ms); atomicMax(row + CS_WORD(len_max), (unsigned long long)lm); }
    } else if (on) {
        atomicAdd(row + CS_WORD(len_sum), (unsigned long long)len); atomicAdd(row + CS_WORD(mapq_sum), (unsigned long long)w.mapq); atomicMax(row + CS_WORD(len_max), (unsigned long long)len);
    }
    // the votes: per k and code one add per group, by the first of the group's lanes that hold it
    unsigned long long vlo = 0, vhi = 0;
    const int nv = on ? imin(soft, UVC_CLIPSITE_NCONS) : 0;
    if (nv > 0) cs_votes(R, W, a, left ? 0 : w.jl + 1, left ? w.jf : W.n_cigar[a], soft, left, vlo, vhi);
    const int kmax = wave_max(nv);
    for (int k = 0; k < kmax; k++) {
        const int code = (int)((k < 16 ? vlo >> (4 * k) : vhi >> (4 * (k - 16))) & 15);
        const bool hv = (k < nv);
#pragma unroll
        for (int c = 0; c < UVC_CLIPSITE_NCODE; c++) {
            m = __ballot(hv && code == c) & grp;
            if (hv && code == c && lane == __ffsll((long long)m) - 1) atomicAdd(row + CS_WORD(VOTE) + k * UVC_CLIPSITE_NCODE + c, (unsigned long long)__popcll(m));
        }
    }
    return on;
}
// epre[a]: the first event row of alignment a; reads: NULL without want_reads
__global__ void __launch_bounds__(CS_STEP) k_cs_fill(RegionDev R, RawReads W, int min_mapq, int min_clip, int min_reads, const int32_t *cnt, const int32_t *keys, int n_sites, const int32_t *epre,
                                                     unsigned long long *rows, UvcClipRead *reads) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const long long n_alns = R.n_alns;
    for (long long a0 = (long long)blockIdx.x * CS_STEP; a0 < n_alns; a0 += (long long)gridDim.x * CS_STEP) {   // (block-uniform: whole waves make the calls below)
        const long long a = a0 + tid;
        CsWalk w;
        w.counted = false; w.flag = w.mapq = w.pos = w.rend = 0; w.jf = w.jl = -1; w.p0 = w.p1 = w.soft0 = w.soft1 = w.hard0 = w.hard1 = 0;
        if (a < n_alns) w = cs_walk(R, W, (int)a, min_mapq);
        const long long k0 = w.counted ? cs_key(R, w.jf, w.p0, w.soft0, w.hard0, 0, min_clip) : -1, k1 = w.counted ? cs_key(R, w.jf, w.p1, w.soft1, w.hard1, 1, min_clip) : -1;
        UvcClipRead *out = (reads && a < n_alns) ? reads + epre[a] : nullptr;
        const bool on0 = cs_fill_side(R, W, (int)a, w, true, k0, w.soft0, w.hard0, min_reads, cnt, keys, n_sites, rows, out, lane);
        cs_fill_side(R, W, (int)a, w, false, k1, w.soft1, w.hard1, min_reads, cnt, keys, n_sites, rows, out ? out + (on0 ? 1 : 0) : nullptr, lane);
    }
}

unsigned cs_aln_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(CS_MAX_BLOCKS, (n + CS_STEP - 1) / CS_STEP)); }
}   // namespace

extern "C" const char *uvc_clipsites_name(int id) { return (id >= 0 && id < UVC_NCLIPSITE) ? CS_SECTIONS[id].name : nullptr; }
// ints per position of the call: cnt[npos][2] and the differences / spanning[npos]
extern "C" int64_t uvc_clipsites_pos_ints(int64_t npos) { return 3 * npos; }
// ints of scan scratch: [tile sums of the differences, their total] [sites per tile, their number] [first event row per alignment, the
// number of rows] [tile sums of the kept counts, their total]
extern "C" int64_t uvc_clipsites_scratch_ints(int64_t n_alns, int64_t npos) { return 2 * (uvc_scan_tiles(npos) + 1) + (n_alns + 1) + (uvc_scan_tiles(n_alns) + 1); }
// where the host reads the number of sites and the number of event rows
extern "C" int64_t uvc_clipsites_sites_at(int64_t n_alns, int64_t npos) { return 2 * uvc_scan_tiles(npos) + 1; }
extern "C" int64_t uvc_clipsites_reads_at(int64_t n_alns, int64_t npos) { return 2 * (uvc_scan_tiles(npos) + 1) + n_alns; }

// The find stage.  d_totals (UVC_CLIPSITE_NTOTAL words) and d_pos (uvc_clipsites_pos_ints) are zero at the start.  R->n_alns >= 1.
extern "C" void uvc_launch_clipsites_find(const RegionDev *R, const RawReads *W, const UvcRangeRow *d_tab, int n_ranges, const UvcClipSitesRequest *req, long long *d_totals, int32_t *d_pos,
                                          int32_t *d_keys, int64_t key_room, int32_t *d_scratch, hipStream_t s) {
    const int n = R->n_alns;
    const long long npos = R->npos;
    if (n <= 0 || npos <= 0) return;
    const int ntp = (int)uvc_scan_tiles(npos), nta = (int)uvc_scan_tiles(n);
    int32_t *cnt = d_pos, *dx = d_pos + 2 * npos;
    int32_t *tsum = d_scratch, *blocks = tsum + ntp + 1, *epre = blocks + ntp + 1, *asum = epre + n + 1;
    unsigned long long *totals = (unsigned long long *)d_totals;
    hipLaunchKernelGGL(k_cs_find, dim3(cs_aln_blocks(n)), dim3(CS_STEP), 0, s, *R, *W, d_tab, n_ranges, req->min_mapq, req->min_clip, cnt, dx, totals);
    uvc_launch_tile_sums(dx, npos, 0, tsum, s);
    uvc_launch_block_scan(tsum, ntp, s);
    hipLaunchKernelGGL(k_cs_span, dim3((unsigned)ntp), dim3(CS_TILE), 0, s, npos, dx, tsum, cnt, req->min_reads, blocks, totals);
    uvc_launch_block_scan(blocks, ntp, s);
    hipLaunchKernelGGL(k_cs_keys, dim3((unsigned)ntp), dim3(CS_TILE), 0, s, npos, cnt, req->min_reads, blocks, d_keys, (long long)key_room);
    hipLaunchKernelGGL(k_cs_kept, dim3((unsigned)nta), dim3(CS_STEP), 0, s, *R, *W, req->min_mapq, req->min_clip, req->min_reads, cnt, epre);
    uvc_launch_tile_sums(epre, n, 0, asum, s);
    uvc_launch_block_scan(asum, nta, s);
    uvc_launch_tile_prefix(epre, n, 0, asum, epre, s);
}
// The fill stage, after a find with the same arguments.  d_rows: n_sites rows, zero at the start; d_reads: room for the event rows the find
// counted, or NULL
extern "C" void uvc_launch_clipsites_fill(const RegionDev *R, const RawReads *W, const UvcRangeRow *d_tab, int n_ranges, const UvcClipSitesRequest *req, const int32_t *d_pos, const int32_t *d_keys,
                                          int n_sites, const int32_t *d_scratch, long long *d_rows, UvcClipRead *d_reads, hipStream_t s) {
    const int n = R->n_alns;
    const long long npos = R->npos;
    if (n <= 0 || n_sites <= 0) return;
    const int ntp = (int)uvc_scan_tiles(npos);
    const int32_t *cnt = d_pos, *span = d_pos + 2 * npos, *epre = d_scratch + 2 * (ntp + 1);
    hipLaunchKernelGGL(k_cs_rowinit, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, s, *R, d_tab, n_ranges, d_keys, n_sites, cnt, span, (unsigned long long *)d_rows);
    hipLaunchKernelGGL(k_cs_fill, dim3(cs_aln_blocks(n)), dim3(CS_STEP), 0, s, *R, *W, req->min_mapq, req->min_clip, req->min_reads, cnt, d_keys, n_sites, epre, (unsigned long long *)d_rows, d_reads);
}
