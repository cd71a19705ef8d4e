// uvc_readprofile.hip -- uvcgpu_region_read_profile: base-quality, cycle and substitution profile of the reads of the handle over a list of
// ranges (the definitions are in uvcgpu.h).  Nothing here reads the planes: the inputs are the read columns of set_reads
// (RawReads), RegionDev::bases / bq / cigars and the reference symbols.
//
// The work is proportional to read bases and is split by read base, never by read: a CHUNK is 64 consecutive query indices of one
// alignment, a wave takes a run of consecutive chunks (uvc_launch_tile_prefix: the exclusive prefix of ceil(l_qseq / 64) over the alignments, a
// three-launch tile scan), finds the alignment of its first chunk by one binary search and moves on from there.  A 150-base read is three
// chunks, a 15 kb read 235; both load the machine alike.  Everything about the alignment is wave-uniform (scalar loads).
//
// The op of a base.  A lane holds query index q0 + lane.  The wave walks the CIGAR together, 64 ops per step: lane j loads op j, a wave
// scan of the query and reference lengths gives every op its first query index and reference coordinate, a ballot finds the ops that
// overlap the chunk, and their fields are broadcast one by one to the lanes they hold.  The walk stops behind the chunk.  So no lane walks
// a CIGAR alone; a chunk of a read with n ops costs n / 64 wave steps in front of it -- a simple alignment ([clip] M [clip]) one.
// An op's own lane owns what happens once per op: the +1 / -1 of an M run (pass one) and the event of a D op (pass two), in the chunk
// that holds the op's first query index (D: the query index in front of it).
//
// Pass one (k_rp_reads<false>), depth and mismatches of the counted alignments.  D is a coverage count but for the rare N bases: every M
// run adds +1 at its first position and -1 behind its last (two atomics per run, not one per base), an N base -1 at its position and +1
// behind it; the scan of pass two turns the differences into D.  X takes one atomic per mismatching base, about 1e-3 of the bases.  (An
// amplicon pile puts the run ends of every read on the same two words: see DESIGN.md 4m.)
// k_rp_status scans the differences (tile sums, one block over the tile sums, a block scan per tile), folds D, X and the reference symbol
// into one status byte per position -- bits 0..1 the status, bit 2 "inside a range" -- and counts positions_*.
// Pass two (k_rp_reads<true>) reads that byte, the packed base | quality and bins into a block-private copy of the row in LDS.
//   RP_CELLS 32-bit words = 22 848 B.  A word grows by at most 1 per read base the block sees, and a handle holds fewer than 2^31 read
//   bases in all (RegionDev::bq_bytes = 2 * bases is 32 bits wide): no word wraps.
//   CYC: consecutive lanes hold consecutive cycles, their adds fall on different words -- except behind the cap (cycle >= 255), where a
//   whole chunk of a long read meets on one word per kind: such a chunk counts each kind by a ballot and one lane adds.
//   Q, SUB and the counters: a wave of one read meets on a handful of words (an instrument reports 4-8 distinct qualities), so equal
//   keys are merged in the wave first -- one ballot per distinct key, the first lane of each adds the popcount.
// At the end a block adds its non-zero words to one of `shards` copies of the row with 64-bit vector atomics; uvc_launch_sum_fold sums the copies.
// Integer adds only: their order does not show, two calls return the same bits.
#include "uvc_report_dev.h"

#include <algorithm>

namespace {
enum {
#define UVC_READPROF(name, first, words) RPROW_##name,
#include "uvc_readprofile.def"
#undef UVC_READPROF
    RPROW_N
};
static_assert(RPROW_N == UVC_NREADPROF, "include/uvc_readprofile.def and UvcReadProfSection of uvcgpu.h list the same sections");
#define UVC_READPROF(name, first, words) static_assert((int)RPROW_##name == (int)UVC_READPROF_##name, "uvc_readprofile.def order = UvcReadProfSection order");
#include "uvc_readprofile.def"
#undef UVC_READPROF
constexpr UvcSection RP_SECTIONS[UVC_NREADPROF] = {
#define UVC_READPROF(name, first, words) { #name, first, words },
#include "uvc_readprofile.def"
#undef UVC_READPROF
};
static_assert(uvc_sections_tile(RP_SECTIONS, UVC_READPROF_ROW), "the sections of uvc_readprofile.def tile the row");
static_assert(RP_SECTIONS[UVC_READPROF_Q].first == UVC_READPROF_Q_BINS && RP_SECTIONS[UVC_READPROF_Q].words == UVC_READPROF_NCLASS * UVC_READPROF_NQUAL * 2
              && RP_SECTIONS[UVC_READPROF_CYC].first == UVC_READPROF_CYC_BINS && RP_SECTIONS[UVC_READPROF_CYC].words == UVC_READPROF_NCLASS * UVC_READPROF_NCYCLE * UVC_READPROF_NKIND
              && RP_SECTIONS[UVC_READPROF_SUB].first == UVC_READPROF_SUB_BINS && RP_SECTIONS[UVC_READPROF_SUB].words == UVC_READPROF_NCLASS * 16
              && RP_SECTIONS[UVC_READPROF_bases_low_mapq].first == UVC_READPROF_COUNTERS && UVC_READPROF_COUNTERS + UVC_READPROF_NCOUNTER == UVC_READPROF_ROW,
              "the block offsets of uvcgpu.h are those of uvc_readprofile.def");

#define RP_CELLS UVC_READPROF_ROW
#define RP_MAX_SHARDS 16
#define RP_TILE UVC_SCAN_TILE   // k_rp_status takes a tile of the depth scan: threads of a block
#define RP_MIN_CHUNKS 8         // chunks a wave takes at least (one binary search per wave)
#define RP_MAX_BLOCKS 1024      // four per CU: a block keeps its copy of the row over all of its chunks
enum { RP_NO_REF = 0, RP_LOW_DEPTH = 1, RP_HIGH_ALT = 2, RP_CLEAN = 3, RP_IN_RANGE = 4 };   // the status byte
enum { RP_K_MATCH = 0, RP_K_MISMATCH, RP_K_INS, RP_K_DEL, RP_K_CLIP };
static_assert(UVC_READPROF_positions_low_depth == UVC_READPROF_positions_no_ref + RP_LOW_DEPTH && UVC_READPROF_positions_high_alt == UVC_READPROF_positions_no_ref + RP_HIGH_ALT
              && UVC_READPROF_positions_clean == UVC_READPROF_positions_no_ref + RP_CLEAN, "the positions_* counters come in status order");
#define RP_WORD(section) (RP_SECTIONS[UVC_READPROF_##section].first)

const char *const RP_CLASS_NAMES[UVC_READPROF_NCLASS] = { "R1_fwd", "R1_rev", "R2_fwd", "R2_rev" };

// is plane index x inside a range of the table (rows { x0, first compact position }, n_ranges + 1 of them)
DEV bool rp_in_ranges(const UvcRangeRow *tab, int n_ranges, int x) {
    int lo = 0, hi = n_ranges;   // the last range that begins at or in front of x (last_le over a member of the rows: kept here, k_rp_status' text is the parent's)
    if (tab[0].x0 > x) return false;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tab[mid].x0 <= x) lo = mid; else hi = mid; }
    return x - tab[lo].x0 < tab[lo + 1].first - tab[lo].first;
}
// dx: the differences of pass one, on return D; status: the byte per position; part: the copy of the row this block's counts go to
__global__ void __launch_bounds__(RP_TILE) k_rp_status(RegionDev R, int32_t *dx, const int32_t *X, const int32_t *tile_pref, const UvcRangeRow *tab, int n_ranges, int min_depth, int permille,
                                                       uint8_t *status, int shards, unsigned long long *parts) {
    __shared__ int sh_wave[RP_TILE / 64];
    __shared__ unsigned cnt[4];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < 4) cnt[tid] = 0;
    const long long x = (long long)blockIdx.x * RP_TILE + tid;
    const bool have = (x < R.npos);
    const int d = have ? dx[x] : 0;
    const int D = tile_pref[blockIdx.x] + block_excl<RP_TILE / 64>(d, sh_wave) + d;   // (the sync inside also orders cnt's zeroing)
    int st = -1; bool in = false;
    if (have) {
        dx[x] = D;
        const int ref = (int)R.refsym[x];
        if (ref > UVC_BASE_T || x == R.npos - 1) st = RP_NO_REF;   // (the region's last position holds no reference base)
        else if (D < min_depth) st = RP_LOW_DEPTH;
        else if ((long long)X[x] * 1000 > (long long)permille * D) st = RP_HIGH_ALT;
        else st = RP_CLEAN;
        in = rp_in_ranges(tab, n_ranges, (int)x);
        status[x] = (uint8_t)(st | (in ? RP_IN_RANGE : 0));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) count_lanes(cnt + k, in && st == k, lane);
    __syncthreads();
    if (tid < 4 && cnt[tid]) atomicAdd(parts + (size_t)(blockIdx.x % (unsigned)shards) * RP_CELLS + RP_WORD(positions_no_ref) + tid, (unsigned long long)cnt[tid]);
}

// BIN = false: pass one (dx, X); BIN = true: pass two (status -> parts)
template <bool BIN> __global__ void __launch_bounds__(256) k_rp_reads(RegionDev R, RawReads W, const int32_t *cpre, int min_mapq, int32_t *dx, int32_t *X, const uint8_t *status,
                                                                       int shards, unsigned long long *parts) {
    __shared__ unsigned prof[BIN ? RP_CELLS : 1];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (BIN) { for (int j = tid; j < RP_CELLS; j += 256) prof[j] = 0; __syncthreads(); }
    const int n_alns = R.n_alns;
    const long long npos = R.npos;
    const int total = cpre[n_alns];
    const int n_waves = (int)gridDim.x * 4;
    const int per = (total + n_waves - 1) / n_waves;
    const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (tid >> 6));
    const long long c0 = (long long)wv * per, c1 = (c0 + per < total ? c0 + per : total);
    if (c0 < c1) {
        int a = last_le(cpre, 0, n_alns, c0);   // the last alignment with cpre <= c0: it holds chunk c0
        for (long long c = c0; c < c1; c++) {
            while (c >= cpre[a + 1]) a++;   // (c < total = cpre[n_alns]: a + 1 <= n_alns)
            const int mapq = (int)W.mapq[a];
            const bool counted = (mapq >= min_mapq);
            if (!BIN && !counted) continue;
            const int pos = W.pos[a], flag = (int)W.flag[a], L = W.l_qseq[a], nc = W.n_cigar[a];
            const long long so = W.seq_off[a], co = W.cigar_off[a];
            const int q0 = (int)(c - cpre[a]) * 64, q = q0 + lane;
            const bool have = (q < L);
            const bool rev = (flag & 0x10) != 0;
            const int cls = 2 * ((flag & 0x80) != 0) + (rev ? 1 : 0);
            int my_op = -1, my_p = 0;   // the op that holds q; the position of an aligned base, the anchor of an inserted or clipped one
            int qcur = 0, pcur = pos;   // (wave-uniform) where the next 64 ops begin
            for (int b0 = 0; b0 < nc && qcur <= q0 + 64; b0 += 64) {
                const int j = b0 + lane;
                const uint32_t cg = (j < nc ? R.cigars[co + j] : (uint32_t)C_PAD);
                const int op = cig_op(cg), len = cig_len(cg);
                const int ql = cig_query(op) ? len : 0, rl = cig_ref(op) ? len : 0;
                const int qi = wave_incl(ql), ri = wave_incl(rl);
                const int qs = qcur + qi - ql, ps = pcur + ri - rl;   // the op's first query index and reference coordinate
                if (!BIN) {
                    if (cig_aligned(op) && len > 0 && qs >= q0 && qs < q0 + 64) {   // the run's ends, clipped to the region
                        const long long lo = (long long)ps - R.beg > 0 ? (long long)ps - R.beg : 0, hi = (long long)ps + len - R.beg < npos ? (long long)ps + len - R.beg : npos;
                        if (lo < hi) { atomicAdd(dx + lo, 1); if (hi < npos) atomicAdd(dx + hi, -1); }
                    }
                } else if (op == C_DEL && counted && j < nc) {
                    const int qe = (qs > 0 ? qs - 1 : 0);
                    const long long x = (long long)ps - R.beg;
                    if (qe >= q0 && qe < q0 + 64 && qe < L && x >= 0 && x < npos && (status[x] & RP_IN_RANGE)) {
                        const int cyc = rev ? L - 1 - qe : qe;
                        lds_add(prof + RP_WORD(CYC) + (cls * UVC_READPROF_NCYCLE + imin(cyc, UVC_READPROF_NCYCLE - 1)) * UVC_READPROF_NKIND + RP_K_DEL, 1u);
                    }
                }
                unsigned long long m = __ballot(ql > 0 && qs < q0 + 64 && qs + ql > q0);
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int o = __shfl(op, l), s = __shfl(qs, l), n = __shfl(ql, l), pp = __shfl(ps, l);
                    if (have && q >= s && q - s < n) { my_op = o; my_p = cig_aligned(o) ? pp + (q - s) : imax(pos, pp - 1); }
                }
                qcur += __shfl(qi, 63); pcur += __shfl(ri, 63);
            }
            const bool act = have && my_op >= 0;
            const long long x = (long long)my_p - R.beg;
            const bool inb = act && x >= 0 && x < npos;
            if (!BIN) {
                if (inb && cig_aligned(my_op)) {
                    const int base = (int)R.bases[so + q];
                    if (base > UVC_BASE_T) { atomicAdd(dx + x, -1); if (x + 1 < npos) atomicAdd(dx + x + 1, 1); }
                    else { const int ref = (int)R.refsym[x]; if (ref <= UVC_BASE_T && ref != base) atomicAdd(X + x, 1); }
                }
                continue;
            }
            const int sb = inb ? (int)status[x] : 0;
            const bool inr = (sb & RP_IN_RANGE) != 0;
            const int st = sb & 3;
            const bool aligned = inr && cig_aligned(my_op);
            if (!counted) { count_lanes(prof + RP_WORD(bases_low_mapq), aligned, lane); continue; }   // (wave-uniform)
            const int v = inr ? (int)R.bq[so + q] : 0, base = v & 0xFF, qb = imin(v >> 8, UVC_READPROF_NQUAL - 1);
            const bool no_ref = aligned && st == RP_NO_REF, isn = aligned && !no_ref && base > UVC_BASE_T;
            const bool clean = aligned && !isn && st == RP_CLEAN;
            count_lanes(prof + RP_WORD(bases_no_ref), no_ref, lane);
            count_lanes(prof + RP_WORD(bases_n), isn, lane);
            count_lanes(prof + RP_WORD(bases_low_depth), aligned && !isn && st == RP_LOW_DEPTH, lane);
            count_lanes(prof + RP_WORD(bases_high_alt), aligned && !isn && st == RP_HIGH_ALT, lane);
            count_lanes(prof + RP_WORD(bases_clean), clean, lane);
            const int ref = clean ? (int)R.refsym[x] : 0;   // (a clean position has an A/C/G/T reference symbol)
            const int mis = (clean && base != ref) ? 1 : 0;
            merge_add(prof + RP_WORD(Q) + cls * UVC_READPROF_NQUAL * 2, qb * 2 + mis, clean, lane);
            merge_add(prof + RP_WORD(SUB) + cls * 16, ref * 4 + (base & 3), clean, lane);
            const int kind = clean ? mis : (inr && my_op == C_INS) ? RP_K_INS : (inr && my_op == C_SOFT_CLIP) ? RP_K_CLIP : -1;
            const int cyc = rev ? L - 1 - q : q;
            unsigned *row = prof + RP_WORD(CYC) + cls * UVC_READPROF_NCYCLE * UVC_READPROF_NKIND;
            const int last = (q0 + 63 < L - 1 ? q0 + 63 : L - 1);   // the chunk's last query index
            if ((rev ? L - 1 - last : q0) >= UVC_READPROF_NCYCLE - 1) {   // (wave-uniform) the whole chunk lies in the last cycle bin
                unsigned *cell = row + (UVC_READPROF_NCYCLE - 1) * UVC_READPROF_NKIND;
                count_lanes(cell + RP_K_MATCH, kind == RP_K_MATCH, lane);
                count_lanes(cell + RP_K_MISMATCH, kind == RP_K_MISMATCH, lane);
                count_lanes(cell + RP_K_INS, kind == RP_K_INS, lane);
                count_lanes(cell + RP_K_CLIP, kind == RP_K_CLIP, lane);
            } else if (kind >= 0) lds_add(row + imin(cyc, UVC_READPROF_NCYCLE - 1) * UVC_READPROF_NKIND + kind, 1u);
        }
    }
    if (BIN) {
        __syncthreads();
        unsigned long long *dst = parts + (size_t)(blockIdx.x % (unsigned)shards) * RP_CELLS;
        for (int j = tid; j < RP_CELLS; j += 256) { const unsigned v = prof[j]; if (v) atomicAdd(dst + j, (unsigned long long)v); }
    }
}

}   // namespace

extern "C" const char *uvc_readprofile_class_name(int c) { return (c >= 0 && c < UVC_READPROF_NCLASS) ? RP_CLASS_NAMES[c] : nullptr; }
// copies of the row a call adds into (the result itself is one more)
extern "C" int64_t uvc_readprofile_copies(void) { return RP_MAX_SHARDS; }
// ints of scratch: the first chunk of every alignment and their number, then the tile sums of the larger of the two scans and their total
extern "C" int64_t uvc_readprofile_scratch_ints(int64_t n_alns, int64_t npos) { return (n_alns + 1) + uvc_scan_tiles(std::max<int64_t>(n_alns, npos)) + 1; }

// The three stages of a call, each one entry of uvcgpu_region_kernel_times.  d_dx / d_x: npos ints each; d_status: npos bytes; d_parts:
// uvc_readprofile_copies() rows, zero like d_dx / d_x when stage one starts (the caller fills them); d_scratch: uvc_readprofile_scratch_ints.
// A handle without reads skips stages one and three: its status bytes come from zero depths.
extern "C" void uvc_launch_readprofile_depth(const RegionDev *R, const RawReads *W, int64_t n_bases, int min_mapq, int32_t *d_dx, int32_t *d_x, int32_t *d_scratch, hipStream_t s) {
    const int n = R->n_alns;
    if (n <= 0) return;
    int32_t *cpre = d_scratch, *tsum = d_scratch + n + 1;
    // cpre[a] = the first chunk of alignment a, cpre[n] = the number of chunks: the tile scan of ceil(l_qseq / 64)
    uvc_launch_tile_sums(W->l_qseq, n, 1, tsum, s);
    uvc_launch_block_scan(tsum, (int)uvc_scan_tiles(n), s);
    uvc_launch_tile_prefix(W->l_qseq, n, 1, tsum, cpre, s);
    const long long most = n_bases / 64 + n;   // no more chunks than this
    const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>(RP_MAX_BLOCKS, (most + 4 * RP_MIN_CHUNKS - 1) / (4 * RP_MIN_CHUNKS)));
    hipLaunchKernelGGL(k_rp_reads<false>, dim3(nb), dim3(256), 0, s, *R, *W, cpre, min_mapq, d_dx, d_x, (const uint8_t *)nullptr, 1, (unsigned long long *)nullptr);
}
extern "C" void uvc_launch_readprofile_status(const RegionDev *R, const UvcRangeRow *d_tab, int n_ranges, int min_depth, int max_alt_permille, int32_t *d_dx, const int32_t *d_x, uint8_t *d_status,
                                              long long *d_parts, int32_t *d_scratch, hipStream_t s) {
    if (R->npos <= 0 || n_ranges <= 0) return;
    int32_t *tsum = d_scratch + (R->n_alns > 0 ? R->n_alns : 0) + 1;
    const unsigned nt = (unsigned)uvc_scan_tiles(R->npos);
    uvc_launch_tile_sums(d_dx, R->npos, 0, tsum, s);
    uvc_launch_block_scan(tsum, (int)nt, s);
    hipLaunchKernelGGL(k_rp_status, dim3(nt), dim3(RP_TILE), 0, s, *R, d_dx, d_x, tsum, d_tab, n_ranges, min_depth, max_alt_permille, d_status, RP_MAX_SHARDS, (unsigned long long *)d_parts);
}
extern "C" void uvc_launch_readprofile_bin(const RegionDev *R, const RawReads *W, int64_t n_bases, int min_mapq, const uint8_t *d_status, long long *d_parts, long long *d_out, const int32_t *d_scratch, hipStream_t s) {
    const int n = R->n_alns;
    if (n > 0) {
        const long long most = n_bases / 64 + n;
        const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>(RP_MAX_BLOCKS, (most + 4 * RP_MIN_CHUNKS - 1) / (4 * RP_MIN_CHUNKS)));
        hipLaunchKernelGGL(k_rp_reads<true>, dim3(nb), dim3(256), 0, s, *R, *W, d_scratch, min_mapq, (int32_t *)nullptr, (int32_t *)nullptr, d_status, RP_MAX_SHARDS, (unsigned long long *)d_parts);
    }
    uvc_launch_sum_fold(d_parts, RP_MAX_SHARDS, RP_CELLS, d_out, s);
}
