// uvc_report_dev.h -- what the kernels of the eleven report calls share on the device: the wave-merged LDS counters, the
// three searches, the segmented fold, a block's LDS window of per-range rows, the rank of a head among the block's heads and the section
// table of a row.  Device code only, force-inlined, with each function's wave or
// block contract beside it; blocks are one-dimensional, 256 threads where a function says "block".  The kernels that several reports
// launch (array scan, tile scan, sum-fold) are in uvc_report_common.hip; UvcRangeCursor / uvc_range_find are in uvc_launch.h.
#ifndef UVC_REPORT_DEV_H
#define UVC_REPORT_DEV_H

#include "uvc_launch.h"
#include "uvc_collectives.h"
#include <limits.h>

// ---- the sections of a row: { name, first word, words } from a .def file, and the check that they follow each other and fill the row
struct UvcSection { const char *name; int first, words; };
template <int N> constexpr bool uvc_sections_tile(const UvcSection (&t)[N], int row_words) {
    int at = 0;
    for (int k = 0; k < N; k++) { if (t[k].first != at) return false; at += t[k].words; }
    return at == row_words;
}

// ---- counters in LDS, T = unsigned or unsigned long long.  The adds are relaxed and workgroup-wide: nobody reads a word before a barrier.
template <class T> UVC_COLL void lds_add(T *p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// a word every lane of the wave would add 1 to: the lanes with `on` are counted by a ballot, the wave's first lane adds the count.  Called
// by the whole wave, p wave-uniform.
template <class T> UVC_COLL void count_lanes(T *p, bool on, int lane) {
    const unsigned long long m = __ballot(on);
    if (lane == 0 && m) lds_add(p, (T)__popcll(m));
}
// tab[key] += 1 for every lane with `on`, equal keys merged first: one round per distinct key among the lanes, its first lane adds the
// popcount.  Called by the whole wave, tab wave-uniform.
template <class T> UVC_COLL void merge_add(T *tab, int key, bool on, int lane) {
    unsigned long long left = __ballot(on);
    while (left) {
        const int lead = __ffsll((long long)left) - 1;
        const int k = __shfl(key, lead);
        const unsigned long long same = __ballot(on && key == k);
        if (lane == lead) lds_add(tab + k, (T)__popcll(same));
        left &= ~same;
    }
}

// ---- binary searches in ascending lists; any lane alone
// the first index in [0, n) whose entry is >= x, n when there is none
UVC_COLL int first_ge(const int32_t *list, int n, int x) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (list[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// the last index in [lo, hi) whose entry is <= x (lo < hi; lo itself where every entry is larger)
template <class X> UVC_COLL int last_le(const int32_t *list, int lo, int hi, X x) {
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (list[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// the first of the caller's ranges (ascending, disjoint) that ends behind lo, where it begins in front of hi: the first range [lo, hi)
// overlaps; n_ranges where it overlaps none
UVC_COLL int first_range(const UvcFamilyRange *ranges, int n_ranges, int lo, int hi) {
    int a = 0, b = n_ranges;
    while (a < b) { const int mid = (a + b) >> 1; if (ranges[mid].pos_end > lo) b = mid; else a = mid + 1; }
    return (a < n_ranges && ranges[a].pos_beg < hi) ? a : n_ranges;
}

// ---- the segmented fold.  The lanes of a wave hold runs of equal keys (the elements of one object are consecutive) and each run folds on
// its own: not a scan or reduction of uvc_collectives.h's kind.  Every lane of the wave makes the call.
// NP (min, max) pairs per lane.  Lane l ends up with the part of its run that lies in lanes [l, 64): after the step with `off` it holds
// lanes [l, l + 2 off) of the run.  The head lane of a run then holds the whole of the run's part in this wave.
template <int NP> UVC_COLL void seg_fold_minmax(int key, int (&lo)[NP], int (&hi)[NP]) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int key2 = __shfl_down(key, off);
        const bool same = (lane + off < 64 && key2 == key);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int lo2 = __shfl_down(lo[p], off), hi2 = __shfl_down(hi[p], off);
            if (same) { lo[p] = lo2 < lo[p] ? lo2 : lo[p]; hi[p] = hi2 > hi[p] ? hi2 : hi[p]; }
        }
    }
}
// is this lane the head of its run: lane 0, or a lane whose left neighbour has another key
UVC_COLL bool seg_head(int key) {
    const int prev = __shfl_up(key, 1);   // (the previous lane's key: a neighbour fetch)
    return (threadIdx.x & 63) == 0 || prev != key;
}

// ---- a block's window of per-range rows in LDS: the rows (ROW words of T) of WIN consecutive ranges beginning at win0, the smallest first
// range of the block's objects, so that most adds of a block stay in LDS; an add outside the window goes to the global row as one 64-bit
// atomic.  In a __shared__ object of a 256-thread block, in this order, every thread making each call but add:
//     begin(tid)  --  the caller's __syncthreads()  --  w0 = choose(first_min)  --  add(w0, ..) by any lane  --  the caller's __syncthreads()  --  flush(tid, w0, ..)
template <class T, int WIN, int ROW> struct UvcRowWindow {
    T part[WIN * ROW];
    int win0;
    UVC_COLL void begin(int tid) {
        for (int j = tid; j < WIN * ROW; j += 256) part[j] = 0;
        if (tid == 0) win0 = INT_MAX;
    }
    // first_min: the smallest first range of this thread's objects, INT_MAX where none meets a range.  ONE barrier.  Returns the window's
    // first range; INT_MAX (block-uniform): no object of the block meets a range, nothing to add or flush
    UVC_COLL int choose(int first_min) {
        if (first_min != INT_MAX) __hip_atomic_fetch_min(&win0, first_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        return win0;
    }
    UVC_COLL void add(int w0, unsigned long long *rows, int i, int word, T v) {
        if ((unsigned)(i - w0) < (unsigned)WIN) lds_add(part + (i - w0) * ROW + word, v);
        else atomicAdd(rows + (size_t)i * ROW + word, (unsigned long long)v);
    }
    // the non-zero words of the window into the global rows (the window may reach past the last range: those rows are zero)
    UVC_COLL void flush(int tid, int w0, int n_ranges, unsigned long long *rows) const {
        for (int j = tid; j < WIN * ROW; j += 256) {
            const T v = part[j];
            const int i = w0 + j / ROW;
            if (v && i < n_ranges) atomicAdd(rows + (size_t)i * ROW + (j % ROW), (unsigned long long)v);
        }
    }
};

// ---- the rank of a head among the heads of a block of four waves, in thread order: the heads up to and including this thread (a head's
// own rank from 1; for any thread the number of the run it lies in), total: the block's heads, in every thread.  sh[4].  ONE barrier
// inside; sh is read behind it, so the caller has a __syncthreads() between this call and the next on the same sh.
UVC_COLL int head_rank(bool head, int *sh, int &total) {
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const unsigned long long heads = __ballot(head);
    if (lane == 0) sh[wv] = __popcll(heads);
    __syncthreads();
    int incl = __popcll(heads & ((2ull << lane) - 1ull));
    for (int w = 0; w < wv; w++) incl += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    return incl;
}
#endif
