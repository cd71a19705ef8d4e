// uvc_collectives.h -- the cross-lane and cross-wave sums of the kernels: each loop over shuffle distances, each "lane 63 writes the wave's
// total" and each difference-array step once, with its barrier contract beside it.  Device code only, force-inlined; the .hip files that
// need it include it.  Blocks are one-dimensional and a whole number of 64-lane waves; every thread of the wave (wave_*) or of the block
// (block_*, waves_*) makes the call.  Sum, min and max only.  What is NOT here: neighbour fetches (__shfl_up(v, 1)), segmented folds,
// suffix scans and the spin protocol of the chained scan stay where they are used.
#ifndef UVC_COLLECTIVES_H
#define UVC_COLLECTIVES_H

#include <hip/hip_runtime.h>
#define UVC_COLL __device__ __forceinline__

// ---- over the lanes of a wave: xor butterfly, every lane gets the result.  W < 64: over each aligned group of W lanes (k_aln_bm's eight)
template <int W = 64, class T> UVC_COLL T wave_sum(T v) {
#pragma unroll
    for (int d = W / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
template <class T> UVC_COLL T wave_min(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const T o = __shfl_xor(v, d); v = (o < v ? o : v); }
    return v;
}
template <class T> UVC_COLL T wave_max(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const T o = __shfl_xor(v, d); v = (o > v ? o : v); }
    return v;
}
// inclusive scan over the 64 lanes: lane l gets v of lanes 0 .. l
template <class T> UVC_COLL T wave_incl(T v) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(v, o); if (lane >= o) v += t; }
    return v;
}

// ---- one value per WAVE, summed over the block's NW waves through sh[NW] ----
// the sum of sh[0 .. NW): no barrier; the caller has one between the writes of sh and this
template <int NW, class T> UVC_COLL T waves_total(const T *sh) {
    T s = sh[0];
#pragma unroll
    for (int q = 1; q < NW; q++) s += sh[q];
    return s;
}
// v is wave-uniform (a wave_sum, a count of ballot bits): the block's sum, valid in THREAD 0 ONLY.  ONE barrier; other threads may pass it
// while thread 0 still reads sh, so sh is not written again before a further barrier.
template <int NW, class T> UVC_COLL T waves_sum(T v, T *sh) {
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return threadIdx.x == 0 ? waves_total<NW>(sh) : (T)0;
}
// block-wide sums of NC values per thread through sh[NC][NW]: v[c] becomes the sum, valid in THREAD 0 ONLY.  ONE barrier for all columns;
// sh is not written again before a further barrier.
template <int NW, int NC, class T> UVC_COLL void block_sums(T (&v)[NC], T (*sh)[NW]) {
#pragma unroll
    for (int c = 0; c < NC; c++) v[c] = wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) { for (int c = 0; c < NC; c++) sh[c][threadIdx.x >> 6] = v[c]; }
    __syncthreads();
    if (threadIdx.x == 0) { for (int c = 0; c < NC; c++) v[c] = waves_total<NW>(sh[c]); }
}

// ---- exclusive scan over the block's threads (thread order), one value per thread, NW waves, scratch sh[NW] per column ----
// In two halves with the CALLER'S __syncthreads() between them, so that any number of columns, of any types, share ONE barrier:
//     x = block_scan_begin(v, sh);     the wave's scan; lane 63 leaves the wave's total in sh[wave]; returns the exclusive prefix inside the wave
//     __syncthreads();
//     x = block_scan_end<NW>(x, sh);     adds the totals of the earlier waves: the exclusive prefix inside the block
// Neither half has a barrier.  block_scan_end and waves_total<NW>(sh) (the block's total, in every thread) read sh: the caller puts a
// barrier between them and the next block_scan_begin on the same scratch.
template <class T> UVC_COLL T block_scan_begin(T v, T *sh) {
    const T incl = wave_incl(v);
    if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = incl;
    return incl - v;
}
template <int NW, class T> UVC_COLL T block_scan_end(T excl, const T *sh) {
    const int wv = (int)(threadIdx.x >> 6);
    // selects over all NW totals, four at a time, instead of a loop up to wv: the four totals of a 256-thread block are one straight-line
    // read, and a 16-wave block keeps four in flight, not fifteen (k_rtr_baq took two VGPRs more fully unrolled)
#pragma unroll 4
    for (int q = 0; q < NW; q++) { if (q < wv) excl += sh[q]; }
    return excl;
}
// The one-value forms: ONE barrier inside, between the halves.  On return other threads may still read sh: a call in a loop, or a second
// call on the same scratch, has a __syncthreads() of the caller's in front of it.
template <int NW, class T> UVC_COLL T block_excl(T v, T *sh) {
    const T x = block_scan_begin(v, sh);
    __syncthreads();
    return block_scan_end<NW>(x, sh);
}
template <int NW, class T> UVC_COLL T block_excl(T v, T *sh, T &total) {   // total: the block's sum, in every thread
    const T x = block_excl<NW>(v, sh);
    total = waves_total<NW>(sh);
    return x;
}
// NC columns of one type through sh[NC][NW]: v[c] becomes its exclusive prefix.  ONE barrier for all columns; sh as above.
template <int NW, int NC, class T> UVC_COLL void block_excl(T (&v)[NC], T (*sh)[NW]) {
#pragma unroll
    for (int c = 0; c < NC; c++) v[c] = block_scan_begin(v[c], sh[c]);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; c++) v[c] = block_scan_end<NW>(v[c], sh[c]);
}

// ---- LDS difference-array tile: d[TILE + 1] holds +v where an interval begins and -v where it ends; the prefix sum over the cells is the
// sum of the v of the intervals that cover a position.  PER consecutive cells per thread (TILE = PER x block size), then the block scan of
// the threads' totals: the value of cell tid * PER + i is block-exclusive-prefix(diff_run's result) + run[i].
// += v on [a, b), a < b, both inside the tile and relative to its begin (b may be TILE: the spare cell)
template <class T> UVC_COLL void diff_put_at(T *d, int a, int b, T v) { atomicAdd(&d[a], v); atomicAdd(&d[b], (T)0 - v); }
// += v on the part of [a, b) that lies in the tile [t0, t1), nothing when there is none
template <class T> UVC_COLL void diff_put(T *d, int t0, int t1, int a, int b, T v) {
    a = (a > t0 ? a : t0); b = (b < t1 ? b : t1);
    if (a < b) diff_put_at(d, a - t0, b - t0, v);
}
// running sums of this thread's PER cells; returns their total, the thread's value in the block scan
template <int PER, class T> UVC_COLL T diff_run(const T *d, T (&run)[PER]) {
    T s = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) { s += d[threadIdx.x * PER + i]; run[i] = s; }
    return s;
}
#endif
