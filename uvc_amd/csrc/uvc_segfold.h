// uvc_segfold.h -- the segmented fold of the fragment profile (uvc_fragprofile.hip), once for its two uses: over the alignments of a
// fragment and over the fragments of a family-strand unit.  Not a scan or reduction of uvc_collectives.h's kind: the lanes of a wave hold
// runs of equal keys (the elements of one object are consecutive) and each run folds on its own.  Device code only, force-inlined; every
// lane of the wave makes the call.
#ifndef UVC_SEGFOLD_H
#define UVC_SEGFOLD_H

#include <hip/hip_runtime.h>

// NP (min, max) pairs per lane.  Lane l ends up with the part of its run that lies in lanes [l, 64): after the step with `off` it holds
// lanes [l, l + 2 off) of the run.  The head lane of a run (lane 0, or a lane whose left neighbour has another key) then holds the whole
// of the run's part in this wave.
template <int NP> __device__ __forceinline__ void seg_fold_minmax(int key, int (&lo)[NP], int (&hi)[NP]) {
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
// is this lane the head of its run
__device__ __forceinline__ bool seg_head(int key) {
    const int prev = __shfl_up(key, 1);   // (the previous lane's key: a neighbour fetch)
    return (threadIdx.x & 63) == 0 || prev != key;
}
#endif
