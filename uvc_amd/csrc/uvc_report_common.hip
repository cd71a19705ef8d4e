// uvc_report_common.hip -- the kernels that several report calls launch: the one-block array scan, the two outer steps of
// the tile scan around it, and the fold of the shard copies of a row.  Their launchers are declared in uvc_launch.h.
#include "uvc_launch.h"
#include "uvc_collectives.h"

namespace {
// The array scan of the reports, one block: in place, a[i] becomes the sum of the elements in front of it, a[n] (one element behind the
// input) their total.  The callable and the MSI call scan their block counts with it (heads in front of block b, at most the positions of
// the call: below 2^31), the site call its waves' row counts, and it is the middle step of the tile scan below.
__global__ void __launch_bounds__(1024) k_block_scan(int *a, int n) {
    __shared__ int sh_wave[16];
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + (int)threadIdx.x;
        const int v = (i < n ? a[i] : 0);
        int total;
        const int excl = block_excl<16>(v, sh_wave, total);
        if (i < n) a[i] = carry + excl;
        carry += total;
        __syncthreads();   // sh_wave is written again in the next round
    }
    if (threadIdx.x == 0) a[n] = carry;
}

// The tile scan: the exclusive prefix of n values in three launches -- the sum of every tile of UVC_SCAN_TILE values, k_block_scan over
// the tile sums, the prefix inside every tile on top of its tile's.  What is scanned: the values as they are, or (chunks) the 64-element
// chunks a length makes, ceil(v / 64), 0 for a length below 1.
DEV int scan_value(const int32_t *in, long long i, long long n, int chunks) {
    if (i >= n) return 0;
    const int v = in[i];
    return chunks ? (v > 0 ? (v + 63) >> 6 : 0) : v;
}
__global__ void __launch_bounds__(UVC_SCAN_TILE) k_tile_sums(const int32_t *in, long long n, int chunks, int32_t *tile_sums) {
    __shared__ int sh_wave[UVC_SCAN_TILE / 64];
    const int total = waves_sum<UVC_SCAN_TILE / 64>(wave_sum(scan_value(in, (long long)blockIdx.x * UVC_SCAN_TILE + threadIdx.x, n, chunks)), sh_wave);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}
// out[i] = the sum of the values in front of i, out[n] = their total; tile_pref: the scanned tile sums.  out may be in (in place)
__global__ void __launch_bounds__(UVC_SCAN_TILE) k_tile_prefix(const int32_t *in, int n, int chunks, const int32_t *tile_pref, int32_t *out) {
    __shared__ int sh_wave[UVC_SCAN_TILE / 64];
    const long long i = (long long)blockIdx.x * UVC_SCAN_TILE + threadIdx.x;
    const int v = scan_value(in, i, n, chunks);
    const int excl = block_excl<UVC_SCAN_TILE / 64>(v, sh_wave);
    if (i < n) out[i] = tile_pref[blockIdx.x] + excl;
    if (i == n - 1) out[n] = tile_pref[blockIdx.x] + excl + v;
}

// Many blocks that flush into one row meet on the same words, and atomics on one word run one after the other (61 ns each).
// The blocks of the error and the read profile then add into `shards` copies of the row (block index modulo shards) and this kernel sums
// the copies into the result: one lane per word, one load after the other (the fragment profile, whose count is a constant, keeps a fold
// of its own with all loads in flight).
__global__ void __launch_bounds__(256) k_sum_fold(const unsigned long long *parts, int shards, int cells, unsigned long long *out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= cells) return;
    unsigned long long v = 0;
    for (int s = 0; s < shards; s++) v += parts[(size_t)s * cells + i];
    out[i] = v;
}
}   // namespace

extern "C" void uvc_launch_block_scan(int *d_a, int n, hipStream_t s) { hipLaunchKernelGGL(k_block_scan, dim3(1), dim3(1024), 0, s, d_a, n); }
extern "C" void uvc_launch_tile_sums(const int32_t *d_in, int64_t n, int chunks, int32_t *d_tile_sums, hipStream_t s) {
    hipLaunchKernelGGL(k_tile_sums, dim3((unsigned)uvc_scan_tiles(n)), dim3(UVC_SCAN_TILE), 0, s, d_in, (long long)n, chunks, d_tile_sums);
}
extern "C" void uvc_launch_tile_prefix(const int32_t *d_in, int n, int chunks, const int32_t *d_tile_pref, int32_t *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_tile_prefix, dim3((unsigned)uvc_scan_tiles(n)), dim3(UVC_SCAN_TILE), 0, s, d_in, n, chunks, d_tile_pref, d_out);
}
extern "C" void uvc_launch_sum_fold(const long long *d_parts, int shards, int cells, long long *d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_fold, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const unsigned long long *)d_parts, shards, cells, (unsigned long long *)d_out);
}
