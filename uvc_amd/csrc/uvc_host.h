// uvc_host.h -- what the other translation units of libuvcgpu.so use of uvc_host.cpp beside the public C ABI (include/uvcgpu.h): the error
// report and the region accessors of the record writer.  Host only (no HIP types): the g++-compiled files include it too.
#ifndef UVC_HOST_H
#define UVC_HOST_H
#include "uvcgpu.h"
#include "uvc_hap.h"

extern "C" {
int uvcgpu_set_error(int code, const char *msg);   // sets the thread's uvcgpu_last_error text; returns `code`
const char *uvcgpu_region_refseq(const uvcgpu_region_t *r, int32_t *beg, int32_t *end);
const int32_t *uvcgpu_region_repeat_tracks(const uvcgpu_region_t *r, int64_t *npos);    // host copy, [UVC_NRTR][npos]; NULL on error
const UvcParams *uvcgpu_region_params(const uvcgpu_region_t *r);
const std::vector<UvcHapLinkHost> *uvcgpu_region_hap_(uvcgpu_region_t *r);   // the three link vectors, NULL on error
int uvcgpu_region_block_stats_(uvcgpu_region_t *r, int32_t refpos_beg, int32_t refpos_end, int32_t *dst);   // 10 ints per position, k_block_stats
int uvcgpu_region_block_stats_windows_(uvcgpu_region_t *r, const int32_t *win, int64_t n_win, int32_t *dst);   // the same for disjoint windows [win[2k], win[2k + 1]), one round trip
}
#endif
