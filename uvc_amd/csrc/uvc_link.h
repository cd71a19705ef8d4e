// uvc_link.h -- the rules of the lazy completion of LINK_M, each once and free of HIP, so that the host code, the kernels and
// tests/native/link_host_main.cpp (host only) read the same text.
// An accumulate leaves the bias counters of LINK_M (its SEG32 / SEG64 cells beyond aDP**, its VQ a1BQ* / a2BQ* cells) complete in the
// 64-position windows with an InDel mark.  A reader of those cells elsewhere names a scope first; the completion pass (k_p2_fast<true, false>,
// or its sparse form k_p2_link_sparse where few windows are asked for: DESIGN 6-r10) then runs the windows of the scope that it has not run
// since the accumulate.  tests/native/link_sparse_main.cpp checks the rules of the sparse form.
#ifndef UVC_LINK_H
#define UVC_LINK_H
#include <stddef.h>
#include <stdint.h>
#include "uvcgpu.h"

#if defined(__HIPCC__)
#define UVC_LINK_FN __host__ __device__ static inline
#else
#define UVC_LINK_FN static inline
#endif

// NONE: the call reads no bias counter of LINK_M outside the windows an accumulate completes.  INDEL: the windows with an InDel (or LINK_NN)
// mark in RegionDev::occ.  POSITIONS: the windows of a list of plane indices.  ALL: every window.
enum { UVC_LINK_NONE = -1, UVC_LINK_INDEL = 0, UVC_LINK_POSITIONS = 1, UVC_LINK_ALL = 2 };

// RegionDev::link_need / link_done live behind the dirty marks (dirty_bytes of them) in one buffer, which one fill zeroes: 8-byte aligned,
// each a multiple of 4 windows long (a block of the wave-per-window form reads its four windows as one word)
UVC_LINK_FN size_t uvc_link_marks_off(size_t dirty_bytes) { return (dirty_bytes + 7) & ~(size_t)7; }
UVC_LINK_FN size_t uvc_link_marks_stride(int64_t nwin) { return ((size_t)nwin + 3 + 7) & ~(size_t)7; }
UVC_LINK_FN size_t uvc_link_marks_bytes(size_t dirty_bytes, int64_t nwin) { return uvc_link_marks_off(dirty_bytes) + 2 * uvc_link_marks_stride(nwin); }

// the completion pass runs window w iff
UVC_LINK_FN bool uvc_link_window_runs(uint8_t need, uint8_t done) { return need && !done; }
// an occ word asks for its window under UVC_LINK_INDEL iff it names a LINK symbol other than LINK_M: only there can the mask of the default
// gate hold two symbols (type_mask / gate_count of uvc_kernels_score.hip)
UVC_LINK_FN bool uvc_link_occ_marks(uint32_t occ) { return ((occ >> UVC_LINK_M) & 0xFEu) != 0; }

// A score request: the default gate opens a LINK group only where the mask holds more than LINK_M, and only with min_altdp_thres > 0 does a
// one-symbol mask give no record.  -A, a normal sample's rescue set and forced sites open groups anywhere.
UVC_LINK_FN int uvc_link_score_scope(int all_out, int should_output_all, int tumor_vcf_is_provided, int64_t n_force_sites, int min_altdp_thres) {
    return (all_out || should_output_all || tumor_vcf_is_provided || n_force_sites > 0 || min_altdp_thres <= 0) ? UVC_LINK_ALL : UVC_LINK_NONE;
}
// A fetch of a whole plane group: the three groups that hold bias counters of LINK_M (BQSUM and the aDP** planes are complete after any accumulate)
UVC_LINK_FN int uvc_link_fetch_scope(int group) { return (group == UVC_F_SEG32 || group == UVC_F_SEG64 || group == UVC_F_VQ) ? UVC_LINK_ALL : UVC_LINK_NONE; }
// uvcgpu_region_fetch_columns (the record writer's read of the planes): the windows of the rows it gathers
UVC_LINK_FN int uvc_link_columns_scope(void) { return UVC_LINK_POSITIONS; }
// uvcgpu_region_check_presence compares zero with non-zero, never a value: it completes nothing, so that the lazy state survives the check
UVC_LINK_FN int uvc_link_presence_scope(void) { return UVC_LINK_NONE; }

// ---- the sparse form of the completion pass: a block per needed window, W waves, wave w on class list w & 3, slice w >> 2 ----
// Behind link_done, in the same buffer and under the same fill: the count of listed windows (one int32 in 8 bytes), then the list itself
// (int32 per window).  k_link_mark appends a window when it is the first to set its need byte, so a window is listed at most once between
// two fills and the list never outgrows nwin entries; the sparse pass walks all of it and leaves at once where link_done is already set.
UVC_LINK_FN size_t uvc_link_list_cnt_off(size_t dirty_bytes, int64_t nwin) { return uvc_link_marks_bytes(dirty_bytes, nwin); }
UVC_LINK_FN size_t uvc_link_list_off(size_t dirty_bytes, int64_t nwin) { return uvc_link_list_cnt_off(dirty_bytes, nwin) + 8; }
UVC_LINK_FN size_t uvc_link_buffer_bytes(size_t dirty_bytes, int64_t nwin) { return uvc_link_list_off(dirty_bytes, nwin) + 4 * (size_t)nwin; }
// slice `slice` of `nslices` of the records [lo, hi) of one class list: contiguous, in order, together exactly [lo, hi), lengths differing by
// at most one (the first (hi - lo) % nslices slices are the longer ones); empty where there are fewer records than slices
UVC_LINK_FN void uvc_link_slice(int lo, int hi, int slice, int nslices, int *slo, int *shi) {
    const int n = (hi > lo ? hi - lo : 0), q = n / nslices, r = n % nslices;
    *slo = lo + slice * q + (slice < r ? slice : r);
    *shi = *slo + q + (slice < r ? 1 : 0);
}
// UVC_LINK_POSITIONS takes the dense form (every window's block or wave looks at its marks) when the list of positions is long: n_xs bounds
// the number of windows from above, and a window of the sparse form costs a whole block
UVC_LINK_FN bool uvc_link_positions_dense(int64_t n_xs, int64_t nwin) { return n_xs * 4 >= nwin; }

// A score request, with what the host knows about where a LINK group can open.  -A, should_output_all and min_altdp_thres <= 0 open groups
// anywhere: ALL.  A normal sample with tumor keys: gate_b opens a LINK group only at a keyed refpos: POSITIONS there.  Forced sites open
// groups at the sites, and the accumulate has completed the InDel windows: POSITIONS at the sites.  A normal sample without keys stays ALL.
UVC_LINK_FN int uvc_link_score_scope_at(int all_out, int should_output_all, int tumor_vcf_is_provided, int64_t n_tumor_keys, int64_t n_force_sites, int min_altdp_thres) {
    if (all_out || should_output_all || min_altdp_thres <= 0) return UVC_LINK_ALL;
    if (tumor_vcf_is_provided) return n_tumor_keys > 0 ? UVC_LINK_POSITIONS : UVC_LINK_ALL;
    return n_force_sites > 0 ? UVC_LINK_POSITIONS : UVC_LINK_NONE;
}

// What a handle remembers: whether every window has been run since the planes were last zeroed.  Later calls then cost nothing.
struct UvcLinkState {
    bool all_done = false;
    void planes_zeroed() { all_done = false; }                    // zero_state, a rebinding reset
    void accumulated(bool eager) { all_done = eager; }            // UVCGPU_LINK=eager runs UVC_LINK_ALL inside the accumulate
    bool wants(bool has_planes, bool planes_released, int scope) const { return scope != UVC_LINK_NONE && has_planes && !planes_released && !all_done; }
    void enqueued(int scope) { if (scope == UVC_LINK_ALL) all_done = true; }
};
#endif
