// uvc_host.cpp -- C ABI of libuvcgpu.so (include/uvcgpu.h): region handles, host-side packing of the
// alns3-equivalent SoA into device records, kernel sequencing on the handle's HIP stream.
// There is no CPU compute fallback in this library: every entry point that computes launches HIP kernels.
#include "uvc_launch.h"
#include "uvc_host.h"
#include "uvc_alloc.h"
#include "uvc_prep.h"
#include "uvc_rtr.h"
#include "uvc_hap.h"
#include "uvc_cpus.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
// C++ exceptions must not cross the C boundary (std::terminate would take the caller's process down): every entry point that allocates
// host memory reports them as an error code instead
template <class F> static int guarded(const char *what, F &&f) {
    try {
        const int rc = f();
        // a HIP call whose failure was handled (or did not matter) still leaves its code in the thread's "last error", where the launch checks of
        // rocPRIM in a later call would find it and refuse: it ends here (UVCGPU_DEBUG names the entry point that left one)
        const hipError_t stale = hipGetLastError();
        if (stale != hipSuccess && getenv("UVCGPU_DEBUG")) fprintf(stderr, "[uvcgpu] %s (rc %d) left HIP error: %s\n", what, rc, hipGetErrorString(stale));
        return rc;
    }
    catch (const std::bad_alloc &) { return fail(UVCGPU_ENOMEM, std::string(what) + ": out of host memory"); }
    catch (const std::exception &e) { return fail(UVCGPU_EDEVICE, std::string(what) + ": " + e.what()); }
}
extern "C" int uvcgpu_set_error(int code, const char *msg) { return fail(code, msg ? msg : ""); }   // for the other translation units of the library
#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(UVCGPU_EDEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

struct uvcgpu_score_stream;
struct uvcgpu_region;
// (the cache hands freed blocks to other handles at once: nothing of this handle may still be running on them)
static void quiesce(const uvcgpu_region *r);   // waits for the handle's streams: main, side and side3
// The two owners of a handle's memory.  Device memory comes from the caching allocator (uvc_alloc.h: freed blocks are reused without the
// device-wide synchronisation of hipFree), page-locked memory from the runtime; both wait for the handle's streams before a block goes back.
// A buffer that is grown on demand: p holds cap units of the size the site's fit() calls name (bytes, elements or records).
template <class T, bool HOST = false> struct Buf {
    const uvcgpu_region *r; T *p = nullptr; size_t cap = 0;
    explicit Buf(const uvcgpu_region *r_) : r(r_) {}
    Buf(const Buf &) = delete; Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    operator T *() const { return p; }
    static hipError_t raw_alloc(void **q, size_t bytes) { return HOST ? hipHostMalloc(q, bytes, hipHostMallocDefault) : uvc_dev_malloc(q, bytes); }
    static hipError_t raw_free(void *q) { return HOST ? hipHostFree(q) : uvc_dev_free(q); }
    void release() { if (p) { quiesce(r); (void)raw_free(p); } p = nullptr; cap = 0; }
    // It stays when it holds `need` units and, with keep_max, no more than keep_max; else it is released and allocated anew with `slack` units
    // on top.  Pointer and capacity change together: both are clear after a failure, whose bytes *bytes then names.
    hipError_t fit(size_t need, size_t slack = 0, size_t keep_max = 0, size_t unit = sizeof(T), size_t *bytes = nullptr) {
        if (cap >= need && !(keep_max && cap > keep_max)) return hipSuccess;
        release();
        const size_t want = (need + slack) * unit;
        if (bytes) *bytes = want;
        const hipError_t e = raw_alloc((void **)&p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        cap = need + slack;
        return hipSuccess;
    }
};
// Device allocations that are made one by one and freed together: the read-dependent arrays of a handle, the temporaries of one call.
struct Pool {
    const uvcgpu_region *r; std::vector<void *> blocks; hipError_t last = hipSuccess;
    explicit Pool(const uvcgpu_region *r_) : r(r_) {}
    Pool(const Pool &) = delete; Pool &operator=(const Pool &) = delete;
    ~Pool() { clear(); }
    void *get(size_t bytes) { void *q = nullptr; last = uvc_dev_malloc(&q, bytes); if (last != hipSuccess) return nullptr; blocks.push_back(q); return q; }
    template <class T> bool get(T **out, size_t count) { *out = (T *)get(count * sizeof(T)); return *out != nullptr; }
    void clear() { if (!blocks.empty()) quiesce(r); for (void *q : blocks) (void)uvc_dev_free(q); blocks.clear(); }
};

struct uvcgpu_region {
    UvcParams P;
    int32_t tid, beg, end;     // state covers [beg, end): end = caller's end + 1 (main.cpp:569)
    int64_t npos;
    std::string refstring;
    std::vector<int32_t> h_rtr; bool h_rtr_valid = false;   // host copy of the repeat tracks as built (begpos / tracklen / unitlen planes), fetched when the record writer first asks
    UvcRtrWork rw; Buf<char> d_rtrwork{this}; bool thr_ready = false;   // scratch of the side-array kernels (uvc_rtr.hip)
    Buf<char, true> h_ref{this};                                        // page-locked staging of the reference characters
    hipStream_t stream = nullptr;
    // the streams (the main one first) and the events of a handle: created and destroyed in one loop over these lists
    std::array<hipStream_t *, 3> streams() { return { { &stream, &side, &side3 } }; }
    std::array<hipEvent_t *, 8> events() { return { { &e_fork, &e_join, &e_fork2, &e_join3, &e_stat, &e_alleles, &e_link_fork, &e_link_join } }; }
    hipStream_t side = nullptr, side3 = nullptr; hipEvent_t e_fork = nullptr, e_join = nullptr, e_fork2 = nullptr, e_join3 = nullptr, e_stat = nullptr, e_alleles = nullptr, e_link_fork = nullptr, e_link_join = nullptr;   // fork/join inside accumulate (see uvc_launch_accumulate)
    // device buffers
    Buf<uint8_t> d_refsym{this}; Buf<int32_t> d_rtr{this}, d_rtr0{this}, d_fsum{this}, d_win{this}; Buf<int64_t> d_baq{this};
    Buf<char> d_state{this}; SlabLayout L = {};   // the plane slab and its layout for npos (uvc_planes.h)
    Buf<int32_t> d_err{this};     // RegionDev::err
    int64_t npos_cap = 0;         // positions the side arrays and the slab were allocated for (uvcgpu_region_reset reuses them)
    bool buckets_clean = false;   // the transient bucket planes (tail of the slab) are left zero by P3b / P5b
    Pool owned{this};             // read-dependent device allocations
    RegionDev R;
    int32_t *d_dup_units = nullptr; int64_t *d_dup_off = nullptr; int n_dup = 0; int64_t n_dup_work = 0;
    bool has_reads = false, accumulated = false;
    UvcLinkState link; int link_split = 0;   // the completion pass of LINK_M has been to every window (link_complete); the form the accumulate took (UVCGPU_SPLIT)
    bool reads_given = false;    // set_reads went through for the present region, with or without reads (uvcgpu_region_family_stats)
    // zero fill without what the last accumulate left untouched (RegionDev::dirty, uvc_launch_zero_state)
    Buf<uint8_t> d_dirty{this}; Buf<ZeroPlane> d_zero_planes{this}; int64_t zero_planes_npos = 0;
    int64_t dirty_npos = 0;      // the region length under which the slab's contents and the marks were written; 0: unknown, fill everything
    bool state_released = false, state_zeroed = false;   // UvcScoreRequest::release_state: planes given up / already zeroed on the side stream (e_join marks the end)
    int64_t last_scored = 0, last_returned = 0;   // record counts of the last score call (uvcgpu_region_last_score_counts)
    size_t zeroed_bytes = 0;     // with state_zeroed: the slab is zero from its start up to here (a rebind to a region that fits keeps the benefit)
    RawReads W;                  // per-read input columns on the device (kept: uvcgpu_region_correct_bq re-derives the per-read records)
    int32_t *d_p2[4] = { nullptr, nullptr, nullptr, nullptr };   // P2 work list: alignment, begin, end, query offset
    int64_t n_bases = 0;
    UvcProf prof;
    // persistent scoring buffers (grown on demand)
    Buf<char> d_score_scratch{this};   // (cap: bytes)
    Buf<int32_t> d_score_fields{this}; int64_t *d_score_count = nullptr;   // (cap: records)
    Buf<uint8_t, true> h_stage{this};   // page-locked staging for the small per-call uploads of score (tumor keys, caller's alleles): never the caller's own pages
    Buf<int32_t> d_score_kept{this};   // UvcScoreRequest::kept_only: the compacted copy, same pitch as d_score_fields (cap: records)
    Buf<char> d_report{this}; Buf<char, true> h_report{this};   // the report calls (uvcgpu_region_coverage, _error_profile, _family_stats, _callable, _read_profile, _msi, _fragment_profile, _site_reads, _clip_sites, _clip_junctions, _clip_mates, _family_concordance): range list + pieces on the device, page-locked result (grown on demand)
    uvcgpu_score_stream *ss = nullptr;   // the streamed score of this handle: its two row sets and page-locked buffers outlive a stream (reused by the next one)
    // InDel allele tables of the last accumulate (built on first use by gap_tables)
    bool gap_ready = false;
    std::vector<UvcGapRow> gap_rows; std::vector<uint8_t> gap_seq;
    std::vector<UvcIndelAllele> gap_alleles; std::vector<int32_t> gap_allele_row;   // what indel_get_majority yields, sorted by (refpos, symbol)
    Buf<UvcIndelAllele> d_gap_alleles{this}; Buf<int32_t> d_gap_allele_row{this}; Buf<UvcGapRow> d_gap_rows{this}; Buf<uint8_t> d_gap_seq{this};   // device copies for k_call
    // haplotype links of the last accumulate (built on first use by hap_tables): hap_bq, hap_fq, hap_f2q of updateByRegion3Aln
    bool hap_ready = false;
    std::vector<UvcHapLinkHost> hap[3];
};

static bool stream_is_open(const uvcgpu_region *r);   // a streamed score is open on the handle: accumulate, reset, set_reads and the one-call scores wait for its end
static void stream_destroy(uvcgpu_region *r);
static void quiesce(const uvcgpu_region *r) { for (hipStream_t s : { r->stream, r->side, r->side3 }) if (s) (void)hipStreamSynchronize(s); }
// A reader of the accumulated planes: they exist and the last score did not release them.  `call` heads the text (the calls differ in it alone).
static int planes_guard(const uvcgpu_region *r, const char *call) {
    if (!r->accumulated) return fail(UVCGPU_ESTATE, std::string(call) + " before accumulate");
    if (r->state_released) return fail(UVCGPU_ESTATE, "the planes were released by the last score (UvcScoreRequest::release_state)");
    return 0;
}

// UVCGPU_TIMING (diagnosis; the one read-back of this path): how many windows the completion pass has been to since the accumulate.  It waits for
// the handle's stream and copies nwin bytes back, behind every accumulate and every link_complete: a UVCGPU_TIMING run is no timing of the step
// (the forms lines it prints are for tests and diagnosis; time with the profiler or uvcgpu_region_set_profiling)
static void link_report(const uvcgpu_region *r, const char *scope) {
    std::vector<uint8_t> done((size_t)r->R.nwin);
    if (hipStreamSynchronize(r->stream) != hipSuccess || hipMemcpy(done.data(), r->R.link_done, done.size(), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
    long long n = 0;
    for (uint8_t b : done) n += (b != 0);
    fprintf(stderr, "[uvcgpu link_complete] scope=%s done=%lld of %d windows\n", scope, n, (int)r->R.nwin);
}
// The bias counters of LINK_M (its SEG32 / SEG64 cells beyond aDP**, its VQ a1BQ* / a2BQ* cells) are made where somebody reads them: an
// accumulate leaves them complete in the 64-position windows with an InDel mark, which is all the default gate reads.  Every other reader
// of those cells calls this first, behind planes_guard: it enqueues the completion pass for the windows of `scope` on the handle's stream,
// once per window and accumulate.  d_xs: n_xs positions on the device (UVC_LINK_POSITIONS), read in place: xs_stride int32 words apart, xs_off
// above their plane index.  Nothing is read back.
static int link_complete(uvcgpu_region *r, int scope, const int32_t *d_xs = nullptr, int64_t n_xs = 0, int xs_stride = 1, int xs_off = 0) {
    if (!r->link.wants(r->accumulated, r->state_released, scope)) return 0;
    uvc_launch_link_complete(&r->R, &r->P, r->link_split, scope, d_xs, n_xs, xs_stride, xs_off, "k_p2_fast_link", nullptr, r->stream);
    if (hipGetLastError() != hipSuccess) return fail(UVCGPU_EDEVICE, "completion pass of LINK_M: launch failed");
    r->link.enqueued(scope);
    if (getenv("UVCGPU_TIMING")) link_report(r, scope == UVC_LINK_ALL ? "all" : "positions");
    return 0;
}

// ---------------------------------------------------------------- region side arrays (a3) ---
// refstring2repeatvec (main.hpp:803-874) + region_repeatvec_to_baq_offsetarr (main.cpp:400-429) run on the device (uvc_rtr.hip); the host
// only stages the reference characters and, once per handle, turns indel_phred (main.hpp:794-801) into its threshold table.
namespace {
// device allocation without a host image (the prelude kernels write every element); optionally zero-filled on the stream
template <class T> int dev_alloc(uvcgpu_region *r, size_t count, T **out, bool zero = false) {
    const size_t n = std::max<size_t>(count, 1);
    if (!r->owned.get(out, n)) return fail(UVCGPU_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(r->owned.last));
    if (zero && hipMemsetAsync(*out, 0, n * sizeof(T), r->stream) != hipSuccess) return fail(UVCGPU_EDEVICE, "hipMemsetAsync");
    return 0;
}
void free_reads(uvcgpu_region *r) { r->owned.clear(); r->has_reads = false; r->reads_given = false; r->accumulated = false; }
}  // namespace

extern "C" {

const char *uvcgpu_last_error(void) { return g_err.c_str(); }
const char *uvcgpu_version(void) { return "uvcgpu 0.1 (gfx950)"; }

int uvcgpu_init(int device_id) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(UVCGPU_EDEVICE, "no HIP device: libuvcgpu has no CPU fallback");
    HIP_OK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) return fail(UVCGPU_EDEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    return 0;
}

int uvcgpu_device_memory(int64_t *free_bytes, int64_t *total_bytes) {
    size_t fr = 0, tot = 0;
    HIP_OK(hipMemGetInfo(&fr, &tot));
    if (free_bytes) *free_bytes = (int64_t)fr;
    if (total_bytes) *total_bytes = (int64_t)tot;
    return 0;
}

int uvcgpu_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }

void uvcgpu_params_default(UvcParams *p) {
    memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(UvcParams);
#define UVC_PI(name, dflt) p->name = (int32_t)(dflt);
#define UVC_PD(name, dflt) p->name = (double)(dflt);
#include "uvc_params.def"
#undef UVC_PI
#undef UVC_PD
}

static void platform_deltas(UvcParams *p, int32_t platform) {   // CmdLineArgs.cpp:13-15, 113-134
    auto dec = [](int32_t &a, int32_t b) { a = a - std::min(a, b); };
    if (platform == UVC_PLATFORM_IONTORRENT) {
        p->bq_phred_added_misma += 8;
        dec(p->fam_thres_highBQ_snv, 30); dec(p->fam_thres_highBQ_indel, 30); dec(p->bias_thres_PFBQ1, 30); dec(p->bias_thres_PFBQ2, 30); dec(p->bias_thres_highBQ, 13);
    } else if (platform == UVC_PLATFORM_ILLUMINA) {
        p->syserr_minABQ_pcr_snv += 200; p->syserr_minABQ_pcr_indel += 100; p->syserr_minABQ_cap_snv += 200; p->syserr_minABQ_cap_indel += 100;
    }
}

void uvcgpu_params_apply_platform(UvcParams *p, int32_t platform, int32_t central_readlen, int32_t max_mapq) {   // CmdLineArgs.cpp:13-15, 50-134
    p->inferred_sequencing_platform = platform;
    if (0 == p->central_readlen) p->central_readlen = central_readlen;
    p->inferred_maxMQ = std::max(p->inferred_maxMQ, max_mapq);
    platform_deltas(p, platform);
}

// selfUpdateByPlatform (CmdLineArgs.cpp:37-134): AUTO and OTHER infer from the file, OTHER keeps the deltas off; ILLUMINA and IONTORRENT
// are taken as given and the file is not read (central_readlen and inferred_maxMQ keep the caller's values)
int uvcgpu_params_apply_platform_ex(UvcParams *p, int32_t sequencing_platform, int32_t inferred, int32_t central_readlen, int32_t max_mapq) {
    if (!p || sequencing_platform < UVC_PLATFORM_AUTO || sequencing_platform > UVC_PLATFORM_OTHER) return fail(UVCGPU_EINVAL, "sequencing platform outside 0..3");
    if (sequencing_platform == UVC_PLATFORM_ILLUMINA || sequencing_platform == UVC_PLATFORM_IONTORRENT) {
        p->inferred_sequencing_platform = sequencing_platform;
        platform_deltas(p, sequencing_platform);
    } else if (sequencing_platform == UVC_PLATFORM_AUTO) {
        uvcgpu_params_apply_platform(p, inferred, central_readlen, max_mapq);
    } else {
        p->inferred_sequencing_platform = inferred;
        if (0 == p->central_readlen) p->central_readlen = central_readlen;
        p->inferred_maxMQ = std::max(p->inferred_maxMQ, max_mapq);
    }
    return 0;
}

// RegionDev::link_need / link_done in the buffer of the dirty marks: 8-byte aligned, a multiple of 4 windows each (k_p2_fast reads a block's four as one word)
static size_t dirty_bytes(const RegionDev &R) { return (size_t)3 * NSYM * (size_t)R.ndblk; }
// (Re)binds a handle to a region: side arrays of the reference (C10) and the plane layout.  Device buffers are kept when they are large
// enough, so that a caller that streams tiles of one size through a handle pays hipMalloc / hipFree once (uvcgpu_region_reset).
static int configure_region(uvcgpu_region *r, int32_t tid, int32_t beg, int32_t end, const char *refseq) {
    r->tid = tid; r->beg = beg; r->end = end + 1; r->npos = (int64_t)end - beg + 1;
    r->refstring.assign(refseq, (size_t)(end - beg));
    r->accumulated = false; r->gap_ready = false; r->hap_ready = false; r->state_released = false;
    r->h_rtr_valid = false;
    r->L = slab_layout(r->npos);   // one slab for all per-position planes (+ the transient bucket planes)
    // planes that the last score zeroed on the side stream (release_state) stay zero under the new layout when it fits into what was zeroed
    r->state_zeroed = r->state_zeroed && r->npos <= r->npos_cap && r->L.total <= r->zeroed_bytes;
    r->buckets_clean = r->state_zeroed;
    const int vmax = r->P.indel_vntr_repeatsize_max, smax = r->P.indel_str_repeatsize_max, bqm = r->P.indel_BQ_max;
    const size_t n_rtr = (size_t)UVC_NRTR * r->npos, n = (size_t)r->npos;
    if (r->npos > r->npos_cap) {   // every buffer to the new length exactly
        r->npos_cap = 0; r->dirty_npos = 0; r->thr_ready = false;
        size_t scan_tmp = 0;
        const size_t work_bytes = uvc_rtr_work_bytes(r->npos, vmax, smax, bqm, &scan_tmp);
        if (r->d_refsym.fit(n + 1) != hipSuccess || r->d_rtr.fit(n_rtr) != hipSuccess || r->d_rtr0.fit(n_rtr) != hipSuccess || r->d_fsum.fit(2 * UVC_FSUM_N * n) != hipSuccess
            || r->d_win.fit(16 * (size_t)((r->npos + 63) / 64)) != hipSuccess || r->d_baq.fit(2 * n) != hipSuccess || r->d_state.fit(r->L.total) != hipSuccess || r->d_rtrwork.fit(work_bytes) != hipSuccess
            || r->d_dirty.fit(uvc_link_buffer_bytes((size_t)3 * NSYM * (size_t)((r->npos >> UVC_DIRTY_SHIFT) + 2), (r->npos + 63) / 64)) != hipSuccess) return fail(UVCGPU_ENOMEM, "hipMalloc(region planes) failed");
        uvc_rtr_bind(&r->rw, r->d_rtrwork, r->npos, vmax, smax, bqm, scan_tmp);
        r->npos_cap = r->npos;
    }
    if (!r->thr_ready) {   // parameters only: once per handle (and again when the scratch moved)
        std::vector<int32_t> thr((size_t)smax * bqm);
        uvc_rtr_thresholds(&r->P, thr.data());
        HIP_OK(hipMemcpy(r->rw.thr, thr.data(), sizeof(int32_t) * thr.size(), hipMemcpyHostToDevice));
        r->thr_ready = true;
    }
    // the reference characters travel from page-locked memory of the handle, so that the copy is a stream operation like the kernels behind it
    const size_t n_ref = (size_t)(end - beg);
    if (r->h_ref.fit(n_ref) != hipSuccess) return fail(UVCGPU_ENOMEM, "hipHostMalloc(reference staging) failed");
    memcpy(r->h_ref, refseq, n_ref);
    HIP_OK(hipMemcpyAsync(r->rw.refchar, r->h_ref, n_ref, hipMemcpyHostToDevice, r->stream));
    {
        const int e = uvc_launch_region_tracks(&r->rw, &r->P, r->npos, r->d_refsym, r->d_rtr0, r->d_baq, r->stream);
        if (e) return fail(UVCGPU_EDEVICE, std::string("side-array kernels: ") + hipGetErrorString((hipError_t)e));
    }
    RegionDev &R = r->R;
    memset(&R, 0, sizeof(R));
    R.beg = r->beg; R.end = r->end; R.npos = r->npos; R.refsym = r->d_refsym; R.rtr = r->d_rtr; R.baq = r->d_baq; R.fsum = r->d_fsum; R.win = r->d_win; R.nwin = (int32_t)((r->npos + 63) / 64);
    char *b = r->d_state;
#define X(g, m) R.m = (decltype(R.m))(b + r->L.off[UVC_F_##g]);
    UVC_SLAB_MEMBERS(X)
#undef X
    R.bucket = (int32_t *)(b + r->L.bucket_off); R.p5flag = (uint8_t *)(b + r->L.p5flag_off); R.occ = (uint32_t *)(b + r->L.occ_off);
    R.dirty = r->d_dirty; R.ndblk = (int32_t)((r->npos + ((int64_t)1 << UVC_DIRTY_SHIFT) - 1) >> UVC_DIRTY_SHIFT);
    R.link_need = r->d_dirty + uvc_link_marks_off(dirty_bytes(R)); R.link_done = R.link_need + uvc_link_marks_stride(R.nwin);   // behind the dirty marks: one fill zeroes both
    R.link_cnt = (int32_t *)(r->d_dirty + uvc_link_list_cnt_off(dirty_bytes(R), R.nwin)); R.link_list = (int32_t *)(r->d_dirty + uvc_link_list_off(dirty_bytes(R), R.nwin));   // (the same fill)
    r->link.planes_zeroed();
    R.err = r->d_err;
    HIP_OK(hipMemsetAsync(R.err, 0, 4, r->stream));
    return 0;   // nothing to wait for: the staging memory belongs to the handle and a handle is rebound only when its streams are idle
}

static int uvcgpu_region_create_impl(uvcgpu_region_t **out, const UvcParams *params, int32_t tid, int32_t beg, int32_t end, const char *refseq) {
    if (!out || !params || !refseq || end <= beg) return fail(UVCGPU_EINVAL, "bad argument");
    if (const int rc = uvcgpu_params_check(params)) return rc;   // uvc_params.cpp: the value refusals, also for callers that check before they open anything
    uvcgpu_region *r = new uvcgpu_region();
    memset(&r->prof, 0, sizeof(r->prof));
    memset(&r->R, 0, sizeof(r->R));
    r->P = *params;
    // UVCGPU_ONE_STREAM=1 (diagnosis): the main stream alone, every kernel of a handle runs there (uvc_launch_accumulate and score see no side
    // stream), so that UVCGPU_TIMING shows undisturbed durations
    const bool one_stream = (getenv("UVCGPU_ONE_STREAM") != nullptr);
    for (hipStream_t *s : r->streams()) {
        const bool main = (s == &r->stream);
        if (!main && one_stream) break;
        if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) { uvcgpu_region_destroy(r); return fail(UVCGPU_EDEVICE, main ? "hipStreamCreate failed (no GPU?)" : "hipStreamCreate / hipEventCreate failed"); }
    }
    if (!one_stream) for (hipEvent_t *e : r->events()) if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { uvcgpu_region_destroy(r); return fail(UVCGPU_EDEVICE, "hipStreamCreate / hipEventCreate failed"); }
    if (r->d_err.fit(1) != hipSuccess) { uvcgpu_region_destroy(r); return fail(UVCGPU_ENOMEM, "hipMalloc failed"); }
    const int rc = configure_region(r, tid, beg, end, refseq);
    if (rc) { uvcgpu_region_destroy(r); return rc; }
    *out = r;
    return 0;
}

// The same handle for another region (the next tile): reads, results and the plane contents of the previous region are dropped, streams,
// events and -- when the new region is not longer than the longest one the handle has seen -- the device buffers are kept.
static int uvcgpu_region_reset_impl(uvcgpu_region_t *r, int32_t tid, int32_t beg, int32_t end, const char *refseq) {
    if (!r || !refseq || end <= beg) return fail(UVCGPU_EINVAL, "bad argument");
    if (stream_is_open(r)) return fail(UVCGPU_ESTATE, "reset while a score stream is open");
    HIP_OK(hipStreamSynchronize(r->stream));
    if (r->side) HIP_OK(hipStreamSynchronize(r->side));
    if (r->side3) HIP_OK(hipStreamSynchronize(r->side3));
    free_reads(r);
    return configure_region(r, tid, beg, end, refseq);
}

// The read-dependent preparation runs on the device (uvc_prep.hip) over the caller's columns; `d` holds DEVICE pointers.
static void *prep_alloc(void *ctx, size_t bytes, int zero) {
    uvcgpu_region *r = (uvcgpu_region *)ctx;
    char *p = nullptr;
    if (dev_alloc(r, bytes, &p, zero != 0)) return nullptr;
    return p;
}
static int set_reads_on_device(uvcgpu_region_t *r, const UvcReadSoA *d, bool timing, std::chrono::steady_clock::time_point t_prev) {
    auto lap = [&](const char *what) { if (!timing) return; hipStreamSynchronize(r->stream); const auto t = std::chrono::steady_clock::now();
                                       fprintf(stderr, "[uvcgpu set_reads] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count()); t_prev = t; };
    const int64_t n = d->n_reads;
    if (r->npos >= ((int64_t)1 << 29)) return fail(UVCGPU_EUNSUPPORTED, "region longer than 2^29");
    if (d->n_bases >= ((int64_t)1 << 31)) return fail(UVCGPU_EUNSUPPORTED, "more than 2^31 read bases in one region: split the region");
    if (!d->bases && !d->bases4 && d->n_bases > 0) return fail(UVCGPU_EINVAL, "neither bases nor bases4");
    // compact input forms: offsets as prefix sums of l_qseq / n_cigar, BAM's 4-bit base codes unpacked on the device
    UvcReadSoA dd = *d;
    int32_t *d_bad = nullptr; uint16_t *bq_done = nullptr;
    if (!d->seq_off || !d->cigar_off || !d->bases) {
        int rc0;
        int64_t *so = nullptr, *co = nullptr, *b4o = nullptr; uint8_t *ub = nullptr; char *tmp = nullptr;
        const size_t tb = uvc_prep_compact_tmp_bytes(n);
        if ((rc0 = dev_alloc(r, tb, &tmp)) || (rc0 = dev_alloc(r, 2, &d_bad, true))) return rc0;   // [0] malformed input, [1] a quality byte of 0
        if (!d->seq_off && (rc0 = dev_alloc(r, (size_t)n, &so))) return rc0;
        if (!d->cigar_off && (rc0 = dev_alloc(r, (size_t)n, &co))) return rc0;
        if (!d->bases && ((rc0 = dev_alloc(r, (size_t)n, &b4o)) || (rc0 = dev_alloc(r, (size_t)std::max<int64_t>(d->n_bases, 1), &ub)) || (rc0 = dev_alloc(r, (size_t)std::max<int64_t>(d->n_bases, 1), &bq_done)))) return rc0;
        const int e = uvc_prep_compact(d->l_qseq, d->n_cigar, n, d->n_bases, d->bases ? nullptr : d->bases4, d->n_bases4_bytes, d->quals, so, d->seq_off, co, b4o, ub, bq_done, d_bad, tmp, tb, r->stream);
        if (e) return fail(UVCGPU_EDEVICE, std::string("offset scans: ") + hipGetErrorString((hipError_t)e));
        if (so) dd.seq_off = so;
        if (co) dd.cigar_off = co;
        if (ub) dd.bases = ub;
        d = &dd;
    }
    UvcPrepIn in; memset(&in, 0, sizeof(in));
    in.n_reads = n; in.n_bases = d->n_bases; in.n_cigar_ops = d->n_cigar_ops; in.n_fams = d->n_fams;
    in.pos = d->pos; in.mpos = d->mpos; in.isize = d->isize; in.nm = d->nm; in.l_qseq = d->l_qseq; in.n_cigar = d->n_cigar; in.frag_id = d->frag_id; in.fam_id = d->fam_id;
    in.flag = d->flag; in.mapq = d->mapq; in.fam_strand = d->fam_strand; in.fam_dflag = d->fam_dflag; in.seq_off = d->seq_off; in.cigar_off = d->cigar_off; in.cigars = d->cigars;
    // base | quality is packed in front of the preparation: the packing kernels say whether the column has a quality byte of 0 at all
    // (UvcPrepIn::zero_qual), which decides whether the fragments' qualities are looked at there
    uint16_t *bq_packed = bq_done;
    if (!bq_packed) {
        int rc1;
        if ((rc1 = dev_alloc(r, (size_t)std::max<int64_t>(d->n_bases, 1), &bq_packed))) return rc1;
        if (!d_bad && (rc1 = dev_alloc(r, 2, &d_bad, true))) return rc1;
        uvc_launch_pack_bq(d->bases, d->quals, bq_packed, d->n_bases, d_bad, r->stream);
    }
    in.quals = d->quals; in.zero_qual = d_bad + 1;
    UvcPrepOut o; char msg[256];
    int rc = uvc_prep_reads(&in, &r->P, r->beg, r->end, r->npos, prep_alloc, r, r->stream, &o, msg, (int)sizeof(msg));
    if (rc) return fail(rc, msg);
    lap("nesting + CIGAR facts (device)");
    RegionDev &R = r->R;
    RawReads &W = r->W;
    W.pos = d->pos; W.endpos = o.endpos; W.mpos = d->mpos; W.isize = d->isize; W.flag = d->flag; W.mapq = d->mapq; W.nm = d->nm; W.l_qseq = d->l_qseq; W.n_cigar = d->n_cigar;
    W.frag = o.frag_of; W.fs = o.fs_of; W.dflag = o.dflag_of; W.kind = o.kind; W.seq_off = d->seq_off; W.cigar_off = d->cigar_off; W.table_off = o.table_off; W.item_off = o.item_off; W.gap_off = o.gap_off;
    R.bases = d->bases; R.quals = d->quals; R.cigars = d->cigars;
    R.frag_off[0] = 0; R.frag_off[1] = o.n_frag_strand0; R.frag_off[2] = o.n_frags;
    const int64_t n_simple = o.n_simple; const size_t nf = (size_t)o.n_frags;
    R.bq = bq_packed; R.bq_bytes = (uint32_t)(d->n_bases * 2);   // (with bases4: packed while the 4-bit bases were unpacked)
    { AlnRec *a; if ((rc = dev_alloc(r, (size_t)n, &a))) return rc; R.alns = a; R.n_alns = (int32_t)n; }
    R.n_fast = (int32_t)n_simple;
    R.complex_ids = o.complex_ids; R.n_complex = o.n_complex;
    R.frags = o.frags; R.n_frags = o.n_frags;
    int pos_bits = 1; while (((int64_t)1 << pos_bits) < r->npos + 1) pos_bits++;   // every sorted position offset is < npos: the radix passes stop there
    {   // stable device sort of the fragments by (strand, begin) -- k_frag walks two beg-sorted sub-lists, one per strand, so that the
        // strand-specific accumulators are fixed registers
        const size_t nmax = std::max<size_t>(nf, 1);
        int32_t *d_fsorted, *d_frank; uint32_t *work; uint8_t *tmp;
        const size_t tmp_bytes = uvc_sort32_tmp_bytes(nmax);
        if ((rc = dev_alloc(r, nf, &d_fsorted)) || (rc = dev_alloc(r, nf, &d_frank)) || (rc = dev_alloc(r, 4 * nmax, &work)) || (rc = dev_alloc(r, tmp_bytes + 16, &tmp))) return rc;
        if (uvc_sort_by_pos_cls(o.frag_beg, o.frag_strand, r->beg, pos_bits, 1, (int64_t)nf, work, tmp, tmp_bytes, r->stream) != 0) return fail(UVCGPU_EDEVICE, "device sort of the fragments failed");
        uvc_launch_rank_from_sorted(work + 3 * nf, (int64_t)nf, (int64_t)nf, d_fsorted, d_frank, r->stream);
        R.frag_sorted = d_fsorted; R.frag_rank = d_frank;
    }
    { FragFast *f; if ((rc = dev_alloc(r, nf, &f, true))) return rc; R.ffast = f; }
    { FragUnit *f; if ((rc = dev_alloc(r, nf, &f, true))) return rc; R.ffast_u = f; }
    R.sweep_frags = o.sweep_frags; R.n_sweep = o.n_sweep;
    { int32_t *q; if ((rc = dev_alloc(r, nf * (size_t)(UVC_MAXEV + 2) + 1, &q, true))) return rc;
      R.frag_nmut = q; R.frag_mut = q + nf; R.overflow_frags = q + nf * (size_t)(UVC_MAXEV + 1); R.n_overflow = q + nf * (size_t)(UVC_MAXEV + 2); }
    R.fss = o.fss; R.n_fs = o.n_fs;
    R.generic_fs = o.generic_fs; R.n_generic_fs = o.n_generic; R.n_generic_work = o.work;
    R.generic_sorted = o.generic_sorted; R.max_unit_span = o.max_unit_span;
    R.frag32 = (getenv("UVCGPU_FRAG32") != nullptr);
    // The form of the family passes, decided here once: deep data (more than 8 (unit, position) cells per position) takes the digest form, with
    // 32 B per cell so that P5 and the duplex pass do not walk the fragments again; shallow data, a digest above 48 GB, a unit with too many
    // fragments for the digest's vote counts, or UVCGPU_FAM_PATH=generic (the tests' reference form) the generic form.  The two give identical
    // planes (tests/test_gpu_fullsize.py).
    const char *fam_path = getenv("UVCGPU_FAM_PATH");
    const bool generic_forced = (fam_path && !strcmp(fam_path, "generic"));
    R.fam_digest = nullptr;
    if (!generic_forced && o.work > 8 * r->npos && (size_t)o.work * 32 <= ((size_t)48 << 30) && o.max_unit_frags < UVC_DIGEST_MAX_VOTES) {
        uint32_t *q = nullptr; if ((rc = dev_alloc(r, (size_t)o.work * 8, &q))) return rc; R.fam_digest = q;
    }
    if (timing) fprintf(stderr, "[uvcgpu set_reads] %d fragments, %d units, %d generic units, %lld (unit, position) cells, longest unit %d, most fragments in a unit %d, %lld positions, family form %s\n",
                        o.n_frags, o.n_fs, o.n_generic, (long long)o.work, o.max_unit_span, o.max_unit_frags, (long long)r->npos, R.fam_digest ? "digest" : "generic");
    { Contrib *t; if ((rc = dev_alloc(r, (size_t)std::max<int64_t>(o.table_rows, 1), &t))) return rc; R.table = t; }
    { int32_t *t; if ((rc = dev_alloc(r, (size_t)(o.gap_slots + 2 * (int64_t)o.n_complex + 4), &t))) return rc; R.ir_list = t; }
    { Item *t; if ((rc = dev_alloc(r, (size_t)std::max<int64_t>(o.item_slots, 1), &t))) return rc; R.items = t;
      int32_t *c; if ((rc = dev_alloc(r, (size_t)o.n_complex + 1, &c, true))) return rc; R.item_cnt = c; }
    {   // InDel allele pipeline (k_gap_*): events, two sort stages, rows
        const int64_t gap_slots = o.gap_slots, ins_total = o.ins_total;
        if (gap_slots >= ((int64_t)1 << 27)) return fail(UVCGPU_EUNSUPPORTED, "more than 2^27 InDel ops in one region");
        if (gap_slots > 0 && r->npos >= ((int64_t)1 << 26)) return fail(UVCGPU_EUNSUPPORTED, "region longer than 2^26 positions: split it (the InDel allele keys hold 26 position bits)");
        GapWork &G = R.gap; memset(&G, 0, sizeof(G));
        G.n_ev = (int32_t)gap_slots; G.inc_cap = (int32_t)(7 * gap_slots + 8); G.seq_cap = ins_total + 8;
        const size_t ne = (size_t)std::max<int64_t>(gap_slots, 1), ni = (size_t)G.inc_cap;
        unsigned long long *k8; int32_t *c4;
        if ((rc = dev_alloc(r, ne, &G.ev)) || (rc = dev_alloc(r, 4 * ne + 4 * ni, &k8)) || (rc = dev_alloc(r, (size_t)4, &c4, true)) || (rc = dev_alloc(r, ne, &G.rows)) || (rc = dev_alloc(r, (size_t)G.seq_cap, &G.seq)) || (rc = dev_alloc(r, 2 * ne, &G.maj))) return rc;
        G.ckey = k8; G.ckey_s = k8 + ne; G.cval = k8 + 2 * ne; G.cval_s = k8 + 3 * ne;
        G.ikey = k8 + 4 * ne; G.ikey_s = G.ikey + ni; G.ival = G.ikey + 2 * ni; G.ival_s = G.ikey + 3 * ni;
        G.n_inc = c4; G.n_rows = c4 + 1; G.seq_len = (unsigned long long *)(c4 + 2);
        G.sort_tmp_bytes = uvc_gap_sort_tmp_bytes(std::max(ne, ni));
        uint8_t *tmp; if ((rc = dev_alloc(r, G.sort_tmp_bytes + 16, &tmp))) return rc; G.sort_tmp = tmp;
    }
    { int32_t *c; if ((rc = dev_alloc(r, (size_t)4, &c, true))) return rc; R.mis_cnt = c; R.mis_total = (unsigned long long *)(c + 2); R.mis = nullptr; R.mis_cap = 0; }
    r->d_dup_units = o.dup_units; r->d_dup_off = o.dup_off; r->n_dup = o.n_dup; r->n_dup_work = o.dup_work;
    R.max_frag_span = o.max_frag_span;
    R.any_amplicon = o.any_amplicon;
    R.max_frag_depth = o.max_frag_depth;   // k_frag packs two 16-bit bucket counters per LDS word when it is below 65 536
    // table rows are written by k_p2_slow<false>; mark all slots empty (0xFF)
    HIP_OK(hipMemsetAsync(R.table, 0, (size_t)std::max<int64_t>(o.table_rows, 1) * sizeof(Contrib), r->stream));   // no base, no LINK symbol
    {   // the work list of P1 and P2: stable order by (class, begin) on the device -- begin - region begin < 2^29 and the class takes the two
        // bits above -- in front of the prelude, which writes the record of a simple alignment straight into the slot of its entry
        const size_t np2 = (size_t)o.n_p2;
        for (int c = 0; c <= 4; c++) R.p2_off[c] = o.p2_off[c];
        uint32_t *work; uint8_t *tmp; int32_t *d_slot;
        const size_t tmp_bytes = uvc_sort32_tmp_bytes(std::max<size_t>(np2, 1));
        if ((rc = dev_alloc(r, 4 * np2, &work)) || (rc = dev_alloc(r, tmp_bytes + 16, &tmp)) || (rc = dev_alloc(r, (size_t)n, &d_slot))) return rc;
        for (int k = 0; k < 4; k++) if ((rc = dev_alloc(r, np2, &r->d_p2[k]))) return rc;
        if (uvc_sort_by_pos_cls(o.p2_beg, o.p2_cls, r->beg, pos_bits, 2, (int64_t)np2, work, tmp, tmp_bytes, r->stream) != 0) return fail(UVCGPU_EDEVICE, "device sort of the work list failed");
        uvc_launch_gather4(work + 3 * np2, (int64_t)np2, o.p2_aln, o.p2_beg, o.p2_end, o.p2_qb, r->d_p2[0], r->d_p2[1], r->d_p2[2], r->d_p2[3], W.kind, n, d_slot, r->stream);
        W.fast_rank = d_slot;
        { FastRec *f; if ((rc = dev_alloc(r, np2, &f))) return rc; R.frec2 = f; R.n_fast2 = (int32_t)np2; R.max_p2_span = o.max_p2_span; }
    }
    lap("allocations + orders");
    uvc_launch_prelude(&R, &W, &r->P, r->stream);
    lap("prelude kernel");
    uvc_launch_build_p2list(&R, W.fast_rank, r->d_p2[0], r->d_p2[1], r->d_p2[2], r->d_p2[3], r->stream);
    HIP_OK(hipGetLastError());
    {   // the queue of mismatching bases (k_p2_fast -> k_p2_mism) is sized from the count the prelude made
        unsigned long long total = 0; int32_t bad4 = 0;
        HIP_OK(hipMemcpyAsync(&total, R.mis_total, sizeof(total), hipMemcpyDeviceToHost, r->stream));
        if (d_bad) HIP_OK(hipMemcpyAsync(&bad4, d_bad, sizeof(bad4), hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipStreamSynchronize(r->stream));
        if (bad4 == 2) return fail(UVCGPU_EINVAL, "a base code outside 0..4 in UvcReadSoA::bases");
        if (bad4) return fail(UVCGPU_EINVAL, "bases4 / l_qseq / n_bases do not fit together");
        if (total > ((unsigned long long)1 << 30)) return fail(UVCGPU_EUNSUPPORTED, "more than 2^30 mismatching bases in one region");
        MisItem *q = nullptr;
        if ((rc = dev_alloc(r, (size_t)(total + 64), &q))) return rc;
        R.mis = q; R.mis_cap = (int32_t)(total + 64);
    }
    lap("work list build");
    r->n_bases = d->n_bases;
    r->has_reads = true; r->reads_given = true;
    return 0;
}

// Host columns: they are copied to the device as they are (no host pass over the reads), then prepared there.
static int uvcgpu_region_set_reads_impl(uvcgpu_region_t *r, const UvcReadSoA *in) {
    if (!r || !in) return fail(UVCGPU_EINVAL, "bad reads");
    if (stream_is_open(r)) return fail(UVCGPU_ESTATE, "set_reads while a score stream is open");
    if (in->struct_size != (int32_t)sizeof(UvcReadSoA)) return fail(UVCGPU_EINVAL, "UvcReadSoA::struct_size mismatch (set it to sizeof(UvcReadSoA))");
    if (in->n_reads < 0 || in->n_fams < 0) return fail(UVCGPU_EINVAL, "bad reads");
    const bool timing = (getenv("UVCGPU_TIMING") != nullptr);   // stderr breakdown of the ingest, for tuning
    auto t_prev = std::chrono::steady_clock::now();
    free_reads(r);
    struct SyncOnExit { hipStream_t s, s2; ~SyncOnExit() { hipStreamSynchronize(s); if (s2) hipStreamSynchronize(s2); } } sync_on_exit = { r->stream, r->side };   // no copy may outlive the caller's arrays, on any return path
    const int64_t n = in->n_reads;
    if (n == 0) { r->reads_given = true; return 0; }
    if (n > INT32_MAX / 2) return fail(UVCGPU_EUNSUPPORTED, "more than 2^30 reads in one region");
    if (in->n_bases < 0 || in->n_cigar_ops < 0) return fail(UVCGPU_EINVAL, "bad reads");
    UvcReadSoA d = *in;
    int rc;
    // The two large columns travel on the handle's main stream, the dozen small ones (8 MB each at 2 M reads; a copy costs ~0.13 ms of set-up
    // whatever its size) on a side stream beside them: their set-up times hide under the large transfers instead of adding up in front.
    hipStream_t small_stream = (r->side ? r->side : r->stream);
    auto up_on = [&](hipStream_t st, const void *src, size_t bytes, void **out) -> int {
        char *q = nullptr;
        int rc2 = dev_alloc(r, bytes, &q);
        if (rc2) return rc2;
        if (bytes && hipMemcpyAsync(q, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return fail(UVCGPU_EDEVICE, "hipMemcpyAsync(H2D)");
        *out = q;
        return 0;
    };
#define UP(field, T, count) { void *q; if ((rc = up_on(small_stream, in->field, sizeof(T) * (size_t)(count), &q))) return rc; d.field = (const T *)q; }
#define UPBIG(field, T, count) { void *q; if ((rc = up_on(r->stream, in->field, sizeof(T) * (size_t)(count), &q))) return rc; d.field = (const T *)q; }
    if (in->bases) UPBIG(bases, uint8_t, in->n_bases)
    else if (in->bases4) { if (in->n_bases4_bytes < 0) return fail(UVCGPU_EINVAL, "bad reads"); UPBIG(bases4, uint8_t, in->n_bases4_bytes) }
    UPBIG(quals, uint8_t, in->n_bases)
    UP(pos, int32_t, n) UP(mpos, int32_t, n) UP(isize, int32_t, n) UP(flag, uint16_t, n) UP(mapq, uint8_t, n) UP(nm, int32_t, n) UP(l_qseq, int32_t, n)
    UP(n_cigar, int32_t, n) UP(frag_id, int32_t, n) UP(fam_id, int32_t, n) UP(fam_strand, uint8_t, n)
    if (in->seq_off) UP(seq_off, int64_t, n)
    if (in->cigar_off) UP(cigar_off, int64_t, n)
    UP(cigars, uint32_t, in->n_cigar_ops) UP(fam_dflag, uint8_t, in->n_fams)
    if (small_stream != r->stream) {   // the preparation kernels read every column: the main stream waits for the side stream's copies
        if (hipEventRecord(r->e_fork2, small_stream) != hipSuccess || hipStreamWaitEvent(r->stream, r->e_fork2, 0) != hipSuccess) return fail(UVCGPU_EDEVICE, "hipEventRecord / hipStreamWaitEvent");
    }
#undef UPBIG
#undef UP
    if (timing) { hipStreamSynchronize(r->stream); const auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[uvcgpu set_reads] %-28s %8.2f ms\n", "H2D of the columns", std::chrono::duration<double, std::milli>(t - t_prev).count()); t_prev = t; }
    return set_reads_on_device(r, &d, timing, t_prev);
}

// The same with the columns already in HBM (every pointer of `in` is a device pointer on the handle's device): nothing is copied.  The
// arrays must stay valid and unchanged until the handle gets other reads, is reset or destroyed -- the kernels of every accumulate
// read bases / quals / cigars in place -- and uvcgpu_region_correct_bq edits `quals` in place, as the reference edits its bam1_t.
static int uvcgpu_region_set_reads_device_impl(uvcgpu_region_t *r, const UvcReadSoA *in) {
    if (!r || !in) return fail(UVCGPU_EINVAL, "bad reads");
    if (stream_is_open(r)) return fail(UVCGPU_ESTATE, "set_reads while a score stream is open");
    if (in->struct_size != (int32_t)sizeof(UvcReadSoA)) return fail(UVCGPU_EINVAL, "UvcReadSoA::struct_size mismatch (set it to sizeof(UvcReadSoA))");
    if (in->n_reads < 0 || in->n_fams < 0 || in->n_bases < 0 || in->n_cigar_ops < 0) return fail(UVCGPU_EINVAL, "bad reads");
    const bool timing = (getenv("UVCGPU_TIMING") != nullptr);
    free_reads(r);
    if (in->n_reads == 0) { r->reads_given = true; return 0; }
    if (in->n_reads > INT32_MAX / 2) return fail(UVCGPU_EUNSUPPORTED, "more than 2^30 reads in one region");
    return set_reads_on_device(r, in, timing, std::chrono::steady_clock::now());
}

// apply_bq_err_correction3 (grouping.cpp:459-543) on the resident reads, then everything derived from the base qualities again:
// the packed base|qual array and the per-read records (the low-quality-InDel test of k_aln_prelude reads them)
static int uvcgpu_region_correct_bq_impl(uvcgpu_region_t *r) {
    if (!r) return fail(UVCGPU_EINVAL, "null region");
    if (!r->has_reads) return fail(UVCGPU_ENOREADS, "no reads");
    uvc_launch_correct_bq(&r->R, r->P.assay_sequencing_BQ_max, r->P.assay_sequencing_BQ_inc, r->stream);
    uvc_launch_pack_bq(r->R.bases, r->R.quals, (uint16_t *)r->R.bq, r->n_bases, nullptr, r->stream);
    // A base whose value is 0 or less sends its fragment to the per-position kernels (FragRec::stat_kind 2, k_build_frags).  The penalties keep
    // a quality at 1 or above, so the correction makes a new quality of 0 only with a negative increment or a cap of 0 or less; where a negative
    // bq_phred_added_* puts the limit above 0, any lowered quality can cross it.  Then the fragments are looked at again.
    const int zthr = uvc_prep_zero_value_qual(&r->P);
    int32_t *d_n_joined = nullptr;   // device word: the fragments that join the sweep list
    if (zthr > 0 || (zthr == 0 && (r->P.assay_sequencing_BQ_inc < 0 || r->P.assay_sequencing_BQ_max <= 0))) {
        int rc = dev_alloc(r, 1, &d_n_joined, true);
        if (rc) return rc;
        uvc_prep_requalify(r->R.quals, r->W.seq_off, r->W.l_qseq, &r->P, r->R.n_frags, (FragRec *)r->R.frags, (int32_t *)r->R.sweep_frags, r->R.n_sweep, d_n_joined, r->stream);
    }
    HIP_OK(hipMemsetAsync(r->R.mis_total, 0, sizeof(unsigned long long), r->stream));
    uvc_launch_prelude(&r->R, &r->W, &r->P, r->stream);
    uvc_launch_build_p2list(&r->R, r->W.fast_rank, r->d_p2[0], r->d_p2[1], r->d_p2[2], r->d_p2[3], r->stream);
    HIP_OK(hipGetLastError());
    if (d_n_joined) {
        // (a blocking copy: it waits for the stream's work, and no copy into this stack slot is left running on any return path)
        HIP_OK(hipStreamSynchronize(r->stream));
        int32_t n_joined = 0;
        HIP_OK(hipMemcpy(&n_joined, d_n_joined, sizeof(n_joined), hipMemcpyDeviceToHost));
        if (getenv("UVCGPU_TIMING")) fprintf(stderr, "[uvcgpu correct_bq] fragments looked at again: %d joined the sweep list (%d)\n", n_joined, r->R.n_sweep + n_joined);
        r->R.n_sweep += n_joined;
    } else HIP_OK(hipStreamSynchronize(r->stream));
    r->accumulated = false;
    return 0;
}

// the base qualities as they are on the device (after uvcgpu_region_correct_bq, if it was called)
int uvcgpu_region_read_quals(uvcgpu_region_t *r, uint8_t *dst, int64_t n) {
    if (!r || !dst) return fail(UVCGPU_EINVAL, "null argument");
    if (!r->has_reads) return fail(UVCGPU_ENOREADS, "no reads");
    if (n != r->n_bases) return fail(UVCGPU_EINVAL, "n must equal UvcReadSoA::n_bases");
    HIP_OK(hipStreamSynchronize(r->stream));
    if (n > 0) HIP_OK(hipMemcpy(dst, r->R.quals, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// Zero fill of the plane slab (everything in front of the bucket planes, and the bucket planes too unless P3b / P5b left them clean) on
// stream `s`.  When the slab's contents were written under the present layout, only what every accumulate writes and what the last one marked
// (RegionDev::dirty) is filled; otherwise (first use, the handle was rebound to a region of another length) the whole slab.
static int zero_state(uvcgpu_region *r, hipStream_t s) {
    const bool selective = (r->dirty_npos == r->npos && !getenv("UVCGPU_FILL_ALL"));
    r->dirty_npos = 0;   // from here on the slab and the marks describe no layout until the caller's launch went through and restores it
    if (selective) {
        if (r->zero_planes_npos != r->npos) {   // the plane table of this layout (once per region length)
            ZeroPlane v[UVC_N_ZERO_PLANES];
            zero_plane_rows(r->L, r->npos, v);
            r->zero_planes_npos = 0;
            const hipError_t e = r->d_zero_planes.fit(UVC_N_ZERO_PLANES);
            if (e != hipSuccess) return fail(UVCGPU_EDEVICE, std::string("hipMalloc(zero-fill table): ") + hipGetErrorString(e));
            HIP_OK(hipMemcpy(r->d_zero_planes, v, sizeof(v), hipMemcpyHostToDevice));
            r->zero_planes_npos = r->npos;
        }
        uvc_launch_zero_state(r->d_state, r->d_zero_planes, UVC_N_ZERO_PLANES, r->d_dirty, r->R.ndblk, r->npos, s);
        if (hipGetLastError() != hipSuccess) return fail(UVCGPU_EDEVICE, "zero fill of the planes failed");
        if (!r->buckets_clean) HIP_OK(hipMemsetAsync(r->d_state + r->L.bucket_off, 0, r->L.total - r->L.bucket_off, s));
    } else {
        HIP_OK(hipMemsetAsync(r->d_state, 0, r->buckets_clean ? r->L.bucket_off : r->L.total, s));
    }
    HIP_OK(hipMemsetAsync(r->d_dirty, 0, uvc_link_buffer_bytes(dirty_bytes(r->R), r->R.nwin), s));   // the marks and link_need / link_done / link_cnt / link_list behind them
    r->link.planes_zeroed();
    return 0;
}

static int uvcgpu_region_accumulate_impl(uvcgpu_region_t *r) {
    if (!r) return fail(UVCGPU_EINVAL, "null region");
    if (stream_is_open(r)) return fail(UVCGPU_ESTATE, "accumulate while a score stream is open");
    if (!r->has_reads) return fail(UVCGPU_ENOREADS, "no reads");   // process_batch returns -1, main.cpp:520-523
    if (r->state_zeroed) { r->dirty_npos = 0; HIP_OK(hipStreamWaitEvent(r->stream, r->e_join, 0)); }   // zeroed behind the last score (release_state)
    else { const int rcz = zero_state(r, r->stream); if (rcz) return rcz; }
    r->state_zeroed = false; r->state_released = false;
    r->buckets_clean = false;
    HIP_OK(hipMemcpyAsync(r->d_rtr, r->d_rtr0, (size_t)4 * UVC_NRTR * r->npos, hipMemcpyDeviceToDevice, r->stream));   // P1b edits indelphred in place
    HIP_OK(hipMemsetAsync(r->R.frag_nmut, 0, sizeof(int32_t) * (size_t)r->R.n_frags, r->stream));
    HIP_OK(hipMemsetAsync(r->R.n_overflow, 0, sizeof(int32_t), r->stream));
    HIP_OK(hipMemsetAsync(r->R.mis_cnt, 0, sizeof(int32_t), r->stream));
    // the table is rebuilt by k_p2_slow<false>: MAX-merge needs empty slots
    if (r->R.n_complex) {
        // rows were set to 0xFF in set_reads and k_p2_slow<false> is idempotent under MAX, so no reset is needed
    }
    const int half = (int)std::round((10.0 / std::log(10.0)) * std::log(r->P.indel_del_to_ins_err_ratio)) / 2;   // main.hpp:1244
    const UvcAccStreams st = { r->stream, r->side, r->side3, r->e_fork, r->e_join, r->e_fork2, r->e_join3, r->e_stat, r->e_alleles, r->e_link_fork, r->e_link_join };
    // UVCGPU_LINK=eager (read on every accumulate, like UVCGPU_SPLIT): every window of LINK_M completed inside the accumulate, for comparison
    const char *lk_env = getenv("UVCGPU_LINK");
    const bool link_eager = (lk_env && !strcmp(lk_env, "eager")) || !uvc_acc_p2_plain(&r->R, &r->P);   // (the generic P2 forms make all of LINK_M in their LINK pass, as before 6-r8)
    r->link_split = uvc_acc_split_windows(&r->R);
    uvc_launch_accumulate(&r->R, &r->P, half, r->d_dup_units, r->n_dup, r->d_dup_off, r->n_dup_work, &st, link_eager ? 1 : 0, &r->prof);
    HIP_OK(hipGetLastError());
    r->link.accumulated(link_eager);
    if (getenv("UVCGPU_TIMING")) link_report(r, link_eager ? "all" : "indel");
    r->buckets_clean = (r->P.inferred_is_vcf_generated != 0);   // k_frag (P3b) and k_p5b cleared every bucket they consumed
    r->dirty_npos = r->npos;   // the slab and the marks now describe this layout
    r->accumulated = true; r->gap_ready = false; r->hap_ready = false;
    return 0;
}

int uvcgpu_region_check_presence(uvcgpu_region_t *r, int64_t *n_violations) {
    if (!r || !n_violations) return fail(UVCGPU_EINVAL, "bad argument");
    if (planes_guard(r, "check_presence")) return fail(UVCGPU_ESTATE, "check_presence needs the planes of an accumulate");
    Pool tmp(r);   // (waits for the streams, then frees, on every return path)
    unsigned long long *d = nullptr, h = 0;
    if (!tmp.get(&d, 1)) return fail(UVCGPU_EDEVICE, std::string("hipMalloc(violation count): ") + hipGetErrorString(tmp.last));
    int rc = 0;
    if (hipMemsetAsync(d, 0, 8, r->stream) != hipSuccess) rc = fail(UVCGPU_EDEVICE, "hipMemsetAsync");
    if (!rc) { uvc_launch_check_presence(&r->R, d, r->stream); uvc_launch_check_dirty(&r->R, d, r->stream); if (hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, r->stream) != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess) rc = fail(UVCGPU_EDEVICE, "check_presence"); }
    *n_violations = (int64_t)h;
    return rc;
}

// Per-kernel timing of the LAST accumulate, measured with HIP events on the handle's own stream.
// (the list of timed entries starts anew, as at an accumulate: a caller that times report calls alone need not accumulate between them)
int uvcgpu_region_set_profiling(uvcgpu_region_t *r, int on) { if (!r) return fail(UVCGPU_EINVAL, "null region"); r->prof.on = on ? 1 : 0; r->prof.n = 0; return 0; }
int uvcgpu_region_kernel_times(uvcgpu_region_t *r, char *names, int names_bytes, float *ms, int capacity) {
    if (!r || !names || !ms) return fail(UVCGPU_EINVAL, "bad argument");
    HIP_OK(hipStreamSynchronize(r->stream));
    std::string all;
    int n = 0;
    for (int i = 0; i < r->prof.n && n < capacity; i++, n++) {
        float t = 0;
        HIP_OK(hipEventElapsedTime(&t, r->prof.ev[i][0], r->prof.ev[i][1]));
        ms[n] = t; all += r->prof.name[i]; all += ";";
    }
    if ((int)all.size() + 1 > names_bytes) return fail(UVCGPU_EINVAL, "names buffer too small");
    memcpy(names, all.c_str(), all.size() + 1);
    return n;
}

// For tests only: the mismatch queue of the last accumulate as the device left it (the order of the items is the order of the atomics)
static_assert(sizeof(UvcMisItem) == sizeof(MisItem), "UvcMisItem is MisItem");
int uvcgpu_region_debug_mis_queue(uvcgpu_region_t *r, UvcMisItem *out, int64_t cap, int64_t *n, int64_t *total) {
    if (!r || !n || cap < 0 || (cap > 0 && !out)) return fail(UVCGPU_EINVAL, "bad argument");
    if (!r->has_reads || !r->accumulated) return fail(UVCGPU_ESTATE, "debug_mis_queue needs an accumulate");
    HIP_OK(hipStreamSynchronize(r->stream));
    if (r->side) HIP_OK(hipStreamSynchronize(r->side));
    if (r->side3) HIP_OK(hipStreamSynchronize(r->side3));
    int32_t cnt = 0; unsigned long long tot = 0;
    HIP_OK(hipMemcpy(&cnt, r->R.mis_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&tot, r->R.mis_total, sizeof(tot), hipMemcpyDeviceToHost));
    *n = cnt; if (total) *total = (int64_t)tot;
    const int64_t k = std::min<int64_t>(std::min<int64_t>(cnt, r->R.mis_cap), cap);
    if (k > 0) HIP_OK(hipMemcpy(out, r->R.mis, sizeof(MisItem) * (size_t)k, hipMemcpyDeviceToHost));
    return 0;
}

// how many records the last uvcgpu_region_score scored, and how many it returned (fewer with UvcScoreRequest::kept_only)
int uvcgpu_region_last_score_counts(const uvcgpu_region_t *r, int64_t *scored, int64_t *returned) {
    if (!r) return fail(UVCGPU_EINVAL, "null region");
    if (scored) *scored = r->last_scored;
    if (returned) *returned = r->last_returned;
    return 0;
}

int uvcgpu_region_sync(uvcgpu_region_t *r) {
    if (!r) return fail(UVCGPU_EINVAL, "null region");
    HIP_OK(hipStreamSynchronize(r->stream));
    int32_t e = 0;
    HIP_OK(hipMemcpy(&e, r->R.err, 4, hipMemcpyDeviceToHost));
    if (e) return fail(e, "a kernel flagged an unsupported read shape (a CIGAR op the reference itself throws on, process_cigar main_conversion.hpp:902-916)");
    return 0;
}

int64_t uvcgpu_region_field_bytes(const uvcgpu_region_t *r, int32_t g) {
    if (!r || g < 0 || g >= UVC_NUM_FIELD_GROUPS) return -1;
    if (uvc_group_in_slab(g) && !r->accumulated) return -1;
    return (int64_t)uvc_group_bytes(g, r->npos);
}

static int uvcgpu_region_fetch_impl(uvcgpu_region_t *r, int32_t g, void *dst, int64_t dst_bytes) {
    if (!r || !dst || g < 0 || g >= UVC_NUM_FIELD_GROUPS) return fail(UVCGPU_EINVAL, "bad argument");
    if (uvc_group_in_slab(g)) { const int rcg = planes_guard(r, "fetch"); if (rcg) return rcg; }
    if ((int64_t)uvc_group_bytes(g, r->npos) != dst_bytes) return fail(UVCGPU_EINVAL, "bad destination size");
    { const int rcl = link_complete(r, uvc_link_fetch_scope(g)); if (rcl) return rcl; }   // the groups with bias counters of LINK_M
    int rc = uvcgpu_region_sync(r);
    if (rc) return rc;
    const void *src = (g == UVC_F_RTR) ? (const void *)(r->accumulated ? r->d_rtr : r->d_rtr0) /* P1b's edit of indelphred exists after accumulate only */ : (g == UVC_F_BAQ) ? (const void *)r->d_baq : (const void *)(r->d_state + r->L.off[g]);
    HIP_OK(hipMemcpy(dst, src, (size_t)dst_bytes, hipMemcpyDeviceToHost));
    return 0;
}

// ---- columns of chosen positions (the read side of the record writer, uvc_vcf.cpp) ----
int32_t uvcgpu_region_column_base(int32_t g) { return (g < 0 || g >= UVC_NUM_FIELD_GROUPS) ? -1 : uvc_group_first_column(g); }
int32_t uvcgpu_region_n_columns(void) { return UVC_N_COLUMNS; }
static int uvcgpu_region_fetch_columns_impl(uvcgpu_region_t *r, const int32_t *refpos, int64_t n, int64_t *dst) {
    if (!r || n < 0 || (n > 0 && (!refpos || !dst))) return fail(UVCGPU_EINVAL, "bad argument");
    { const int rcg = planes_guard(r, "fetch"); if (rcg) return rcg; }
    if (n == 0) return 0;
    int rc = uvcgpu_region_sync(r);
    if (rc) return rc;
    const int32_t ncol = UVC_N_COLUMNS;
    const char *base[UVC_NUM_FIELD_GROUPS]; int32_t first[UVC_NUM_FIELD_GROUPS + 1], elem[UVC_NUM_FIELD_GROUPS];
    for (int g = 0; g <= UVC_NUM_FIELD_GROUPS; g++) first[g] = uvc_columns_before(g);
    for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) { elem[g] = uvc_group_elem(g); base[g] = r->d_state + r->L.off[g]; }   // (a group outside the slab has no columns)
    std::vector<int32_t> xs((size_t)n);
    for (int64_t i = 0; i < n; i++) xs[(size_t)i] = refpos[i] - r->beg;   // out of range -> a row of zeros (checked in the kernel)
    Pool tmp(r);   // (waits for the streams, then frees, on every return path: a launched kernel may still write the blocks when a later step fails)
    int32_t *d_xs = nullptr; long long *d_out = nullptr;
    if (!tmp.get(&d_xs, (size_t)n)) return fail(UVCGPU_ENOMEM, "hipMalloc(column positions) failed");
    if (!tmp.get(&d_out, (size_t)n * ncol)) return fail(UVCGPU_ENOMEM, "hipMalloc(columns) failed");
    hipError_t e = hipMemcpyAsync(d_xs, xs.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) { const int rcl = link_complete(r, uvc_link_columns_scope(), d_xs, n); if (rcl) return rcl; }   // a row holds the bias counters of LINK_M at its position
    if (e == hipSuccess) { uvc_launch_gather_columns(base, first, elem, r->npos, d_xs, n, d_out, r->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d_out, sizeof(long long) * (size_t)n * ncol, hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return fail(UVCGPU_EDEVICE, hipGetErrorString(e));
    return 0;
}
// position-level numbers for the MGVCF block and ADDITIONAL_INDEL_CANDIDATE lines of the record writer: 10 ints per position of
// [refpos_beg, refpos_end), see k_block_stats
int uvcgpu_region_block_stats_(uvcgpu_region_t *r, int32_t refpos_beg, int32_t refpos_end, int32_t *dst) {
    if (!r || !dst || refpos_end < refpos_beg) return fail(UVCGPU_EINVAL, "bad argument");
    { const int rcg = planes_guard(r, "fetch"); if (rcg) return rcg; }
    const int64_t n = (int64_t)refpos_end - refpos_beg;
    if (n == 0) return 0;
    int rc = uvcgpu_region_sync(r);
    if (rc) return rc;
    Pool tmp(r);   // (waits for the streams, then frees, on every return path)
    int32_t *d = nullptr;
    if (!tmp.get(&d, 10 * (size_t)n)) return fail(UVCGPU_ENOMEM, "hipMalloc(block stats) failed");
    uvc_launch_block_stats(&r->R, &r->P, (int64_t)refpos_beg - r->beg, n, d, r->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d, sizeof(int32_t) * 10 * (size_t)n, hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    if (e != hipSuccess) return fail(UVCGPU_EDEVICE, hipGetErrorString(e));
    return 0;
}
// The same for n_win disjoint windows [win[2k], win[2k + 1]) of refpos in one round trip: one upload of the window table, one launch, one D2H.
// dst receives the windows' rows back to back.
int uvcgpu_region_block_stats_windows_(uvcgpu_region_t *r, const int32_t *win, int64_t n_win, int32_t *dst) {
    if (!r || !win || !dst || n_win < 0 || n_win > INT32_MAX) return fail(UVCGPU_EINVAL, "bad argument");
    { const int rcg = planes_guard(r, "fetch"); if (rcg) return rcg; }
    std::vector<long long> tab((size_t)(2 * n_win));
    int64_t n = 0;
    for (int64_t k = 0; k < n_win; k++) {
        if (win[2 * k + 1] <= win[2 * k]) return fail(UVCGPU_EINVAL, "block statistics: empty window");
        tab[(size_t)(2 * k)] = (long long)win[2 * k] - r->beg; tab[(size_t)(2 * k + 1)] = n; n += (int64_t)win[2 * k + 1] - win[2 * k];
    }
    if (n == 0) return 0;
    int rc = uvcgpu_region_sync(r);
    if (rc) return rc;
    Pool tmp(r);   // declared behind `tab`: it waits for the streams before `tab` goes, on every return path, and then frees the two blocks
    long long *d_tab = nullptr; int32_t *d = nullptr;
    if (!tmp.get(&d_tab, tab.size()) || !tmp.get(&d, 10 * (size_t)n)) return fail(UVCGPU_ENOMEM, "hipMalloc(block stats) failed");
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), sizeof(long long) * tab.size(), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) { uvc_launch_block_stats_windows(&r->R, &r->P, d_tab, (int)n_win, n, d, r->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d, sizeof(int32_t) * 10 * (size_t)n, hipMemcpyDeviceToHost, r->stream);
    const hipError_t e2 = hipStreamSynchronize(r->stream);
    if (e != hipSuccess || e2 != hipSuccess) return fail(UVCGPU_EDEVICE, hipGetErrorString(e != hipSuccess ? e : e2));
    return 0;
}
// Page-locks a caller buffer (the records buffer of uvcgpu_region_score, the read arrays of uvcgpu_region_set_reads) so that copies to
// and from it run at PCIe speed instead of through the runtime's staging buffers.  Optional; the buffer must be unpinned before it is freed.
int uvcgpu_pin_host_buffer(void *p, int64_t bytes) {
    if (!p || bytes <= 0) return fail(UVCGPU_EINVAL, "bad argument");
    hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(UVCGPU_EDEVICE, std::string("hipHostRegister: ") + hipGetErrorString(e)); }
    return 0;
}
int uvcgpu_host_alloc(void **p, int64_t bytes) {
    if (!p || bytes <= 0) return fail(UVCGPU_EINVAL, "bad argument");
    *p = nullptr;
    hipError_t e = Buf<char, true>::raw_alloc(p, (size_t)bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return fail(UVCGPU_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    return 0;
}
int uvcgpu_host_free(void *p) {
    if (!p) return 0;
    hipError_t e = Buf<char, true>::raw_free(p);
    if (e != hipSuccess) { (void)hipGetLastError(); if (getenv("UVCGPU_DEBUG")) fprintf(stderr, "[uvcgpu] hipHostFree: %s\n", hipGetErrorString(e)); return fail(UVCGPU_EDEVICE, std::string("hipHostFree: ") + hipGetErrorString(e)); }
    return 0;
}
int uvcgpu_unpin_host_buffer(void *p) {
    if (!p) return 0;
    hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(UVCGPU_EDEVICE, std::string("hipHostUnregister: ") + hipGetErrorString(e)); }
    return 0;
}

// what uvc_vcf.cpp reads of a handle besides the public calls
const char *uvcgpu_region_refseq(const uvcgpu_region_t *r, int32_t *beg, int32_t *end) { if (beg) *beg = r->beg; if (end) *end = r->end - 1; return r->refstring.c_str(); }
// begpos / tracklen / unitlen of every position as refstring2repeatvec built them (the first three planes of UVC_F_RTR before P1b): the
// record writer's INFO/R3X2.  Fetched from the device on first use after a (re)bind; NULL when the copy fails.
const int32_t *uvcgpu_region_repeat_tracks(const uvcgpu_region_t *cr, int64_t *npos) {
    uvcgpu_region_t *r = const_cast<uvcgpu_region_t *>(cr);
    if (npos) *npos = r->npos;
    if (!r->h_rtr_valid) {
        r->h_rtr.resize((size_t)3 * r->npos);
        // on the handle's own stream: a null-stream copy would also wait for every other handle's work
        if (hipMemcpyAsync(r->h_rtr.data(), r->d_rtr0, sizeof(int32_t) * r->h_rtr.size(), hipMemcpyDeviceToHost, r->stream) != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        r->h_rtr_valid = true;
    }
    return r->h_rtr.data();
}
const UvcParams *uvcgpu_region_params(const uvcgpu_region_t *r) { return &r->P; }

// ---- InDel allele tables: the host half of fill_by_indel_info / indel_get_majority (instcode.hpp, main.hpp:5350-5455) ----
// The device reduces the allele-keyed counters to one GapRow per (position, symbol, allele) (k_gap_rows); what is left is per InDel
// site: splitting by strand, the reference's two sorts, and the quarter-of-the-best filter.
namespace {
struct GapAl { int32_t len; const uint8_t *seq; bool del; };   // allele text: inserted bases (codes 0..4) or a deleted length
inline int text_rank(int b) { return b == 4 ? 3 : (b == 3 ? 4 : b); }   // "ACGTN": A < C < G < N < T
int gap_al_cmp(const GapAl &a, const GapAl &b) {   // std::string order of the reference's keys
    if (a.del) return (a.len > b.len) - (a.len < b.len);   // prefixes of the same reference text
    const int n = std::min(a.len, b.len);
    for (int i = 0; i < n; i++) { const int ra = text_rank(a.seq[i]), rb = text_rank(b.seq[i]); if (ra != rb) return ra < rb ? -1 : 1; }
    return (a.len > b.len) - (a.len < b.len);
}
}
static int gap_tables(uvcgpu_region_t *r) {
    if (r->gap_ready) return 0;
    // The allele pipeline runs on the side stream and ends long before the main stream does (uvc_launch_accumulate): wait for it alone,
    // so that this host step and the launches of the scoring kernels behind it stay hidden under the fragment / family kernels.
    hipStream_t cs = (r->side ? r->side : r->stream);
    if (r->side) HIP_OK(hipEventSynchronize(r->e_fork2)); else HIP_OK(hipStreamSynchronize(r->stream));
    r->gap_rows.clear(); r->gap_seq.clear(); r->gap_alleles.clear(); r->gap_allele_row.clear();
    const GapWork &G = r->R.gap;
    int32_t cnt[4] = { 0, 0, 0, 0 };
    if (G.n_inc) { HIP_OK(hipMemcpyAsync(cnt, G.n_inc, 16, hipMemcpyDeviceToHost, cs)); HIP_OK(hipStreamSynchronize(cs)); }
    const int32_t n_rows = cnt[1];
    unsigned long long seq_len = 0; memcpy(&seq_len, &cnt[2], 8);
    if (n_rows < 0 || n_rows > G.n_ev || seq_len > (unsigned long long)G.seq_cap) return fail(UVCGPU_EDEVICE, "allele table overflow");   // before anything is sized from them
    std::vector<GapRow> dev((size_t)n_rows);
    std::vector<uint8_t> dseq((size_t)seq_len);
    if (n_rows) HIP_OK(hipMemcpyAsync(dev.data(), G.rows, sizeof(GapRow) * (size_t)n_rows, hipMemcpyDeviceToHost, cs));
    if (seq_len) HIP_OK(hipMemcpyAsync(dseq.data(), G.seq, (size_t)seq_len, hipMemcpyDeviceToHost, cs));
    if (n_rows || seq_len) HIP_OK(hipStreamSynchronize(cs));
    auto al_of = [&](const GapRow &g) { GapAl a; a.len = g.len; a.del = (g.seq_off < 0); a.seq = (a.del ? nullptr : dseq.data() + g.seq_off); return a; };
    std::sort(dev.begin(), dev.end(), [&](const GapRow &a, const GapRow &b) {
        if (a.x != b.x) return a.x < b.x;
        if (a.sym != b.sym) return a.sym < b.sym;
        return gap_al_cmp(al_of(a), al_of(b)) < 0; });   // ascending allele text: the iteration order of the reference's maps
    struct Tup { int32_t fq, bq, c2, c2d; const GapRow *g; };
    for (size_t g0 = 0; g0 < dev.size();) {
        size_t g1 = g0;
        while (g1 < dev.size() && dev[g1].x == dev[g0].x && dev[g1].sym == dev[g0].sym) g1++;
        const int32_t refpos = r->beg + dev[g0].x, symbol = dev[g0].sym;
        const size_t first_row = r->gap_rows.size();
        std::vector<const GapRow *> row_allele;   // parallel to the rows pushed for this site
        for (int strand = 0; strand < 2; strand++) {   // fill_by_indel_info2_{1,2}: the strand's tuples, sorted descending (instcode.hpp:44-62)
            std::vector<Tup> t;
            for (size_t g = g0; g < g1; g++) if (dev[g].cnt[strand * 4] > 0) t.push_back(Tup{ dev[g].cnt[strand * 4 + 1], dev[g].cnt[strand * 4], dev[g].cnt[strand * 4 + 2], dev[g].cnt[strand * 4 + 3], &dev[g] });
            std::sort(t.begin(), t.end(), [&](const Tup &a, const Tup &b) {
                if (a.fq != b.fq) return a.fq > b.fq;
                if (a.bq != b.bq) return a.bq > b.bq;
                if (a.c2 != b.c2) return a.c2 > b.c2;
                if (a.c2d != b.c2d) return a.c2d > b.c2d;
                return gap_al_cmp(al_of(*a.g), al_of(*b.g)) > 0; });
            for (const Tup &u : t) {
                UvcGapRow o; memset(&o, 0, sizeof(o));
                o.refpos = refpos; o.symbol = symbol; o.strand = strand; o.len = u.g->len; o.seq_off = -1;
                if (u.g->seq_off >= 0) { o.seq_off = (int64_t)r->gap_seq.size(); r->gap_seq.insert(r->gap_seq.end(), dseq.begin() + u.g->seq_off, dseq.begin() + u.g->seq_off + u.g->len); }
                o.bAD1 = u.bq; o.cAD1 = u.fq; o.c2AD = u.c2; o.c2dAD = u.c2d;
                r->gap_rows.push_back(o); row_allele.push_back(u.g);
            }
        }
        // indel_get_majority (main.hpp:5406-5455): merge the strands per allele, keep those with at least a quarter of the best fragment
        // support, order by descending bAD1^2 * length (ties: ascending text -- what the reference's std::sort over
        // reverse iterators leaves for the short vectors that occur)
        struct Maj { int32_t b, c; const GapRow *g; };
        std::vector<Maj> m;
        int32_t max_b = 0;
        for (size_t g = g0; g < g1; g++) {
            Maj a = { 0, 0, &dev[g] };
            for (int strand = 0; strand < 2; strand++) if (dev[g].cnt[strand * 4] > 0) { a.b += dev[g].cnt[strand * 4]; a.c += dev[g].cnt[strand * 4 + 1]; }
            if (a.b > 0) { m.push_back(a); max_b = std::max(max_b, a.b); }
        }
        std::vector<Maj> kept;
        for (const Maj &a : m) if (a.b >= (max_b + 3) / 4) kept.push_back(a);
        std::stable_sort(kept.begin(), kept.end(), [](const Maj &a, const Maj &b) { return (int64_t)a.b * a.b * (int64_t)a.g->len > (int64_t)b.b * b.b * (int64_t)b.g->len; });
        for (const Maj &a : kept) {
            r->gap_alleles.push_back(UvcIndelAllele{ refpos, symbol, a.b, a.c, a.g->len });
            int32_t row = -1;
            for (size_t q = 0; q < row_allele.size() && row < 0; q++) if (row_allele[q] == a.g) row = (int32_t)(first_row + q);
            r->gap_allele_row.push_back(row);
        }
        g0 = g1;
    }
    const int64_t na = (int64_t)r->gap_alleles.size();
    const int64_t nr = (int64_t)r->gap_rows.size(), ns = (int64_t)r->gap_seq.size();
    // (64 elements of slack each; the alleles and their rows grow together)
    for (const hipError_t e : { r->d_gap_alleles.fit((size_t)na, 64), r->d_gap_allele_row.fit((size_t)na, 64), r->d_gap_rows.fit((size_t)nr, 64), r->d_gap_seq.fit((size_t)ns, 64) })
        if (e != hipSuccess) return fail(UVCGPU_EDEVICE, std::string("hipMalloc(InDel allele tables): ") + hipGetErrorString(e));
    if (nr) HIP_OK(hipMemcpyAsync(r->d_gap_rows, r->gap_rows.data(), sizeof(UvcGapRow) * (size_t)nr, hipMemcpyHostToDevice, cs));
    if (ns) HIP_OK(hipMemcpyAsync(r->d_gap_seq, r->gap_seq.data(), (size_t)ns, hipMemcpyHostToDevice, cs));
    if (nr || ns) HIP_OK(hipStreamSynchronize(cs));
    if (na) {
        HIP_OK(hipMemcpyAsync(r->d_gap_alleles, r->gap_alleles.data(), sizeof(UvcIndelAllele) * (size_t)na, hipMemcpyHostToDevice, cs));
        HIP_OK(hipMemcpyAsync(r->d_gap_allele_row, r->gap_allele_row.data(), sizeof(int32_t) * (size_t)na, hipMemcpyHostToDevice, cs));
        HIP_OK(hipStreamSynchronize(cs));
    }
    r->gap_ready = true;
    return 0;
}

static int uvcgpu_region_indel_alleles_impl(uvcgpu_region_t *r, UvcGapRow *rows, int64_t row_capacity, int64_t *n_rows, uint8_t *seq, int64_t seq_capacity, int64_t *seq_bytes) {
    if (!r) return fail(UVCGPU_EINVAL, "null region");
    if (!r->accumulated) return fail(UVCGPU_ESTATE, "indel_alleles before accumulate");
    int rc = gap_tables(r);
    if (rc) return rc;
    if (n_rows) *n_rows = (int64_t)r->gap_rows.size();
    if (seq_bytes) *seq_bytes = (int64_t)r->gap_seq.size();
    if ((int64_t)r->gap_rows.size() > row_capacity || (int64_t)r->gap_seq.size() > seq_capacity) return fail(UVCGPU_ENOMEM, "allele table capacity too small");
    if (!r->gap_rows.empty()) memcpy(rows, r->gap_rows.data(), r->gap_rows.size() * sizeof(UvcGapRow));
    if (!r->gap_seq.empty()) memcpy(seq, r->gap_seq.data(), r->gap_seq.size());
    return 0;
}

// ---- haplotype links: hap_bq / hap_fq / hap_f2q of updateByRegion3Aln (main.hpp:3665-3742) ----
// Built on request (the record writer and uvcgpu_region_hap_links ask): candidate fragments / units -> their mutated (position, symbol)
// lists on the device (k_hap_*), maps + updateHapMap on the host (uvc_hap.cpp).  Needs the planes (P5's cDPM / cDPm).
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int hap_tables(uvcgpu_region_t *r) {
    if (r->hap_ready) return 0;
    { const int rcg = planes_guard(r, "haplotype links"); if (rcg) return rcg; }
    const RegionDev &R = r->R;
    std::vector<int32_t> events;
    const bool timing = (getenv("UVCGPU_TIMING") != nullptr);
    double t_prev = now_s();
    auto lap = [&](const char *what, long long n) { if (timing) { const double t = now_s(); fprintf(stderr, "[uvcgpu hap_links] %-34s %8.2f ms (%lld)\n", what, 1e3 * (t - t_prev), n); t_prev = t; } };
    Pool tmp(r);   // (waits for the streams, then frees, on every return path)
    auto get = [&](size_t bytes) { return tmp.get(std::max<size_t>(bytes, 8)); };
    for (int units = 0; units < 2; units++) {
        // the fragment links come from P3 (updateByAlns3UsingBQ, main.hpp:3691), the family links from P5, which updateByAlns3UsingFQ runs
        // only for a VCF run as well (main.hpp:3371-3521): a FASTQ-only run has no links
        if (!r->P.inferred_is_vcf_generated) continue;
        const size_t n = (size_t)(units ? R.n_fs : R.n_frags);
        if (n == 0) continue;
        HapWork H; memset(&H, 0, sizeof(H));
        H.cand = (int32_t *)get(4 * n); H.cand_off = (int32_t *)get(4 * n); H.cand_cap = (int32_t *)get(4 * n);
        char *ctr = (char *)get(16);
        if (!H.cand || !H.cand_off || !H.cand_cap || !ctr) return fail(UVCGPU_ENOMEM, "hipMalloc(haplotype candidates)");
        H.n_cand = (int32_t *)ctr; H.total = (unsigned long long *)(ctr + 8);
        HIP_OK(hipMemsetAsync(ctr, 0, 16, r->stream));
        uvc_launch_hap_cand(&R, &H, units, r->stream);
        struct { int32_t n_cand, pad; unsigned long long total; } c;
        HIP_OK(hipMemcpyAsync(&c, ctr, 16, hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipStreamSynchronize(r->stream));
        lap(units ? "candidates of units" : "candidates of fragments", (long long)c.n_cand);
        if (c.n_cand == 0) continue;
        if (c.total >= ((unsigned long long)1 << 31)) return fail(UVCGPU_EUNSUPPORTED, "more than 2^31 haplotype event slots in one region");
        H.events = (int32_t *)get(4 * (size_t)c.total);
        if (!H.events) return fail(UVCGPU_ENOMEM, "hipMalloc(haplotype events)");
        HIP_OK(hipMemsetAsync(H.events, 0xFF, 4 * (size_t)c.total, r->stream));
        uvc_launch_hap_events(&R, &r->P, &H, units, c.n_cand, r->stream);
        HIP_OK(hipGetLastError());
        const size_t at = events.size();
        events.resize(at + (size_t)c.total);
        HIP_OK(hipMemcpyAsync(events.data() + at, H.events, 4 * (size_t)c.total, hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipStreamSynchronize(r->stream));
        lap(units ? "events of units + D2H" : "events of fragments + D2H", (long long)c.total);
    }
    { const int rc = uvcgpu_region_sync(r); if (rc) return rc; }
    uvc_hap_build(events.data(), (int64_t)events.size(), r->beg, r->npos, r->P.phasing_haplotype_max_count, r->P.phasing_haplotype_min_ad, r->P.phasing_haplotype_max_detail_cnt, r->hap);
    lap("maps + links (host)", (long long)(r->hap[0].size() + r->hap[1].size() + r->hap[2].size()));
    r->hap_ready = true;
    return 0;
}
const std::vector<UvcHapLinkHost> *uvcgpu_region_hap_(uvcgpu_region_t *r) { return hap_tables(r) ? nullptr : r->hap; }   // for uvc_vcf.cpp

static int uvcgpu_region_hap_links_impl(uvcgpu_region_t *r, UvcHapLink *links, int64_t link_capacity, int64_t *n_links, int32_t *muts, int64_t mut_capacity, int64_t *n_mut_ints) {
    if (!r) return fail(UVCGPU_EINVAL, "null region");
    int rc = hap_tables(r);
    if (rc) return rc;
    int64_t nl = 0, nm = 0;
    for (int w = 0; w < 3; w++) for (const UvcHapLinkHost &h : r->hap[w]) { nl++; nm += 2 * (int64_t)h.form.size(); }
    if (n_links) *n_links = nl;
    if (n_mut_ints) *n_mut_ints = nm;
    if (nl > link_capacity || nm > mut_capacity || (nl && !links) || (nm && !muts)) return fail(UVCGPU_ENOMEM, "haplotype link capacity too small");
    int64_t li = 0, mi = 0;
    for (int w = 0; w < 3; w++) for (const UvcHapLinkHost &h : r->hap[w]) {
        UvcHapLink &o = links[li++];
        o.which = w; o.n_muts = (int32_t)h.form.size(); o.mut_off = mi; o.fr_cnt[0] = h.fr[0]; o.fr_cnt[1] = h.fr[1]; o.other_cnt[0] = h.other[0]; o.other_cnt[1] = h.other[1];
        for (const auto &ps : h.form) { muts[mi++] = ps.first; muts[mi++] = ps.second; }
    }
    return 0;
}

int64_t uvcgpu_region_score_size(const uvcgpu_region_t *r, const UvcScoreRequest *req) {
    if (!r) return -1;
    const int64_t np = (req && req->pos_beg >= 0) ? (req->pos_end - req->pos_beg) : r->npos;
    return NSYM * (np + 1) + (req ? req->n_indel_alleles + req->n_tumor_keys + 16 * std::max<int64_t>(req->n_force_sites, 0) : 0) + (int64_t)r->gap_alleles.size();
}
int64_t uvcgpu_region_score_ranges_size(const uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges) {
    if (!r || !ranges || n_ranges < 0) return -1;
    int64_t np = 0;
    for (int64_t k = 0; k < n_ranges; k++) np += std::max<int64_t>((int64_t)ranges[k].pos_end - ranges[k].pos_beg, 0);
    return NSYM * (np + 1) + (req ? req->n_indel_alleles + req->n_tumor_keys + 16 * std::max<int64_t>(req->n_force_sites, 0) : 0) + (int64_t)r->gap_alleles.size();
}

// Small host arrays of a score call go to the device through the handle's own page-locked staging buffer: an asynchronous copy straight from
// the caller's pageable memory lets the runtime map those heap pages for the GPU (read-only, as a copy source), and heap pages come back to the
// caller in other roles -- as a records buffer the next copy writes to.  `at` advances through the staging buffer within one call.
static int stage_upload(uvcgpu_region_t *r, void *dst, const void *src, size_t bytes, size_t &at, size_t total) {
    if (r->h_stage.fit(total, total / 2 + 4096) != hipSuccess) return fail(UVCGPU_ENOMEM, "hipHostMalloc(staging)");
    memcpy(r->h_stage + at, src, bytes);
    if (hipMemcpyAsync(dst, r->h_stage + at, bytes, hipMemcpyHostToDevice, r->stream) != hipSuccess) return fail(UVCGPU_EDEVICE, "hipMemcpyAsync(staging)");
    at += (bytes + 63) & ~(size_t)63;
    return 0;
}

// `ranges` (uvcgpu_region_score_ranges) or NULL (uvcgpu_region_score): everything but the group axis is the same call
// What a score request becomes before any scoring kernel runs -- the checked request, the ranges' device table, the caller's alleles merged
// with the region's, tumor keys, force-output sites, all uploaded through the staging buffer -- for the one call and for a stream alike.
// The temporaries (the merged alleles and their rows, the tumor keys, the force-output sites, the ranges) live in a pool of the call, which
// drains the handle's streams (async copies, kernels that read the blocks) before it frees them.
struct ScorePrep {
    UvcScoreRequest rq; std::vector<UvcScoreRangeDev> rtab; int64_t npos_scored = 0;
    std::unique_ptr<Pool> tmp;
    UvcScoreIn in = {};   // what the score launchers take: views of the above and of the handle (scratch: set where the scratch is allocated)
};
static int score_prepare(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, ScorePrep &p) {
    { const int rcg = planes_guard(r, "score"); if (rcg) return rcg; }
    if (stream_is_open(r)) return fail(UVCGPU_ESTATE, "a score stream is open on this handle (uvcgpu_score_stream_end closes it)");
    p.tmp.reset(new Pool(r));
    UvcScoreRequest &rq = p.rq; memset(&rq, 0, sizeof(rq)); rq.pos_beg = -1;
    if (req) rq = *req;
    std::vector<UvcScoreRangeDev> &rtab = p.rtab;   // ranges call: the device table; npos_scored = the compact length
    int64_t &npos_scored = p.npos_scored;
    if (ranges) {
        if (n_ranges < 1 || n_ranges > INT32_MAX) return fail(UVCGPU_EINVAL, "score_ranges: n_ranges must be at least 1");
        if (rq.pos_beg != -1 || rq.base_at_pos_beg != 0 || rq.region_beg != 0) return fail(UVCGPU_EINVAL, "score_ranges: the request's pos_beg must be -1, its base_at_pos_beg and region_beg 0 (the ranges carry them)");
        rtab.resize((size_t)n_ranges);
        for (int64_t k = 0; k < n_ranges; k++) {
            const UvcScoreRange &q = ranges[k];
            if (q.pos_beg < r->beg + (q.base_at_pos_beg ? 1 : 0) || q.pos_end > r->end - 1 || q.pos_end < q.pos_beg)   // the bounds rule of the plain call, below
                return fail(UVCGPU_EINVAL, "score_ranges: range " + std::to_string(k) + " [" + std::to_string(q.pos_beg) + ", " + std::to_string(q.pos_end) + ") is outside the region");
            if (k > 0 && q.pos_beg < ranges[k - 1].pos_end)
                return fail(UVCGPU_EINVAL, "score_ranges: range " + std::to_string(k) + " begins at " + std::to_string(q.pos_beg) + ", in front of the end " + std::to_string(ranges[k - 1].pos_end) + " of range " + std::to_string(k - 1) + " (ranges must be sorted and disjoint)");
            rtab[(size_t)k] = UvcScoreRangeDev{ q.pos_beg, q.pos_end, (int32_t)npos_scored, q.base_at_pos_beg ? 1 : 0 };
            npos_scored += (int64_t)q.pos_end - q.pos_beg;
        }
        rq.pos_beg = ranges[0].pos_beg; rq.pos_end = ranges[n_ranges - 1].pos_end;   // (the kernels take the table; these only keep the request well-formed)
    } else {
        if (rq.pos_beg < 0) { rq.pos_beg = r->beg + 1; rq.pos_end = r->end - 1; }
        // zerobased_pos == region begin is legal (a contig that starts inside the region: main.cpp:617-619 guards its "base in front" with BASE_NN);
        // with base_at_pos_beg the BASE sub-position of pos_beg reads refpos pos_beg - 1, which must be inside the region
        if (rq.pos_beg < r->beg + (rq.base_at_pos_beg ? 1 : 0) || rq.pos_end > r->end - 1 || rq.pos_end < rq.pos_beg) return fail(UVCGPU_EINVAL, "score range outside the region");
        npos_scored = (int64_t)rq.pos_end - rq.pos_beg;
    }
    // InDel alleles: the region's own tables (fill_by_indel_info / indel_get_majority); a (refpos, symbol) the caller lists is overridden
    { int rc0 = gap_tables(r); if (rc0) return rc0; }
    UvcIndelAllele *d_al = nullptr; int32_t *d_al_row = nullptr; UvcTumorKey *d_tk = nullptr; int32_t *d_fs = nullptr; UvcScoreRangeDev *d_rg = nullptr;
    auto no_room = [&] { return fail(UVCGPU_EDEVICE, std::string("hipMalloc(score request): ") + hipGetErrorString(p.tmp->last)); };
    std::vector<UvcIndelAllele> merged; std::vector<int32_t> merged_row;
    const UvcIndelAllele *use_al = r->d_gap_alleles; const int32_t *use_row = r->d_gap_allele_row; int64_t n_al = (int64_t)r->gap_alleles.size();
    // one staging layout per call (an earlier call's copies are complete: score synchronises before it returns)
    size_t stage_at = 0;
    const size_t stage_total = (sizeof(UvcIndelAllele) + sizeof(int32_t)) * (size_t)(r->gap_alleles.size() + (size_t)std::max<int64_t>(rq.n_indel_alleles, 0)) + sizeof(UvcTumorKey) * (size_t)std::max<int64_t>(rq.n_tumor_keys, 0)
                              + sizeof(int32_t) * (size_t)std::max<int64_t>(rq.n_force_sites, 0) + sizeof(UvcScoreRangeDev) * rtab.size() + 320;
    if (rq.n_indel_alleles > 0) {
        auto less = [](const UvcIndelAllele &a, const UvcIndelAllele &b) { return a.refpos < b.refpos || (a.refpos == b.refpos && a.symbol < b.symbol); };
        for (int64_t q = 1; q < rq.n_indel_alleles; q++) if (less(rq.indel_alleles[q], rq.indel_alleles[q - 1])) return fail(UVCGPU_EINVAL, "indel_alleles must be sorted by (refpos, symbol)");
        size_t i = 0; int64_t j = 0;
        while (i < r->gap_alleles.size() || j < rq.n_indel_alleles) {
            const bool take_own = (j >= rq.n_indel_alleles) || (i < r->gap_alleles.size() && less(r->gap_alleles[i], rq.indel_alleles[j]));
            if (take_own) { merged.push_back(r->gap_alleles[i]); merged_row.push_back(r->gap_allele_row[i]); i++; continue; }
            const UvcIndelAllele key = rq.indel_alleles[j];
            while (i < r->gap_alleles.size() && !less(key, r->gap_alleles[i])) i++;   // drop the library's alleles of this (refpos, symbol)
            while (j < rq.n_indel_alleles && !less(key, rq.indel_alleles[j])) { merged.push_back(rq.indel_alleles[j]); merged_row.push_back(-1); j++; }
        }
        n_al = (int64_t)merged.size();
        if (!p.tmp->get(&d_al, (size_t)n_al) || !p.tmp->get(&d_al_row, (size_t)n_al)) return no_room();
        { int rc1 = stage_upload(r, d_al, merged.data(), sizeof(UvcIndelAllele) * (size_t)n_al, stage_at, stage_total); if (rc1) return rc1; }
        { int rc1 = stage_upload(r, d_al_row, merged_row.data(), sizeof(int32_t) * (size_t)n_al, stage_at, stage_total); if (rc1) return rc1; }
        use_al = d_al; use_row = d_al_row;
    }
    if (r->P.tumor_vcf_is_provided && rq.n_tumor_keys > 0) {   // normal sample of a T/N pair: the tumor records, sorted by (refpos, symbol)
        for (int64_t q = 1; q < rq.n_tumor_keys; q++) {
            const UvcTumorKey &a = rq.tumor_keys[q - 1], &b = rq.tumor_keys[q];
            if (a.refpos > b.refpos || (a.refpos == b.refpos && a.symbol > b.symbol)) return fail(UVCGPU_EINVAL, "tumor_keys must be sorted by (refpos, symbol)");
        }
        if (!p.tmp->get(&d_tk, (size_t)rq.n_tumor_keys)) return no_room();
        { int rc1 = stage_upload(r, d_tk, rq.tumor_keys, sizeof(UvcTumorKey) * (size_t)rq.n_tumor_keys, stage_at, stage_total); if (rc1) return rc1; }
    }
    if (rq.n_force_sites < 0 || (rq.n_force_sites > 0 && !rq.force_sites)) return fail(UVCGPU_EINVAL, "force_sites: bad count or NULL array");
    if (rq.n_force_sites > 0) {   // force-output sites: sorted zerobased_pos values, uploaded like the tumor keys (k_force_mask makes the bit mask)
        if (r->P.tumor_vcf_is_provided) return fail(UVCGPU_EINVAL, "force_sites cannot go with tumor_vcf_is_provided (the normal sample's gate is the rescue set)");
        for (int64_t q = 1; q < rq.n_force_sites; q++) if (rq.force_sites[q] < rq.force_sites[q - 1]) return fail(UVCGPU_EINVAL, "force_sites must be sorted ascending");
        if (!p.tmp->get(&d_fs, (size_t)rq.n_force_sites)) return no_room();
        { int rc1 = stage_upload(r, d_fs, rq.force_sites, sizeof(int32_t) * (size_t)rq.n_force_sites, stage_at, stage_total); if (rc1) return rc1; }
    }
    if (!rtab.empty()) {   // the ranges, through the staging buffer like the keys and the sites (k_range_map makes the position table)
        if (!p.tmp->get(&d_rg, rtab.size())) return no_room();
        { int rc1 = stage_upload(r, d_rg, rtab.data(), sizeof(UvcScoreRangeDev) * rtab.size(), stage_at, stage_total); if (rc1) return rc1; }
    }
    // The default gate opens a LINK group only at a position with an InDel mark (gate_count: one symbol in the mask and min_altdp_thres > 0
    // give no record), and the accumulate has completed LINK_M in those windows.  A normal sample's gate opens one only at a keyed refpos, forced
    // sites only at the sites: the mark kernel reads the uploaded keys and sites in place.  Every other gate can open one anywhere.
    {
        static_assert(sizeof(UvcTumorKey) % sizeof(int32_t) == 0 && offsetof(UvcTumorKey, refpos) == 0, "k_link_mark strides over UvcTumorKey::refpos");
        const int scope = uvc_link_score_scope_at(rq.all_out, r->P.should_output_all, r->P.tumor_vcf_is_provided, d_tk ? rq.n_tumor_keys : 0, rq.n_force_sites, r->P.min_altdp_thres);
        const int rcl = (scope != UVC_LINK_POSITIONS) ? link_complete(r, scope)
                      : d_tk ? link_complete(r, scope, &d_tk->refpos, rq.n_tumor_keys, (int)(sizeof(UvcTumorKey) / sizeof(int32_t)), r->beg)
                             : link_complete(r, scope, d_fs, rq.n_force_sites, 1, r->beg);
        if (rcl) return rcl;
    }
    p.in = UvcScoreIn{ &r->R, &r->P, &rq, use_al, use_row, n_al, r->d_gap_rows, r->d_gap_seq, d_tk, nullptr, d_fs, d_rg, (int64_t)rtab.size(), npos_scored };
    return 0;
}
// Buf::fit for the score paths, whose failures name the size: `err` with "what (N bytes)"
extern "C++" template <class B>
static int fit_buffer(B &b, size_t need, size_t slack, size_t keep_max, size_t unit, int err, const std::string &what) {
    size_t bytes = 0;
    return b.fit(need, slack, keep_max, unit, &bytes) == hipSuccess ? 0 : fail(err, what + " (" + std::to_string(bytes) + " bytes)");
}
static const size_t SCORE_RECORD_BYTES = sizeof(int32_t) * UVC_NUM_SCORE_FIELDS;   // one record of a [fields][capacity] array
// UvcScoreRequest::release_state: zero the planes on the side stream for the next accumulate, under the copies of the records.  The side
// stream has to be behind the scoring kernels: the one call orders it here (e_fork); a chunk's caller has done so already (behind e_k).
static bool queue_release_state(uvcgpu_region *r, bool stream_already_ordered) {
    if (!stream_already_ordered && (hipEventRecord(r->e_fork, r->stream) != hipSuccess || hipStreamWaitEvent(r->side, r->e_fork, 0) != hipSuccess)) return false;
    if (zero_state(r, r->side) != 0 || hipEventRecord(r->e_join, r->side) != hipSuccess) return false;
    r->state_released = true; r->state_zeroed = true; r->zeroed_bytes = r->L.total; r->dirty_npos = r->npos;
    return true;
}
static int uvcgpu_region_score_impl(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, UvcScoreOut *out) {
    if (!r || !out || !out->fields) return fail(UVCGPU_EINVAL, "bad argument");
    ScorePrep prep;   // (its destructor frees the temporaries on every return path)
    { const int rc0 = score_prepare(r, req, ranges, n_ranges, prep); if (rc0) return rc0; }
    const UvcScoreRequest &rq = prep.rq; const int64_t npos_scored = prep.npos_scored;
    const bool kept_only = (rq.kept_only != 0);
    // device capacity: the caller's in the plain form; with kept_only the caller's buffer only has to hold the kept groups, the device
    // array every record -- start from a guess and grow once if the count says so
    int64_t cap = std::max<int64_t>(out->capacity, 1);
    if (kept_only) cap = std::max<int64_t>(std::max<int64_t>(cap, (int64_t)r->d_score_fields.cap), npos_scored / 8 + 4096);
    int rc = 0;
    int64_t cnt[2] = { 0, 0 };
    for (int attempt = 0; attempt < 2 && !rc; attempt++) {
        if ((rc = fit_buffer(r->d_score_fields, (size_t)cap, 0, 0, SCORE_RECORD_BYTES, UVCGPU_EDEVICE, "score: hipMalloc of the records"))) break;
        // the kept copy has the pitch of the records: exactly their capacity
        if (kept_only && (rc = fit_buffer(r->d_score_kept, r->d_score_fields.cap, 0, r->d_score_fields.cap, SCORE_RECORD_BYTES, UVCGPU_EDEVICE, "score: hipMalloc of the kept records"))) break;
        // the staged rows of the scoring kernels are sized by the record capacity (and the groups of the request)
        const size_t need = uvc_score_scratch_bytes(npos_scored, (int64_t)r->d_score_fields.cap);
        if ((rc = fit_buffer(r->d_score_scratch, need, need / 8, 0, 1, UVCGPU_EDEVICE, "score: hipMalloc of the scratch"))) break;
        r->d_score_count = (int64_t *)r->d_score_scratch.p;   // the record counts head the scratch (zeroed with the scan states)
        HIP_OK(hipMemsetAsync(r->d_score_scratch, 0, uvc_score_scratch_zero_bytes(npos_scored, (int64_t)r->d_score_fields.cap), r->stream));
        const int pi = uvc_prof_begin(&r->prof, "k_score_all", r->stream);   // with profiling on, the scoring kernels (gate + scan + k_score + k_call + the kept-groups copy) as one more entry of uvcgpu_region_kernel_times
        prep.in.scratch = r->d_score_scratch;
        rc = uvc_launch_score(&prep.in, r->d_score_fields, (int64_t)r->d_score_fields.cap, kept_only ? r->d_score_kept : nullptr, r->stream);
        if (rc) rc = fail(rc, "score: the force-output mask could not be cleared");
        uvc_prof_end(&r->prof, pi, r->stream);
        if (!rc && hipGetLastError() != hipSuccess) rc = fail(UVCGPU_EDEVICE, "score kernel launch failed");
        if (!rc) rc = uvcgpu_region_sync(r);
        // copies on the handle's own stream: a null-stream hipMemcpy would also wait for every other handle's work
        if (!rc && (hipMemcpyAsync(cnt, r->d_score_count, 16, hipMemcpyDeviceToHost, r->stream) != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess)) rc = fail(UVCGPU_EDEVICE, "hipMemcpy(count)");
        if (rc || !kept_only || cnt[0] <= (int64_t)r->d_score_fields.cap) break;
        cap = cnt[0] + cnt[0] / 8;   // the guess was too small: nothing was written, once more with room for every record
    }
    if (!rc) {
        const int64_t n_out = (kept_only ? cnt[1] : cnt[0]);
        r->last_scored = cnt[0]; r->last_returned = n_out;
        const int32_t *src = (kept_only ? r->d_score_kept : r->d_score_fields);
        out->n_records = n_out;
        if (kept_only && cnt[0] > (int64_t)r->d_score_fields.cap) rc = fail(UVCGPU_EDEVICE, "score: the record count changed between two passes");
        else if (n_out > out->capacity) rc = fail(UVCGPU_ENOMEM, "score output capacity too small");   // the planes stay: the caller comes back with a larger buffer
        else if (rq.release_state && r->side) (void)queue_release_state(r, false);   // the scoring kernels are done: under the D2H of the records
        if (!rc && n_out > 0 && (hipMemcpy2DAsync(out->fields, sizeof(int32_t) * out->capacity, src, sizeof(int32_t) * (int64_t)r->d_score_fields.cap, sizeof(int32_t) * n_out, UVC_NUM_SCORE_FIELDS, hipMemcpyDeviceToHost, r->stream) != hipSuccess
                             || hipStreamSynchronize(r->stream) != hipSuccess))
            rc = fail(UVCGPU_EDEVICE, "hipMemcpy2D(records)");
    }
    return rc;   // ~ScorePrep frees the temporaries
}

// ---- streamed score (uvcgpu_region_score_stream_begin / uvcgpu_score_stream_next / uvcgpu_score_stream_end) ----
// One gate pass over the whole request and the cut (k_chunk_cut) on the handle's stream, the small chunk table read back once; then the
// per-record kernels chunk by chunk into one of TWO row sets, each with a page-locked host buffer of its own.  Chunk k's kernels run on the
// handle's stream, its D2H on the side stream behind an event; `next` for chunk j queues chunk j + 1 (whose set and host buffer the caller
// gave back with this very call: it held chunk j - 1) and then waits for chunk j's copy alone.  So chunk j + 1 is computed and copied while
// the caller formats chunk j.  Two streams, four events, no graph; no allocation per chunk.
struct ScoreSet { Buf<char> d; Buf<char, true> h; hipEvent_t e_k = nullptr, e_c = nullptr; explicit ScoreSet(const uvcgpu_region *r) : d(r), h(r) {} };   // (cap: bytes)
struct uvcgpu_score_stream {
    uvcgpu_region *r; bool open = false;
    int64_t chunk_records = 0; ScoreSet set[2];          // kept across streams with the same chunk_records
    ScorePrep *prep = nullptr;                           // the open stream's request and its device temporaries
    std::vector<UvcScoreRange> ranges; bool plain = true;   // the request's ranges (a plain request: its one range)
    std::vector<UvcChunkDev> tab;                        // [n_chunks], as k_chunk_cut wrote it
    int64_t n_chunks = 0, launched = 0, returned = 0, ngroups = 0; int with_kept = 0; bool release_queued = false;
    explicit uvcgpu_score_stream(uvcgpu_region *r_) : r(r_), set{ ScoreSet(r_), ScoreSet(r_) } {}
};
static bool stream_is_open(const uvcgpu_region *r) { return r && r->ss && r->ss->open; }
#define UVC_STREAM_HOST_TAIL 64   /* behind the records of a page-locked buffer: */
struct StreamTail { int64_t counts[2]; int32_t err; };   // the set's record counts ([1] = kept records) and the kernels' error word
static_assert(sizeof(StreamTail) <= UVC_STREAM_HOST_TAIL, "the tail of a page-locked records buffer holds a StreamTail");
static StreamTail *stream_tail(const ScoreSet &q, int64_t chunk_records) { return (StreamTail *)(q.h + SCORE_RECORD_BYTES * (size_t)chunk_records); }
static void stream_free_sets(uvcgpu_score_stream *s) {
    for (ScoreSet &q : s->set) { q.d.release(); q.h.release(); }
    s->chunk_records = 0;
}
static void stream_destroy(uvcgpu_region *r) {
    uvcgpu_score_stream *s = r->ss;
    if (!s) return;
    delete s->prep; s->prep = nullptr;
    stream_free_sets(s);
    for (ScoreSet &q : s->set) { if (q.e_k) hipEventDestroy(q.e_k); if (q.e_c) hipEventDestroy(q.e_c); }
    delete s; r->ss = nullptr;
}
// chunk k: kernels on the handle's stream, then counts + records to the set's host buffer on the side stream
static int stream_launch_chunk(uvcgpu_score_stream *s, int64_t k) {
    uvcgpu_region *r = s->r; const ScorePrep &p = *s->prep; ScoreSet &q = s->set[k & 1];
    const UvcChunkDev &t = s->tab[(size_t)k];
    const int64_t c = s->chunk_records, nr = t.nr;
    const int64_t win_groups = std::min<int64_t>(std::min<int64_t>(t.ng, nr), c);   // active groups of the window: at most its groups, at most its records
    int rc = uvc_launch_score_chunk(&p.in, q.d, c, s->with_kept, &t, win_groups, r->stream);
    if (rc) return fail(rc, "score stream: chunk launch refused");
    if (hipGetLastError() != hipSuccess) return fail(UVCGPU_EDEVICE, "score stream: kernel launch failed");
    hipStream_t cs = r->side ? r->side : r->stream;
    HIP_OK(hipEventRecord(q.e_k, r->stream));
    if (r->side) HIP_OK(hipStreamWaitEvent(cs, q.e_k, 0));
    StreamTail *tail = stream_tail(q, c);
    HIP_OK(hipMemcpyAsync(tail->counts, q.d, sizeof(tail->counts), hipMemcpyDeviceToHost, cs));   // (they head the row set)
    HIP_OK(hipMemcpyAsync(&tail->err, r->R.err, sizeof(tail->err), hipMemcpyDeviceToHost, cs));
    // (kept_only: the kept count is on the device; the copy takes the columns of all the chunk's records, of which the kept ones are a prefix --
    //  under -A nearly all of them, at the default gate a few hundred KB more than needed, and nothing waits for a count)
    if (nr > 0) HIP_OK(hipMemcpy2DAsync(q.h, sizeof(int32_t) * (size_t)c, uvc_score_set_fields(q.d, c, s->ngroups, p.rq.kept_only ? 1 : 0), sizeof(int32_t) * (size_t)c, sizeof(int32_t) * (size_t)nr, UVC_NUM_SCORE_FIELDS, hipMemcpyDeviceToHost, cs));
    // behind the last chunk's kernels (and its copy): cs is the side stream, ordered behind e_k above
    if (k == s->n_chunks - 1 && p.rq.release_state && r->side && queue_release_state(r, true)) s->release_queued = true;
    HIP_OK(hipEventRecord(q.e_c, cs));
    s->launched = k + 1;
    return 0;
}
static int stream_close(uvcgpu_score_stream *s) {
    uvcgpu_region *r = s->r;
    int rc = 0;
    if (hipStreamSynchronize(r->stream) != hipSuccess) rc = fail(UVCGPU_EDEVICE, "score stream: hipStreamSynchronize");
    if (r->side && hipStreamSynchronize(r->side) != hipSuccess) rc = fail(UVCGPU_EDEVICE, "score stream: hipStreamSynchronize(side)");
    delete s->prep; s->prep = nullptr;
    s->open = false; s->tab.clear(); s->ranges.clear();
    return rc;
}
static int uvcgpu_region_score_stream_begin_impl(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, int64_t chunk_records, uvcgpu_score_stream_t **out) {
    if (!r || !out) return fail(UVCGPU_EINVAL, "bad argument");
    *out = nullptr;
    if (chunk_records < 1 || chunk_records > INT32_MAX) return fail(UVCGPU_EINVAL, "score stream: chunk_records must be at least 1");
    if (!ranges && n_ranges != 0) return fail(UVCGPU_EINVAL, "score stream: ranges is NULL but n_ranges is not 0");
    std::unique_ptr<ScorePrep> prep(new ScorePrep());
    { const int rc0 = score_prepare(r, req, ranges, n_ranges, *prep); if (rc0) return rc0; }
    if (!r->ss) {
        r->ss = new uvcgpu_score_stream(r);
        for (ScoreSet &q : r->ss->set) if (hipEventCreateWithFlags(&q.e_k, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&q.e_c, hipEventDisableTiming) != hipSuccess) { stream_destroy(r); return fail(UVCGPU_EDEVICE, "hipEventCreate"); }
    }
    uvcgpu_score_stream *s = r->ss;
    const UvcScoreRequest &rq = prep->rq;
    const int64_t npos = prep->npos_scored, ngroups = 2 * npos;
    // a greedy cut leaves no two neighbouring chunks that would fit one: at most 2 * records / chunk_records + 1 chunks, and one per position
    const int64_t upper = NSYM * (npos + 1) + rq.n_indel_alleles + rq.n_tumor_keys + 16 * std::max<int64_t>(rq.n_force_sites, 0) + (int64_t)r->gap_alleles.size();
    const int64_t tab_cap = std::max<int64_t>(1, std::min<int64_t>(npos, 2 * upper / chunk_records + 2));
    // the record-sized buffers of the one-call path go (a later plain call allocates what it needs again); the position-sized scratch is kept
    // when it fits and is not a plain call's record-sized one
    HIP_OK(hipStreamSynchronize(r->stream));
    r->d_score_fields.release(); r->d_score_kept.release();
    const size_t pos_need = uvc_score_stream_pos_bytes(npos, tab_cap);
    r->d_score_count = nullptr;
    { const int rcb = fit_buffer(r->d_score_scratch, pos_need, 0, pos_need + pos_need / 4 + 65536, 1, UVCGPU_ENOMEM, "score stream: hipMalloc of the position-sized scratch"); if (rcb) return rcb; }
    r->d_score_count = (int64_t *)r->d_score_scratch.p;
    prep->in.scratch = r->d_score_scratch;   // (the chunks of the stream use it too)
    const int with_kept = rq.kept_only ? 1 : 0;
    const size_t set_need = uvc_score_set_bytes(chunk_records, ngroups, with_kept), host_need = SCORE_RECORD_BYTES * (size_t)chunk_records + UVC_STREAM_HOST_TAIL;
    if (s->chunk_records != chunk_records) stream_free_sets(s);
    for (ScoreSet &q : s->set) {
        int rcb = fit_buffer(q.d, set_need, 0, 0, 1, UVCGPU_ENOMEM, "score stream: hipMalloc of a row set for chunk_records = " + std::to_string(chunk_records));
        if (!rcb) rcb = fit_buffer(q.h, host_need, 0, 0, 1, UVCGPU_ENOMEM, "score stream: hipHostMalloc of a records buffer");
        if (rcb) { stream_free_sets(s); return rcb; }
    }
    s->chunk_records = chunk_records; s->with_kept = with_kept; s->ngroups = ngroups;
    s->n_chunks = 0; s->launched = 0; s->returned = 0; s->release_queued = false; s->tab.clear();
    s->plain = (ranges == nullptr); s->ranges.clear();
    if (ranges) s->ranges.assign(ranges, ranges + n_ranges);
    else s->ranges.push_back(UvcScoreRange{ rq.pos_beg, rq.pos_end, rq.base_at_pos_beg ? 1 : 0, rq.region_beg });
    if (npos > 0) {
        HIP_OK(hipMemsetAsync(r->d_score_scratch, 0, uvc_score_scratch_zero_bytes(npos, 1), r->stream));
        int rc = uvc_launch_score_gate(&prep->in, chunk_records, tab_cap, r->stream);
        if (rc) return fail(rc, "score stream: the force-output mask could not be cleared");
        if (hipGetLastError() != hipSuccess) return fail(UVCGPU_EDEVICE, "score stream: kernel launch failed");
        { const int rcs = uvcgpu_region_sync(r); if (rcs) return rcs; }
        const char *d_tab = r->d_score_scratch + uvc_score_stream_table_offset(npos);
        int64_t hdr[4] = { 0, 0, 0, 0 };
        if (hipMemcpyAsync(hdr, d_tab, 32, hipMemcpyDeviceToHost, r->stream) != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess) return fail(UVCGPU_EDEVICE, "score stream: hipMemcpy(chunk count)");
        if (hdr[0] == -1) {   // one position alone is more than a chunk: name it (compact position -> zerobased_pos)
            int64_t z = hdr[1], at = 0;
            for (const UvcScoreRange &g : s->ranges) { const int64_t len = std::max<int64_t>((int64_t)g.pos_end - g.pos_beg, 0); if (hdr[1] < at + len) { z = g.pos_beg + (hdr[1] - at); break; } at += len; }
            return fail(UVCGPU_ENOMEM, "score stream: zerobased_pos " + std::to_string(z) + " alone has " + std::to_string(hdr[2]) + " records, more than chunk_records = " + std::to_string(chunk_records));
        }
        if (hdr[0] < 0 || hdr[0] > tab_cap) return fail(UVCGPU_EDEVICE, "score stream: the chunk table overflowed");
        s->n_chunks = hdr[0];
        s->tab.resize((size_t)s->n_chunks);
        if (s->n_chunks > 0 && (hipMemcpyAsync(s->tab.data(), d_tab + 32, sizeof(UvcChunkDev) * (size_t)s->n_chunks, hipMemcpyDeviceToHost, r->stream) != hipSuccess || hipStreamSynchronize(r->stream) != hipSuccess)) return fail(UVCGPU_EDEVICE, "score stream: hipMemcpy(chunk table)");
    }
    s->prep = prep.release(); s->open = true;
    r->last_scored = 0; r->last_returned = 0;
    for (int64_t k = 0; k < std::min<int64_t>(2, s->n_chunks); k++) { const int rc = stream_launch_chunk(s, k); if (rc) { const std::string msg = g_err; stream_close(s); return fail(rc, msg); } }
    *out = s;
    return 0;
}
static int uvcgpu_score_stream_next_impl(uvcgpu_score_stream_t *s, UvcScoreOut *chunk, UvcScoreRange *covered, int64_t *n_covered) {
    if (!s || !chunk) return fail(UVCGPU_EINVAL, "bad argument");
    if (!s->open) return fail(UVCGPU_ESTATE, "score stream: not open");
    uvcgpu_region *r = s->r;
    if (n_covered) *n_covered = 0;
    chunk->capacity = s->chunk_records; chunk->n_records = 0; chunk->fields = (int32_t *)s->set[0].h.p;
    const int64_t j = s->returned;
    if (j >= s->n_chunks) return UVCGPU_STREAM_END;
    // this call gives back the buffers of chunk j - 1: chunk j + 1 takes them
    if (j + 1 < s->n_chunks && s->launched == j + 1) { const int rc = stream_launch_chunk(s, j + 1); if (rc) return rc; }
    ScoreSet &q = s->set[j & 1];
    HIP_OK(hipEventSynchronize(q.e_c));
    const UvcChunkDev &t = s->tab[(size_t)j];
    const StreamTail tail = *stream_tail(q, s->chunk_records);
    if (tail.err) return fail(tail.err, "a scoring kernel flagged an error");
    const int64_t n_out = (s->prep->rq.kept_only ? tail.counts[1] : (int64_t)t.nr);
    if (n_out < 0 || n_out > t.nr) return fail(UVCGPU_EDEVICE, "score stream: the kept count of a chunk is out of range");
    chunk->fields = (int32_t *)q.h.p; chunk->n_records = n_out;
    r->last_scored += t.nr; r->last_returned += n_out;
    // the ranges this chunk covers: the request's ranges cut to the chunk's compact positions; a piece that begins inside a range continues it
    const int64_t c0 = t.g0 / 2, c1 = c0 + t.ng / 2;
    int64_t at = 0, nc = 0;
    for (const UvcScoreRange &g : s->ranges) {
        const int64_t len = std::max<int64_t>((int64_t)g.pos_end - g.pos_beg, 0), lo = std::max(c0, at), hi = std::min(c1, at + len);
        if (hi > lo) {
            if (covered) covered[nc] = UvcScoreRange{ (int32_t)(g.pos_beg + (lo - at)), (int32_t)(g.pos_beg + (hi - at)), (lo > at) ? 1 : g.base_at_pos_beg, g.region_beg };
            nc++;
        }
        at += len;
    }
    if (n_covered) *n_covered = nc;
    s->returned = j + 1;
    return 0;
}
static int uvcgpu_score_stream_end_impl(uvcgpu_score_stream_t *s) {
    if (!s) return fail(UVCGPU_EINVAL, "null stream");
    if (!s->open) return fail(UVCGPU_ESTATE, "score stream: not open");
    return stream_close(s);
}
int uvcgpu_region_score_stream_begin(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, int64_t chunk_records, uvcgpu_score_stream_t **out) {
    return guarded("uvcgpu_region_score_stream_begin", [&] { return uvcgpu_region_score_stream_begin_impl(r, req, ranges, n_ranges, chunk_records, out); });
}
int uvcgpu_score_stream_next(uvcgpu_score_stream_t *s, UvcScoreOut *chunk, UvcScoreRange *covered, int64_t *n_covered) { return guarded("uvcgpu_score_stream_next", [&] { return uvcgpu_score_stream_next_impl(s, chunk, covered, n_covered); }); }
int uvcgpu_score_stream_end(uvcgpu_score_stream_t *s) { return guarded("uvcgpu_score_stream_end", [&] { return uvcgpu_score_stream_end_impl(s); }); }
int64_t uvcgpu_score_stream_bytes_per_record(void) { return 2 * ((int64_t)uvc_score_set_bytes_per_record() + (int64_t)SCORE_RECORD_BYTES); }
int64_t uvcgpu_score_stream_footprint(const uvcgpu_region_t *r) {
    if (!r) return -1;
    int64_t b = (int64_t)r->d_score_scratch.cap + (int64_t)r->h_stage.cap;
    if (r->d_score_fields) b += (int64_t)SCORE_RECORD_BYTES * (int64_t)r->d_score_fields.cap;
    if (r->d_score_kept) b += (int64_t)SCORE_RECORD_BYTES * (int64_t)r->d_score_kept.cap;
    if (r->ss) for (const ScoreSet &q : r->ss->set) b += (int64_t)q.d.cap + (int64_t)q.h.cap;
    return b;
}

// ---- the report calls: uvcgpu_region_coverage, _error_profile, _family_stats, _callable, _read_profile, _msi, _fragment_profile, _site_reads, _clip_sites, _clip_junctions, _clip_mates and _family_concordance ----
// What the twelve share.  Each is synchronous: a checked list of sorted, disjoint ranges (the site call: of ascending sites) goes up through the staging buffer into the head of
// the handle's report buffer, the kernels write behind it, and the result comes home through the page-locked report buffer.

// The state a call needs.  planes_to ("reduce", "classify"): a reader of the accumulated planes; NULL: a reader of the family units, which
// belong to the reads of the handle and are there from set_reads on, whatever was scored since.
static int report_guard(const uvcgpu_region_t *r, const std::string &call, const char *planes_to, const char *reads_give = "family units") {
    if (!r) return fail(UVCGPU_EINVAL, call + ": null region");
    if (!planes_to) return r->reads_given ? 0 : fail(UVCGPU_EINVAL, call + " before set_reads: the region has no " + reads_give + " yet (uvcgpu_region_set_reads or _set_reads_device of this region comes first)");
    if (!r->accumulated) return fail(UVCGPU_EINVAL, call + " before accumulate: there are no planes to " + planes_to);
    if (r->state_released) return fail(UVCGPU_EINVAL, call + " after the planes were released by the last score (UvcScoreRequest::release_state): call it before that score");
    if (stream_is_open(r)) return fail(UVCGPU_EINVAL, call + " while a score stream is open on this handle (the stream may release the planes): call it before uvcgpu_region_score_stream_begin");
    return 0;
}
// The state of the one call that evaluates the units' votes again (uvcgpu_region_family_concordance).  It reads what accumulate leaves beside
// the planes -- RegionDev::ffast / frag_rank, the contribution table, the InDel-phred track as P1b edited it -- and none of the planes: only
// set_reads, reset and correct_bq end its window (each clears `accumulated`), a releasing score and an open score stream do not.
static int report_guard_votes(const uvcgpu_region_t *r, const std::string &call) {
    if (!r) return fail(UVCGPU_EINVAL, call + ": null region");
    if (!r->reads_given) return fail(UVCGPU_EINVAL, call + " before set_reads: the region has no family units yet (uvcgpu_region_set_reads or _set_reads_device of this region comes first)");
    if (r->has_reads && !r->accumulated) return fail(UVCGPU_EINVAL, call + " before accumulate: there are no fragment records and no contribution table to take the votes from (uvcgpu_region_accumulate of the current reads comes first)");
    return 0;
}
static int range_count(const std::string &call, int64_t n_ranges, int64_t most) {
    if (n_ranges < 1) return fail(UVCGPU_EINVAL, call + ": n_ranges " + std::to_string(n_ranges) + " must be at least 1");
    if (n_ranges > most) return fail(UVCGPU_EINVAL, call + ": n_ranges " + std::to_string(n_ranges) + " is more than one call takes (" + std::to_string(most) + ")");
    return 0;
}
static std::string range_name(const std::string &call, int64_t k, int32_t pos_beg, int32_t pos_end) {
    return call + ": range " + std::to_string(k) + " [" + std::to_string(pos_beg) + ", " + std::to_string(pos_end) + ")";
}
// The rules of a range list: no range empty, every range inside the region, sorted and disjoint.  last_end: the end of range k - 1 (not read
// for k = 0).  The text is made for a range that breaks a rule only: a list can have a million ranges.
static int range_check(const uvcgpu_region_t *r, const std::string &call, int64_t k, int32_t pos_beg, int32_t pos_end, int32_t last_end) {
    if (pos_end <= pos_beg) return fail(UVCGPU_EINVAL, range_name(call, k, pos_beg, pos_end) + " is empty");
    if (pos_beg < r->beg || pos_end > r->end) return fail(UVCGPU_EINVAL, range_name(call, k, pos_beg, pos_end) + " is outside the region [" + std::to_string(r->beg) + ", " + std::to_string(r->end) + ")");
    if (k > 0 && pos_beg < last_end) return fail(UVCGPU_EINVAL, range_name(call, k, pos_beg, pos_end) + " begins in front of the end " + std::to_string(last_end) + " of range " + std::to_string(k - 1) + " (ranges must be sorted and disjoint)");
    return 0;
}
// The list of a plane reader, checked range by range, as the table its kernels search (UvcRangeRow, uvc_launch.h): n_ranges rows and the
// { 0, n_total } behind them.  The caller has checked n_ranges (range_count, at most INT32_MAX >> 1: compact positions are 32-bit).
static int range_table(const uvcgpu_region_t *r, const std::string &call, const UvcCoverageRange *ranges, int64_t n_ranges, std::vector<UvcRangeRow> &tab, int64_t &n_total) {
    tab.resize((size_t)n_ranges + 1);
    n_total = 0;
    for (int64_t k = 0; k < n_ranges; k++) {
        const UvcCoverageRange &q = ranges[k];
        { int rc1 = range_check(r, call, k, q.pos_beg, q.pos_end, k > 0 ? ranges[k - 1].pos_end : 0); if (rc1) return rc1; }
        tab[(size_t)k] = UvcRangeRow{ q.pos_beg - r->beg, (int32_t)n_total };
        n_total += (int64_t)q.pos_end - q.pos_beg;   // (<= npos: the ranges are disjoint and inside the region)
    }
    tab[(size_t)n_ranges] = UvcRangeRow{ 0, (int32_t)n_total };
    return 0;
}
// The pieces of a call in the device report buffer, each on a 64-byte boundary: take() returns a piece's offset, bytes is the room so far
struct ReportLayout {
    size_t bytes = 0;
    size_t take(size_t n) { const size_t at = bytes; bytes += (n + 63) & ~(size_t)63; return at; }
};
// the device and the page-locked buffer that the report calls share (every one synchronises before it returns), grown on demand
static int report_buffers(uvcgpu_region_t *r, size_t dev_bytes, size_t out_bytes, const char *what) {
    if (r->d_report.fit(dev_bytes, dev_bytes / 2) != hipSuccess) return fail(UVCGPU_ENOMEM, std::string("hipMalloc(") + what + ") failed");
    if (r->h_report.fit(out_bytes, out_bytes / 2) != hipSuccess) return fail(UVCGPU_ENOMEM, std::string("hipHostMalloc(") + what + ") failed");
    return 0;
}
// Room for a call's pieces and its result, and the range list (piece 0 of every layout) on its way: through the handle's staging buffer
// (stage_upload: never an asynchronous copy from the caller's or the heap's pages); an earlier call's copy out of it is complete, every
// user of the buffer synchronises before it returns.
static int report_begin(uvcgpu_region_t *r, const ReportLayout &L, size_t out_bytes, const char *what, const void *list, size_t list_bytes) {
    { int rc1 = report_buffers(r, L.bytes, out_bytes, what); if (rc1) return rc1; }
    size_t at = 0;
    return stage_upload(r, r->d_report, list, list_bytes, at, (list_bytes + 63) & ~(size_t)63);
}
// What was launched, to the caller: the launch's status, `bytes` from the device into the page-locked buffer, the wait, the copy out.  The
// plane readers wait with uvcgpu_region_sync, which also reports a read shape that an accumulate kernel flagged; the family call, legal
// before any accumulate, waits for the stream alone.
static int report_result(uvcgpu_region_t *r, const void *d_src, void *dst, size_t bytes, bool planes) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(r->h_report, d_src, bytes, hipMemcpyDeviceToHost, r->stream));
    if (planes) { int rc1 = uvcgpu_region_sync(r); if (rc1) return rc1; }
    else HIP_OK(hipStreamSynchronize(r->stream));
    memcpy(dst, r->h_report, bytes);
    return 0;
}

// ---- depth statistics of ranges (uvc_coverage.hip): [table] [result rows] [scratch rows] ----
static int uvcgpu_region_coverage_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const int32_t *thresholds, int32_t n_thresholds, int64_t *out) {
    { int rc1 = report_guard(r, "coverage", "reduce"); if (rc1) return rc1; }
    if (!ranges || !out) return fail(UVCGPU_EINVAL, "coverage: ranges and out must not be NULL");
    { int rc1 = range_count("coverage", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    if (n_thresholds < 0 || n_thresholds > UVC_COV_MAX_THRESHOLDS || (n_thresholds > 0 && !thresholds)) return fail(UVCGPU_EINVAL, "coverage: n_thresholds " + std::to_string(n_thresholds) + " is outside 0.." + std::to_string((int)UVC_COV_MAX_THRESHOLDS));
    for (int32_t k = 0; k < n_thresholds; k++) {
        if (thresholds[k] < 0) return fail(UVCGPU_EINVAL, "coverage: threshold " + std::to_string(k) + " is negative (" + std::to_string(thresholds[k]) + ")");
        if (k > 0 && thresholds[k] <= thresholds[k - 1]) return fail(UVCGPU_EINVAL, "coverage: threshold " + std::to_string(k) + " (" + std::to_string(thresholds[k]) + ") is not larger than the one before it (" + std::to_string(thresholds[k - 1]) + "): thresholds ascend");
    }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "coverage", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const int64_t scratch_rows = uvc_coverage_scratch_rows((int)n_ranges, n_total);   // the shard copies of few long ranges (0: the waves merge into the result rows)
    const size_t row_bytes = sizeof(int64_t) * UVC_NCOV * UVC_COV_ROW, out_bytes = row_bytes * (size_t)n_ranges;
    ReportLayout L;
    const size_t o_tab = L.take(sizeof(UvcRangeRow) * tab.size()), o_rows = L.take(out_bytes), o_scratch = L.take(row_bytes * (size_t)scratch_rows);
    { int rc1 = report_begin(r, L, out_bytes, "coverage rows", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
    long long *d_rows = (long long *)(r->d_report + o_rows);
    uvc_launch_coverage(&r->R, (const UvcRangeRow *)(r->d_report + o_tab), (int)n_ranges, n_total, thresholds, n_thresholds, d_rows, (long long *)(r->d_report + o_scratch), scratch_rows, r->stream);
    return report_result(r, d_rows, out, out_bytes, true);
}
int uvcgpu_region_coverage(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const int32_t *thresholds, int32_t n_thresholds, int64_t *out) {
    return guarded("uvcgpu_region_coverage", [&] { return uvcgpu_region_coverage_impl(r, ranges, n_ranges, thresholds, n_thresholds, out); });
}
const char *uvcgpu_coverage_measure_name(int32_t id) { return uvc_coverage_name(id); }

// ---- background error profile of ranges (uvc_errprofile.hip): [table] [profile] [shard copies] ----
static int uvcgpu_region_error_profile_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcErrorProfileRequest *req, int64_t *out) {
    { int rc1 = report_guard(r, "error_profile", "reduce"); if (rc1) return rc1; }
    if (!ranges || !req || !out) return fail(UVCGPU_EINVAL, "error_profile: ranges, req and out must not be NULL");
    if (req->min_depth < 1) return fail(UVCGPU_EINVAL, "error_profile: min_depth " + std::to_string(req->min_depth) + " must be at least 1");
    if (req->max_alt_permille < 0 || req->max_alt_permille > 1000) return fail(UVCGPU_EINVAL, "error_profile: max_alt_permille " + std::to_string(req->max_alt_permille) + " is outside 0..1000");
    { int rc1 = range_count("error_profile", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "error_profile", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const size_t out_bytes = sizeof(int64_t) * UVC_NERRLEVEL * UVC_ERR_ROW;
    ReportLayout L;
    const size_t o_tab = L.take(sizeof(UvcRangeRow) * tab.size()), o_prof = L.take(out_bytes), o_scratch = L.take(sizeof(int64_t) * (size_t)uvc_errprofile_scratch_cells());
    { int rc1 = report_begin(r, L, out_bytes, "error profile", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
    long long *d_prof = (long long *)(r->d_report + o_prof);
    uvc_launch_errprofile(&r->R, (const UvcRangeRow *)(r->d_report + o_tab), (int)n_ranges, n_total, req->min_depth, req->max_alt_permille, d_prof, (long long *)(r->d_report + o_scratch), r->stream);
    return report_result(r, d_prof, out, out_bytes, true);
}
int uvcgpu_region_error_profile(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcErrorProfileRequest *req, int64_t *out) {
    return guarded("uvcgpu_region_error_profile", [&] { return uvcgpu_region_error_profile_impl(r, ranges, n_ranges, req, out); });
}
const char *uvcgpu_error_level_name(int32_t id) { return uvc_errprofile_level_name(id); }

// ---- family statistics of ranges (uvc_famstats.hip): [ranges] [rows] [unit spans] ----
// The unit records, the fragments and the per-alignment columns belong to the reads of the handle (uvcgpu_region::owned): only set_reads, reset
// and destroy free them, and the first two are refused while a score stream is open.  A score with release_state gives up the planes and
// nothing else.  So the call is legal from set_reads on, whatever was scored since.  Its kernels read the caller's rows as they are, no table.
// The rules of a list of UvcFamilyRange rows (uvcgpu_region_family_stats, _fragment_profile): those of a range list, and prev_end and the flags
static int family_ranges_check(const uvcgpu_region_t *r, const std::string &call, const UvcFamilyRange *ranges, int64_t n_ranges) {
    { int rc1 = range_count(call, n_ranges, INT32_MAX >> 10); if (rc1) return rc1; }
    for (int64_t k = 0; k < n_ranges; k++) {
        const UvcFamilyRange &q = ranges[k];
        { int rc1 = range_check(r, call, k, q.pos_beg, q.pos_end, k > 0 ? ranges[k - 1].pos_end : 0); if (rc1) return rc1; }
        auto name = [&] { return range_name(call, k, q.pos_beg, q.pos_end); };
        if (q.prev_end > q.pos_beg) return fail(UVCGPU_EINVAL, name() + " has prev_end " + std::to_string(q.prev_end) + " behind its begin (prev_end is the end of an earlier range)");
        if (k > 0 && q.prev_end < ranges[k - 1].prev_end) return fail(UVCGPU_EINVAL, name() + " has prev_end " + std::to_string(q.prev_end) + " below the prev_end " + std::to_string(ranges[k - 1].prev_end) + " of range " + std::to_string(k - 1) + " (prev_end must not decrease)");
        if (k > 0 && q.prev_end < ranges[k - 1].pos_end) return fail(UVCGPU_EINVAL, name() + " has prev_end " + std::to_string(q.prev_end) + " below the end " + std::to_string(ranges[k - 1].pos_end) + " of range " + std::to_string(k - 1) + ": that range's families would be counted twice");
        if (q.flags & ~(int32_t)UVC_FAMRANGE_CONTINUES) return fail(UVCGPU_EINVAL, name() + " has unknown flag bits (flags " + std::to_string(q.flags) + "; only UVC_FAMRANGE_CONTINUES = 1 is defined)");
    }
    return 0;
}
static int uvcgpu_region_family_stats_impl(uvcgpu_region_t *r, const UvcFamilyRange *ranges, int64_t n_ranges, int64_t *out) {
    { int rc1 = report_guard(r, "family_stats", nullptr); if (rc1) return rc1; }
    if (!ranges || !out) return fail(UVCGPU_EINVAL, "family_stats: ranges and out must not be NULL");
    { int rc1 = family_ranges_check(r, "family_stats", ranges, n_ranges); if (rc1) return rc1; }
    const size_t out_bytes = sizeof(int64_t) * UVC_FAMSTAT_ROW * (size_t)n_ranges;
    if (!r->has_reads) { memset(out, 0, out_bytes); return 0; }   // set_reads with zero reads: no family, nothing to launch
    ReportLayout L;
    const size_t o_ranges = L.take(sizeof(UvcFamilyRange) * (size_t)n_ranges), o_rows = L.take(out_bytes), o_span = L.take(sizeof(UvcUnitSpan) * (size_t)std::max(r->R.n_fs, 1));
    { int rc1 = report_begin(r, L, out_bytes, "family statistics", ranges, sizeof(UvcFamilyRange) * (size_t)n_ranges); if (rc1) return rc1; }
    long long *d_rows = (long long *)(r->d_report + o_rows);
    const int pi = uvc_prof_begin(&r->prof, "k_famstats", r->stream);   // with profiling on, the three kernels as one more entry of uvcgpu_region_kernel_times (accumulate starts the list anew)
    uvc_launch_famstats(&r->R, r->W.pos, r->W.endpos, r->W.fs, (UvcUnitSpan *)(r->d_report + o_span), (const UvcFamilyRange *)(r->d_report + o_ranges), (int)n_ranges, d_rows, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    return report_result(r, d_rows, out, out_bytes, false);
}
int uvcgpu_region_family_stats(uvcgpu_region_t *r, const UvcFamilyRange *ranges, int64_t n_ranges, int64_t *out) {
    return guarded("uvcgpu_region_family_stats", [&] { return uvcgpu_region_family_stats_impl(r, ranges, n_ranges, out); });
}
const char *uvcgpu_family_stat_name(int32_t id) { return uvc_famstats_name(id); }

// ---- family concordance of ranges (the end of uvc_kernels_acc.hip): [table] [row] [shard copies] ----
static int uvcgpu_region_family_concordance_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, int64_t *out) {
    { int rc1 = report_guard_votes(r, "family_concordance"); if (rc1) return rc1; }
    if (!ranges || !out) return fail(UVCGPU_EINVAL, "family_concordance: ranges and out must not be NULL");
    { int rc1 = range_count("family_concordance", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "family_concordance", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const size_t out_bytes = sizeof(int64_t) * UVC_FAMCONC_ROW;
    if (!r->has_reads) { memset(out, 0, out_bytes); return 0; }   // set_reads with zero reads: no unit, nothing to launch
    ReportLayout L;
    const size_t o_tab = L.take(sizeof(UvcRangeRow) * tab.size()), o_row = L.take(out_bytes), o_scratch = L.take(sizeof(int64_t) * (size_t)uvc_famconcord_scratch_cells());
    { int rc1 = report_begin(r, L, out_bytes, "family concordance", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
    long long *d_row = (long long *)(r->d_report + o_row);
    uvc_launch_famconcord(&r->R, &r->P, (const UvcRangeRow *)(r->d_report + o_tab), (int)n_ranges, r->d_dup_units, r->n_dup, r->d_dup_off, r->n_dup_work, d_row,
                          (long long *)(r->d_report + o_scratch), &r->prof, r->stream);
    return report_result(r, d_row, out, out_bytes, true);
}
int uvcgpu_region_family_concordance(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, int64_t *out) {
    return guarded("uvcgpu_region_family_concordance", [&] { return uvcgpu_region_family_concordance_impl(r, ranges, n_ranges, out); });
}
const char *uvcgpu_family_concordance_section_name(int32_t id) { return uvc_famconcord_section_name(id); }

// ---- fragment length and end-motif profile of ranges (uvc_fragprofile.hip): [ranges] [TARGET rows, the profile row] [profile copies]
// [fragment spans] [unit template spans] ----
// The reads' columns, fragments and units: the legality and the ranges are those of uvcgpu_region_family_stats.
static int uvcgpu_region_fragment_profile_impl(uvcgpu_region_t *r, const UvcFamilyRange *ranges, int64_t n_ranges, const UvcFragmentProfileRequest *req, int64_t *out_ranges, int64_t *out_profile) {
    { int rc1 = report_guard(r, "fragment_profile", nullptr, "fragments"); if (rc1) return rc1; }
    if (!ranges || !req || !out_ranges || !out_profile) return fail(UVCGPU_EINVAL, "fragment_profile: ranges, req, out_ranges and out_profile must not be NULL");
    if (req->min_mapq < 0 || req->min_mapq > 255) return fail(UVCGPU_EINVAL, "fragment_profile: min_mapq " + std::to_string(req->min_mapq) + " is outside 0..255");
    if (req->short_lo < 0 || req->short_hi < 0 || req->long_lo < 0 || req->long_hi < 0)
        return fail(UVCGPU_EINVAL, "fragment_profile: a length bound is negative (short " + std::to_string(req->short_lo) + "-" + std::to_string(req->short_hi) + ", long " + std::to_string(req->long_lo) + "-" + std::to_string(req->long_hi) + ")");
    if (req->short_lo > req->short_hi) return fail(UVCGPU_EINVAL, "fragment_profile: short_lo " + std::to_string(req->short_lo) + " is above short_hi " + std::to_string(req->short_hi));
    if (req->long_lo > req->long_hi) return fail(UVCGPU_EINVAL, "fragment_profile: long_lo " + std::to_string(req->long_lo) + " is above long_hi " + std::to_string(req->long_hi));
    { int rc1 = family_ranges_check(r, "fragment_profile", ranges, n_ranges); if (rc1) return rc1; }
    const size_t rows_bytes = sizeof(int64_t) * UVC_FRAGPROF_TARGET_ROW * (size_t)n_ranges, prof_bytes = sizeof(int64_t) * UVC_FRAGPROF_ROW, out_bytes = rows_bytes + prof_bytes;
    if (!r->has_reads) { memset(out_ranges, 0, rows_bytes); memset(out_profile, 0, prof_bytes); return 0; }   // set_reads with zero reads: no fragment, nothing to launch
    ReportLayout L;
    const size_t o_ranges = L.take(sizeof(UvcFamilyRange) * (size_t)n_ranges), o_out = L.take(out_bytes), o_parts = L.take(prof_bytes * (size_t)uvc_fragprofile_copies());
    const size_t o_fspan = L.take(sizeof(UvcFragSpan) * (size_t)std::max(r->R.n_frags, 1)), o_uspan = L.take(sizeof(UvcUnitSpan) * (size_t)std::max(r->R.n_fs, 1));
    { int rc1 = report_begin(r, L, out_bytes, "fragment profile", ranges, sizeof(UvcFamilyRange) * (size_t)n_ranges); if (rc1) return rc1; }
    long long *d_out = (long long *)(r->d_report + o_out);
    const int pi = uvc_prof_begin(&r->prof, "k_fragprofile", r->stream);   // with profiling on, the five kernels as one more entry of uvcgpu_region_kernel_times
    uvc_launch_fragprofile(&r->R, &r->W, req, (UvcFragSpan *)(r->d_report + o_fspan), (UvcUnitSpan *)(r->d_report + o_uspan), (const UvcFamilyRange *)(r->d_report + o_ranges), (int)n_ranges, d_out,
                           (long long *)(r->d_report + o_parts), r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    // the rows and the profile come home in one copy and part in the page-locked buffer
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(r->h_report, d_out, out_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipStreamSynchronize(r->stream));
    memcpy(out_ranges, r->h_report, rows_bytes);
    memcpy(out_profile, (const char *)r->h_report + rows_bytes, prof_bytes);
    return 0;
}
int uvcgpu_region_fragment_profile(uvcgpu_region_t *r, const UvcFamilyRange *ranges, int64_t n_ranges, const UvcFragmentProfileRequest *req, int64_t *out_ranges, int64_t *out_profile) {
    return guarded("uvcgpu_region_fragment_profile", [&] { return uvcgpu_region_fragment_profile_impl(r, ranges, n_ranges, req, out_ranges, out_profile); });
}
const char *uvcgpu_fragment_profile_name(int32_t id) { return uvc_fragprofile_name(id); }

// ---- base-quality and cycle profile of the reads over ranges (uvc_readprofile.hip): [table] [D, X: 2 x npos int32] [status: npos bytes]
// [profile copies: the result row and the shard copies] [scratch ints: the chunk prefix of the alignments and the tile sums of the scans] ----
// The read columns, bases, qualities and CIGARs belong to the reads of the handle as the family units do: the legality is that of
// uvcgpu_region_family_stats.  Without reads the status stage runs on zero depths and the row holds positions_* alone.
static int uvcgpu_region_read_profile_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcReadProfileRequest *req, int64_t *out) {
    { int rc1 = report_guard(r, "read_profile", nullptr, "reads"); if (rc1) return rc1; }
    if (!ranges || !req || !out) return fail(UVCGPU_EINVAL, "read_profile: ranges, req and out must not be NULL");
    if (req->min_mapq < 0 || req->min_mapq > 255) return fail(UVCGPU_EINVAL, "read_profile: min_mapq " + std::to_string(req->min_mapq) + " is outside 0..255");
    if (req->min_depth < 1) return fail(UVCGPU_EINVAL, "read_profile: min_depth " + std::to_string(req->min_depth) + " must be at least 1");
    if (req->max_alt_permille < 0 || req->max_alt_permille > 1000) return fail(UVCGPU_EINVAL, "read_profile: max_alt_permille " + std::to_string(req->max_alt_permille) + " is outside 0..1000");
    { int rc1 = range_count("read_profile", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "read_profile", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const int64_t n_alns = r->has_reads ? r->R.n_alns : 0;
    RegionDev R0 = r->R; if (!r->has_reads) R0.n_alns = 0;   // (the read pointers of an earlier region are gone)
    const size_t npos = (size_t)r->npos, out_bytes = sizeof(int64_t) * UVC_READPROF_ROW, copies = 1 + (size_t)uvc_readprofile_copies();
    ReportLayout L;
    const size_t o_tab = L.take(sizeof(UvcRangeRow) * tab.size()), o_dx = L.take(sizeof(int32_t) * 2 * npos), o_status = L.take(npos), o_prof = L.take(out_bytes * copies);
    const size_t o_scratch = L.take(sizeof(int32_t) * (size_t)uvc_readprofile_scratch_ints(n_alns, r->npos));
    { int rc1 = report_begin(r, L, out_bytes, "read profile", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
    int32_t *d_dx = (int32_t *)(r->d_report + o_dx), *d_x = d_dx + npos, *d_scratch = (int32_t *)(r->d_report + o_scratch);
    uint8_t *d_status = (uint8_t *)(r->d_report + o_status);
    long long *d_prof = (long long *)(r->d_report + o_prof), *d_parts = d_prof + UVC_READPROF_ROW;
    HIP_OK(hipMemsetAsync(r->d_report + o_dx, 0, o_scratch - o_dx, r->stream));   // D, X, status, the copies
    // with profiling on, three more entries of uvcgpu_region_kernel_times (accumulate starts the list anew)
    int pi = uvc_prof_begin(&r->prof, "k_readprofile_depth", r->stream);
    uvc_launch_readprofile_depth(&R0, &r->W, r->n_bases, req->min_mapq, d_dx, d_x, d_scratch, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    pi = uvc_prof_begin(&r->prof, "k_readprofile_status", r->stream);
    uvc_launch_readprofile_status(&R0, (const UvcRangeRow *)(r->d_report + o_tab), (int)n_ranges, req->min_depth, req->max_alt_permille, d_dx, d_x, d_status, d_parts, d_scratch, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    pi = uvc_prof_begin(&r->prof, "k_readprofile_bin", r->stream);
    uvc_launch_readprofile_bin(&R0, &r->W, r->n_bases, req->min_mapq, d_status, d_parts, d_prof, d_scratch, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    return report_result(r, d_prof, out, out_bytes, false);
}
int uvcgpu_region_read_profile(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcReadProfileRequest *req, int64_t *out) {
    return guarded("uvcgpu_region_read_profile", [&] { return uvcgpu_region_read_profile_impl(r, ranges, n_ranges, req, out); });
}
const char *uvcgpu_read_class_name(int32_t c) { return uvc_readprofile_class_name(c); }

// ---- the alignments behind listed sites (uvc_sitereads.hip): [sites] [counts, n_sites x 8 ints] [scratch ints] [rows, `room` of them] ----
// The read columns, CIGARs and packed base | quality belong to the reads of the handle: the legality is that of uvcgpu_region_family_stats.
// Sizes first, in one pass where the buffer allows (as uvcgpu_region_msi): the count runs, the host reads the number of items, the number
// of kept rows and the counts in one wait, and only a call with enough room launches the write and copies 32 bytes per row.  A call whose
// caller has room the device buffer lacks lays the buffer out for that number of rows and counts once more (the buffer keeps its size).
static int uvcgpu_region_site_reads_impl(uvcgpu_region_t *r, const int32_t *sites, int64_t n_sites, const UvcSiteReadsRequest *req, int32_t *counts, UvcSiteRead *rows, int64_t row_capacity, int64_t *n_rows) {
    { int rc1 = report_guard(r, "site_reads", nullptr, "reads"); if (rc1) return rc1; }
    if (!sites || !req || !counts || !n_rows) return fail(UVCGPU_EINVAL, "site_reads: sites, req, counts and n_rows must not be NULL");
    if (n_sites < 1) return fail(UVCGPU_EINVAL, "site_reads: n_sites " + std::to_string(n_sites) + " must be at least 1");
    if (req->min_mapq < 0 || req->min_mapq > 255) return fail(UVCGPU_EINVAL, "site_reads: min_mapq " + std::to_string(req->min_mapq) + " is outside 0..255");
    if (req->alt_only < 0 || req->alt_only > 1) return fail(UVCGPU_EINVAL, "site_reads: alt_only " + std::to_string(req->alt_only) + " is outside 0..1");
    if (row_capacity < 0) return fail(UVCGPU_EINVAL, "site_reads: row_capacity " + std::to_string(row_capacity) + " is negative");
    if (!rows && row_capacity > 0) return fail(UVCGPU_EINVAL, "site_reads: rows is NULL with row_capacity " + std::to_string(row_capacity));
    for (int64_t k = 0; k < n_sites; k++) {
        if (sites[k] < r->beg || sites[k] >= r->end) return fail(UVCGPU_EINVAL, "site_reads: site " + std::to_string(k) + " (" + std::to_string(sites[k]) + ") is outside the region [" + std::to_string(r->beg) + ", " + std::to_string(r->end) + ")");
        if (k > 0 && sites[k] <= sites[k - 1]) return fail(UVCGPU_EINVAL, "site_reads: site " + std::to_string(k) + " (" + std::to_string(sites[k]) + ") is not above site " + std::to_string(k - 1) + " (" + std::to_string(sites[k - 1]) + "): sites ascend strictly");
    }
    const size_t counts_bytes = sizeof(int32_t) * UVC_SITEREAD_NCOL * (size_t)n_sites;
    if (!r->has_reads) { memset(counts, 0, counts_bytes); *n_rows = 0; return 0; }   // set_reads with zero reads: nothing to launch
    const int64_t n_alns = r->R.n_alns, scratch_ints = uvc_sitereads_scratch_ints(n_alns, n_sites), rows_at = uvc_sitereads_rows_at(n_alns, n_sites);
    ReportLayout L0;
    const size_t o_sites = L0.take(sizeof(int32_t) * (size_t)n_sites), o_counts = L0.take(counts_bytes), o_scratch = L0.take(sizeof(int32_t) * (size_t)scratch_ints);
    const size_t head_bytes = 64;   // the page-locked result: the number of items and of rows, then the counts
    int64_t room = 0;   // the rows the buffer as it is has room for behind the fixed pieces, never more than the caller's
    if (row_capacity > 0 && r->d_report.cap > L0.bytes + 128) room = std::min(row_capacity, (int64_t)((r->d_report.cap - L0.bytes - 128) / sizeof(UvcSiteRead)));
    int32_t n = 0;
    int32_t *d_scratch = nullptr; const int32_t *d_sites = nullptr; UvcSiteRead *d_rows = nullptr;
    for (;;) {
        ReportLayout L = L0;
        const size_t o_rows = L.take(sizeof(UvcSiteRead) * (size_t)room);
        { int rc1 = report_begin(r, L, head_bytes + counts_bytes, "site reads", sites, sizeof(int32_t) * (size_t)n_sites); if (rc1) return rc1; }
        d_sites = (const int32_t *)(r->d_report + o_sites); d_scratch = (int32_t *)(r->d_report + o_scratch); d_rows = (UvcSiteRead *)(r->d_report + o_rows);
        int32_t *d_counts = (int32_t *)(r->d_report + o_counts);
        HIP_OK(hipMemsetAsync(d_counts, 0, o_scratch - o_counts + 64, r->stream));   // the counts and the number of items at the head of the scratch
        // with profiling on, two more entries of uvcgpu_region_kernel_times (accumulate starts the list anew); a call that counts twice adds two
        const int pi = uvc_prof_begin(&r->prof, "k_sitereads_count", r->stream);
        uvc_launch_sitereads_count(&r->R, &r->W, d_sites, (int)n_sites, req, d_counts, d_scratch, r->stream);
        uvc_prof_end(&r->prof, pi, r->stream);
        HIP_OK(hipGetLastError());
        char *h = r->h_report;
        HIP_OK(hipMemcpyAsync(h, d_scratch, sizeof(int64_t), hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipMemcpyAsync(h + 8, d_scratch + rows_at, sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipMemcpyAsync(h + head_bytes, d_counts, counts_bytes, hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipStreamSynchronize(r->stream));
        int64_t n_items; memcpy(&n_items, h, sizeof n_items); memcpy(&n, h + 8, sizeof n);
        if (n_items > INT32_MAX) return fail(UVCGPU_EUNSUPPORTED, "site_reads: " + std::to_string(n_items) + " (alignment, site) candidates, more than one call takes (2^31 - 1): pass the sites in several calls");
        if (n <= room || n > row_capacity) break;
        room = n;
    }
    *n_rows = n;
    memcpy(counts, (const char *)r->h_report + head_bytes, counts_bytes);
    if (n > row_capacity) return fail(UVCGPU_ENOMEM, "site_reads: " + std::to_string(n) + " rows, room for " + std::to_string(row_capacity));
    if (n == 0) return 0;
    const size_t out_bytes = sizeof(UvcSiteRead) * (size_t)n;
    { int rc1 = report_buffers(r, 0, out_bytes, "site reads"); if (rc1) return rc1; }
    const int pi = uvc_prof_begin(&r->prof, "k_sitereads_write", r->stream);
    uvc_launch_sitereads_write(&r->R, &r->W, d_sites, (int)n_sites, req, d_scratch, d_rows, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    return report_result(r, d_rows, rows, out_bytes, false);
}
int uvcgpu_region_site_reads(uvcgpu_region_t *r, const int32_t *sites, int64_t n_sites, const UvcSiteReadsRequest *req, int32_t *counts, UvcSiteRead *rows, int64_t row_capacity, int64_t *n_rows) {
    return guarded("uvcgpu_region_site_reads", [&] { return uvcgpu_region_site_reads_impl(r, sites, n_sites, req, counts, rows, row_capacity, n_rows); });
}
const char *uvcgpu_site_read_kind_name(int32_t kind) { return uvc_sitereads_kind_name(kind); }

// ---- clipped-read breakpoint sites of ranges (uvc_clipsites.hip): [table] [totals] [per-position counts: cnt[npos][2], spanning[npos]]
// [site keys] [rows, `room_sites` of them] [scan scratch ints] [event rows, `room_reads` of them] ----
// The read columns, CIGARs and bases belong to the reads of the handle: the legality is that of uvcgpu_region_read_profile.
// Sizes first in one pass: no call has more sites than min(2 positions of its ranges, 2 alignments) or more event rows than 2 alignments,
// so the room is the caller's capacity capped by those bounds, and a call whose room is too small is one whose capacity is.  The find
// stage runs, the host reads the totals and the two numbers in one wait, and only a call with enough room launches the fill.
static int uvcgpu_region_clip_sites_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcClipSitesRequest *req, int64_t *totals, int64_t *sites, int64_t site_capacity,
                                         int64_t *n_sites, UvcClipRead *reads, int64_t read_capacity, int64_t *n_reads) {
    { int rc1 = report_guard(r, "clip_sites", nullptr, "reads"); if (rc1) return rc1; }
    if (!ranges || !req || !totals || !n_sites || !n_reads) return fail(UVCGPU_EINVAL, "clip_sites: ranges, req, totals, n_sites and n_reads must not be NULL");
    if (req->min_mapq < 0 || req->min_mapq > 255) return fail(UVCGPU_EINVAL, "clip_sites: min_mapq " + std::to_string(req->min_mapq) + " is outside 0..255");
    if (req->min_clip < 1) return fail(UVCGPU_EINVAL, "clip_sites: min_clip " + std::to_string(req->min_clip) + " must be at least 1");
    if (req->min_reads < 1) return fail(UVCGPU_EINVAL, "clip_sites: min_reads " + std::to_string(req->min_reads) + " must be at least 1");
    if (req->want_reads < 0 || req->want_reads > 1) return fail(UVCGPU_EINVAL, "clip_sites: want_reads " + std::to_string(req->want_reads) + " is outside 0..1");
    if (site_capacity < 0) return fail(UVCGPU_EINVAL, "clip_sites: site_capacity " + std::to_string(site_capacity) + " is negative");
    if (read_capacity < 0) return fail(UVCGPU_EINVAL, "clip_sites: read_capacity " + std::to_string(read_capacity) + " is negative");
    if (!sites && site_capacity > 0) return fail(UVCGPU_EINVAL, "clip_sites: sites is NULL with site_capacity " + std::to_string(site_capacity));
    if (!reads && read_capacity > 0) return fail(UVCGPU_EINVAL, "clip_sites: reads is NULL with read_capacity " + std::to_string(read_capacity));
    { int rc1 = range_count("clip_sites", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "clip_sites", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const size_t totals_bytes = sizeof(int64_t) * UVC_CLIPSITE_NTOTAL, row_bytes = sizeof(int64_t) * UVC_CLIPSITE_ROW;
    if (!r->has_reads) { memset(totals, 0, totals_bytes); *n_sites = 0; *n_reads = 0; return 0; }   // set_reads with zero reads: nothing to launch
    const int64_t n_alns = r->R.n_alns, most_sites = std::min<int64_t>(2 * n_total, 2 * n_alns);
    const int64_t room_sites = std::min(site_capacity, most_sites), room_reads = req->want_reads ? std::min<int64_t>(read_capacity, 2 * n_alns) : 0;
    const int64_t sites_at = uvc_clipsites_sites_at(n_alns, r->npos), reads_at = uvc_clipsites_reads_at(n_alns, r->npos);
    ReportLayout L;
    const size_t o_tab = L.take(sizeof(UvcRangeRow) * tab.size()), o_totals = L.take(totals_bytes), o_pos = L.take(sizeof(int32_t) * (size_t)uvc_clipsites_pos_ints(r->npos));
    const size_t o_keys = L.take(sizeof(int32_t) * (size_t)most_sites), o_rows = L.take(row_bytes * (size_t)room_sites);
    const size_t o_scratch = L.take(sizeof(int32_t) * (size_t)uvc_clipsites_scratch_ints(n_alns, r->npos)), o_reads = L.take(sizeof(UvcClipRead) * (size_t)room_reads);
    const size_t head_bytes = 128;   // the page-locked head: the totals, the number of sites and of event rows
    { int rc1 = report_begin(r, L, std::max(head_bytes, row_bytes * (size_t)room_sites + sizeof(UvcClipRead) * (size_t)room_reads), "clip sites", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
    const UvcRangeRow *d_tab = (const UvcRangeRow *)(r->d_report + o_tab);
    long long *d_totals = (long long *)(r->d_report + o_totals), *d_rows = (long long *)(r->d_report + o_rows);
    int32_t *d_pos = (int32_t *)(r->d_report + o_pos), *d_keys = (int32_t *)(r->d_report + o_keys), *d_scratch = (int32_t *)(r->d_report + o_scratch);
    UvcClipRead *d_reads = (UvcClipRead *)(r->d_report + o_reads);
    HIP_OK(hipMemsetAsync(d_totals, 0, o_keys - o_totals, r->stream));   // the totals and the per-position counts
    // with profiling on, two more entries of uvcgpu_region_kernel_times (accumulate starts the list anew)
    int pi = uvc_prof_begin(&r->prof, "k_clipsites_find", r->stream);
    uvc_launch_clipsites_find(&r->R, &r->W, d_tab, (int)n_ranges, req, d_totals, d_pos, d_keys, most_sites, d_scratch, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    HIP_OK(hipGetLastError());
    char *h = r->h_report;
    HIP_OK(hipMemcpyAsync(h, d_totals, totals_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipMemcpyAsync(h + totals_bytes, d_scratch + sites_at, sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipMemcpyAsync(h + totals_bytes + 4, d_scratch + reads_at, sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipStreamSynchronize(r->stream));
    int32_t ns = 0, nr = 0;
    memcpy(totals, h, totals_bytes); memcpy(&ns, h + totals_bytes, sizeof ns); memcpy(&nr, h + totals_bytes + 4, sizeof nr);
    *n_sites = ns; *n_reads = nr;
    if (ns > site_capacity) return fail(UVCGPU_ENOMEM, "clip_sites: " + std::to_string(ns) + " sites, room for " + std::to_string(site_capacity));
    if (req->want_reads && nr > read_capacity) return fail(UVCGPU_ENOMEM, "clip_sites: " + std::to_string(nr) + " event rows, room for " + std::to_string(read_capacity));
    if (ns == 0) return 0;
    const size_t sites_bytes = row_bytes * (size_t)ns, reads_bytes = req->want_reads ? sizeof(UvcClipRead) * (size_t)nr : 0;
    HIP_OK(hipMemsetAsync(d_rows, 0, sites_bytes, r->stream));
    pi = uvc_prof_begin(&r->prof, "k_clipsites_fill", r->stream);
    uvc_launch_clipsites_fill(&r->R, &r->W, d_tab, (int)n_ranges, req, d_pos, d_keys, ns, d_scratch, d_rows, req->want_reads ? d_reads : nullptr, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, d_rows, sites_bytes, hipMemcpyDeviceToHost, r->stream));
    if (reads_bytes) HIP_OK(hipMemcpyAsync(h + sites_bytes, d_reads, reads_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipStreamSynchronize(r->stream));
    memcpy(sites, h, sites_bytes);
    if (reads_bytes) memcpy(reads, h + sites_bytes, reads_bytes);
    return 0;
}
int uvcgpu_region_clip_sites(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcClipSitesRequest *req, int64_t *totals, int64_t *sites, int64_t site_capacity, int64_t *n_sites,
                             UvcClipRead *reads, int64_t read_capacity, int64_t *n_reads) {
    return guarded("uvcgpu_region_clip_sites", [&] { return uvcgpu_region_clip_sites_impl(r, ranges, n_ranges, req, totals, sites, site_capacity, n_sites, reads, read_capacity, n_reads); });
}
const char *uvcgpu_clip_site_section_name(int32_t id) { return uvc_clipsites_name(id); }

// ---- clip-site junctions (uvc_clipjunc.hip): [the caller's site rows] [the mate lists] [packed reference] [its "not a base"
// mask] [query rows] [best keys] [hist] [junction rows] ----
// The call reads the reference of the region and the caller's rows: legal from create / reset on, whatever was done with reads, planes or
// scores since.  The rows and the two mate lists (the plane indices of the LEFT sites ascending, then those of the RIGHT sites, and the row
// each belongs to) go up through the staging buffer.  The totals are sums over the returned rows.
namespace {
enum {   // the first words of the sections the host reads: of a site row and of a junction row
#define UVC_CLIPSITE(name, first, words) CS_AT_##name = first,
#include "uvc_clipsites.def"
#undef UVC_CLIPSITE
#define UVC_CLIPJUNC(name, first, words) CJ_AT_##name = first,
#include "uvc_clipjunc.def"
#undef UVC_CLIPJUNC
};
}
static int uvcgpu_region_clip_junctions_impl(uvcgpu_region_t *r, const int64_t *sites, int64_t n_sites, const UvcClipJunctionsRequest *req, int64_t *junctions, int64_t *totals) {
    if (!r) return fail(UVCGPU_EINVAL, "clip_junctions: null region");
    if (!req || !totals) return fail(UVCGPU_EINVAL, "clip_junctions: req and totals must not be NULL");
    if (n_sites < 0) return fail(UVCGPU_EINVAL, "clip_junctions: n_sites " + std::to_string(n_sites) + " is negative");
    if (n_sites > 0 && (!sites || !junctions)) return fail(UVCGPU_EINVAL, "clip_junctions: sites and junctions must not be NULL");
    if (req->min_votes < 1) return fail(UVCGPU_EINVAL, "clip_junctions: min_votes " + std::to_string(req->min_votes) + " must be at least 1");
    if (req->min_len < 1 || req->min_len > UVC_CLIPSITE_NCONS) return fail(UVCGPU_EINVAL, "clip_junctions: min_len " + std::to_string(req->min_len) + " is outside 1.." + std::to_string((int)UVC_CLIPSITE_NCONS));
    if (req->max_mismatch < 0 || req->max_mismatch >= UVC_CLIPJUNC_NHIST) return fail(UVCGPU_EINVAL, "clip_junctions: max_mismatch " + std::to_string(req->max_mismatch) + " is outside 0.." + std::to_string(UVC_CLIPJUNC_NHIST - 1));
    if (req->max_dist < 0) return fail(UVCGPU_EINVAL, "clip_junctions: max_dist " + std::to_string(req->max_dist) + " is negative");
    if (req->mate_slop < 0) return fail(UVCGPU_EINVAL, "clip_junctions: mate_slop " + std::to_string(req->mate_slop) + " is negative");
    if (n_sites > (INT32_MAX >> 1)) return fail(UVCGPU_EINVAL, "clip_junctions: n_sites " + std::to_string(n_sites) + " is more than one call takes (" + std::to_string(INT32_MAX >> 1) + ")");
    const size_t sites_bytes = sizeof(int64_t) * UVC_CLIPSITE_ROW * (size_t)n_sites, list_bytes = sizeof(int32_t) * (size_t)n_sites, rows_bytes = sizeof(int64_t) * UVC_CLIPJUNC_ROW * (size_t)n_sites;
    int64_t n_left = 0;
    for (int64_t k = 0; k < n_sites; k++) {
        const int64_t *row = sites + k * UVC_CLIPSITE_ROW, pos = row[CS_AT_pos], side = row[CS_AT_side];
        if (pos < r->beg || pos - r->beg >= r->npos) return fail(UVCGPU_EINVAL, "clip_junctions: row " + std::to_string(k) + " has pos " + std::to_string(pos) + ", outside the region [" + std::to_string(r->beg) + ", " + std::to_string(r->end) + ")");
        if (side != UVC_CLIPSITE_LEFT && side != UVC_CLIPSITE_RIGHT) return fail(UVCGPU_EINVAL, "clip_junctions: row " + std::to_string(k) + " has side " + std::to_string(side) + ", neither 0 nor 1");
        const int64_t *prev = row - UVC_CLIPSITE_ROW;
        if (k > 0 && std::make_pair(prev[CS_AT_pos], prev[CS_AT_side]) >= std::make_pair(pos, side))
            return fail(UVCGPU_EINVAL, "clip_junctions: row " + std::to_string(k) + " (" + std::to_string(pos) + ", " + std::to_string(side) + ") is not above row " + std::to_string(k - 1) + ": rows ascend strictly by (pos, side)");
        n_left += (side == UVC_CLIPSITE_LEFT);
    }
    memset(totals, 0, sizeof(int64_t) * UVC_CLIPJUNC_NTOTAL);
    if (n_sites == 0) return 0;
    // the two mate lists: mpos, midx
    std::vector<int32_t> lists(2 * (size_t)n_sites);
    {
        int32_t *mpos = lists.data(), *midx = mpos + n_sites;
        int64_t at[2] = { 0, n_left };
        for (int64_t k = 0; k < n_sites; k++) {
            const int64_t *row = sites + k * UVC_CLIPSITE_ROW;
            const int64_t j = at[row[CS_AT_side]]++;
            mpos[j] = (int32_t)(row[CS_AT_pos] - r->beg); midx[j] = (int32_t)k;
        }
    }
    const size_t ref_bytes = sizeof(uint64_t) * (size_t)uvc_clipjunc_ref_words(r->npos);
    ReportLayout L;
    const size_t o_sites = L.take(sites_bytes), o_lists = L.take(2 * list_bytes), o_ref2 = L.take(ref_bytes), o_inv = L.take(ref_bytes), o_query = L.take((size_t)uvc_clipjunc_query_bytes(n_sites));
    const size_t o_best = L.take(sizeof(uint64_t) * (size_t)n_sites), o_hist = L.take(sizeof(uint32_t) * UVC_CLIPJUNC_NHIST * (size_t)n_sites), o_rows = L.take(rows_bytes);
    { int rc1 = report_buffers(r, L.bytes, rows_bytes, "clip junctions"); if (rc1) return rc1; }
    char *d = r->d_report;
    {   // the rows and the lists through the staging buffer, one piece behind the other (stage_upload: never a copy from the caller's pages)
        size_t at = 0;
        const size_t total = o_ref2;   // (the two pieces lie at the head of the layout, each on a 64-byte boundary, as `at` counts them)
        { int rc1 = stage_upload(r, d + o_sites, sites, sites_bytes, at, total); if (rc1) return rc1; }
        { int rc1 = stage_upload(r, d + o_lists, lists.data(), 2 * list_bytes, at, total); if (rc1) return rc1; }
    }
    const long long *d_sites = (const long long *)(d + o_sites);
    const int32_t *d_mpos = (const int32_t *)(d + o_lists), *d_midx = d_mpos + n_sites;
    unsigned long long *d_ref2 = (unsigned long long *)(d + o_ref2), *d_inv = (unsigned long long *)(d + o_inv), *d_best = (unsigned long long *)(d + o_best);
    unsigned *d_hist = (unsigned *)(d + o_hist);
    void *d_query = d + o_query;
    long long *d_rows = (long long *)(d + o_rows);
    // with profiling on, four more entries of uvcgpu_region_kernel_times (accumulate starts the list anew)
    int pi = uvc_prof_begin(&r->prof, "k_clipjunc_pack", r->stream);
    uvc_launch_clipjunc_pack(&r->R, d_ref2, d_inv, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    pi = uvc_prof_begin(&r->prof, "k_clipjunc_queries", r->stream);
    uvc_launch_clipjunc_queries(&r->R, d_sites, (int)n_sites, req, d_query, d_best, d_hist, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    pi = uvc_prof_begin(&r->prof, "k_clipjunc_search", r->stream);
    uvc_launch_clipjunc_search(&r->R, d_ref2, d_inv, d_query, (int)n_sites, req, d_best, d_hist, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    pi = uvc_prof_begin(&r->prof, "k_clipjunc_finish", r->stream);
    uvc_launch_clipjunc_finish(&r->R, d_query, (int)n_sites, req, d_best, d_hist, d_mpos, d_midx, (int)n_left, d_rows, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    { int rc1 = report_result(r, d_rows, junctions, rows_bytes, false); if (rc1) return rc1; }
    totals[UVC_CLIPJTOTAL_sites] = n_sites;
    for (int64_t k = 0; k < n_sites; k++) {
        const int64_t *row = junctions + k * UVC_CLIPJUNC_ROW;
        totals[UVC_CLIPJTOTAL_searched] += (row[CJ_AT_status] != UVC_CLIPJUNC_NOT_SEARCHED);
        totals[UVC_CLIPJTOTAL_placed] += (row[CJ_AT_status] == UVC_CLIPJUNC_PLACED);
        totals[UVC_CLIPJTOTAL_unique] += (row[CJ_AT_n_best] == 1);
        totals[UVC_CLIPJTOTAL_mated] += (row[CJ_AT_mate] >= 0);
    }
    return 0;
}
int uvcgpu_region_clip_junctions(uvcgpu_region_t *r, const int64_t *sites, int64_t n_sites, const UvcClipJunctionsRequest *req, int64_t *junctions, int64_t *totals) {
    return guarded("uvcgpu_region_clip_junctions", [&] { return uvcgpu_region_clip_junctions_impl(r, sites, n_sites, req, junctions, totals); });
}
const char *uvcgpu_clip_junction_section_name(int32_t id) { return uvc_clipjunc_name(id); }
const char *uvcgpu_clip_class_name(int32_t klass) { return uvc_clipjunc_class_name(klass); }

// ---- clip-site mates (uvc_clipmates.hip): in the report buffer [the site lists] [the mtid column] [site rows] [totals] [per-site ints];
// what depends on the number of witnesses and of clusters comes from a pool of this call ----
// The read columns belong to the reads of the handle: the legality is that of uvcgpu_region_clip_sites.  The lists (the absolute positions
// of the LEFT sites ascending, then those of the RIGHT sites, and the row each belongs to) and the caller's mtid go up through the staging
// buffer.  Sizes first: the host waits behind the count (the four totals, the witnesses, the rank blocks), behind the cut (the clusters)
// and behind the reduce (the site rows, the kept clusters); only a call with enough room copies cluster and witness rows.
static int uvcgpu_region_clip_mates_impl(uvcgpu_region_t *r, const int64_t *sites, int64_t n_sites, const int32_t *mtid, const UvcClipMatesRequest *req, int64_t *totals, int64_t *site_rows,
                                         int64_t *clusters, int64_t cluster_capacity, int64_t *n_clusters, UvcClipMate *reads, int64_t read_capacity, int64_t *n_reads) {
    { int rc1 = report_guard(r, "clip_mates", nullptr, "reads"); if (rc1) return rc1; }
    if (!req || !totals || !n_clusters || !n_reads) return fail(UVCGPU_EINVAL, "clip_mates: req, totals, n_clusters and n_reads must not be NULL");
    if (n_sites < 0) return fail(UVCGPU_EINVAL, "clip_mates: n_sites " + std::to_string(n_sites) + " is negative");
    if (n_sites > 0 && (!sites || !site_rows)) return fail(UVCGPU_EINVAL, "clip_mates: sites and site_rows must not be NULL");
    if (req->tid < 0) return fail(UVCGPU_EINVAL, "clip_mates: tid " + std::to_string(req->tid) + " is negative");
    if (req->min_mapq < 0 || req->min_mapq > 255) return fail(UVCGPU_EINVAL, "clip_mates: min_mapq " + std::to_string(req->min_mapq) + " is outside 0..255");
    if (req->window < 1) return fail(UVCGPU_EINVAL, "clip_mates: window " + std::to_string(req->window) + " must be at least 1");
    if (req->overhang < 0) return fail(UVCGPU_EINVAL, "clip_mates: overhang " + std::to_string(req->overhang) + " is negative");
    if (req->min_dist < 1) return fail(UVCGPU_EINVAL, "clip_mates: min_dist " + std::to_string(req->min_dist) + " must be at least 1");
    if (req->max_gap < 0) return fail(UVCGPU_EINVAL, "clip_mates: max_gap " + std::to_string(req->max_gap) + " is negative");
    if (req->min_pairs < 1) return fail(UVCGPU_EINVAL, "clip_mates: min_pairs " + std::to_string(req->min_pairs) + " must be at least 1");
    if (req->want_reads < 0 || req->want_reads > 1) return fail(UVCGPU_EINVAL, "clip_mates: want_reads " + std::to_string(req->want_reads) + " is outside 0..1");
    if (cluster_capacity < 0) return fail(UVCGPU_EINVAL, "clip_mates: cluster_capacity " + std::to_string(cluster_capacity) + " is negative");
    if (read_capacity < 0) return fail(UVCGPU_EINVAL, "clip_mates: read_capacity " + std::to_string(read_capacity) + " is negative");
    if (!clusters && cluster_capacity > 0) return fail(UVCGPU_EINVAL, "clip_mates: clusters is NULL with cluster_capacity " + std::to_string(cluster_capacity));
    if (!reads && read_capacity > 0) return fail(UVCGPU_EINVAL, "clip_mates: reads is NULL with read_capacity " + std::to_string(read_capacity));
    if (n_sites > (INT32_MAX >> 1)) return fail(UVCGPU_EINVAL, "clip_mates: n_sites " + std::to_string(n_sites) + " is more than one call takes (" + std::to_string(INT32_MAX >> 1) + ")");
    int64_t n_left = 0;
    for (int64_t k = 0; k < n_sites; k++) {
        const int64_t *row = sites + k * UVC_CLIPSITE_ROW, pos = row[CS_AT_pos], side = row[CS_AT_side];
        if (pos < r->beg || pos - r->beg >= r->npos) return fail(UVCGPU_EINVAL, "clip_mates: row " + std::to_string(k) + " has pos " + std::to_string(pos) + ", outside the region [" + std::to_string(r->beg) + ", " + std::to_string(r->end) + ")");
        if (side != UVC_CLIPSITE_LEFT && side != UVC_CLIPSITE_RIGHT) return fail(UVCGPU_EINVAL, "clip_mates: row " + std::to_string(k) + " has side " + std::to_string(side) + ", neither 0 nor 1");
        const int64_t *prev = row - UVC_CLIPSITE_ROW;
        if (k > 0 && std::make_pair(prev[CS_AT_pos], prev[CS_AT_side]) >= std::make_pair(pos, side))
            return fail(UVCGPU_EINVAL, "clip_mates: row " + std::to_string(k) + " (" + std::to_string(pos) + ", " + std::to_string(side) + ") is not above row " + std::to_string(k - 1) + ": rows ascend strictly by (pos, side)");
        n_left += (side == UVC_CLIPSITE_LEFT);
    }
    const size_t totals_bytes = sizeof(int64_t) * UVC_CLIPMATE_NTOTAL, rows_bytes = sizeof(int64_t) * UVC_CLIPMATE_SITE_ROW * (size_t)n_sites;
    if (n_sites == 0 || !r->has_reads) {   // no site, or set_reads with zero reads: nothing to launch
        memset(totals, 0, totals_bytes);
        if (n_sites) memset(site_rows, 0, rows_bytes);
        for (int64_t k = 0; k < n_sites; k++) site_rows[k * UVC_CLIPMATE_SITE_ROW + UVC_CLIPMSITE_site] = k;
        *n_clusters = 0; *n_reads = 0;
        return 0;
    }
    std::vector<int32_t> lists(2 * (size_t)n_sites);
    {
        int32_t *spos = lists.data(), *sidx = spos + n_sites;
        int64_t at[2] = { 0, n_left };
        for (int64_t k = 0; k < n_sites; k++) {
            const int64_t *row = sites + k * UVC_CLIPSITE_ROW;
            const int64_t j = at[row[CS_AT_side]]++;
            spos[j] = (int32_t)row[CS_AT_pos]; sidx[j] = (int32_t)k;
        }
    }
    const int64_t n_alns = r->R.n_alns, site_ints = uvc_clipmates_site_ints(n_sites);
    const size_t list_bytes = sizeof(int32_t) * 2 * (size_t)n_sites, mtid_bytes = mtid ? sizeof(int32_t) * (size_t)n_alns : 0;
    ReportLayout L;
    const size_t o_lists = L.take(list_bytes), o_mtid = L.take(mtid_bytes), o_rows = L.take(rows_bytes), o_totals = L.take(totals_bytes), o_ints = L.take(sizeof(int32_t) * (size_t)site_ints);
    const size_t head_bytes = 128;   // the page-locked head: the totals and the numbers the host waits for
    { int rc1 = report_buffers(r, L.bytes, head_bytes + rows_bytes, "clip mates"); if (rc1) return rc1; }
    char *d = r->d_report, *h = r->h_report;
    {
        size_t at = 0;
        const size_t total = o_rows;   // (the two pieces lie at the head of the layout, each on a 64-byte boundary, as `at` counts them)
        { int rc1 = stage_upload(r, d + o_lists, lists.data(), list_bytes, at, total); if (rc1) return rc1; }
        if (mtid) { int rc1 = stage_upload(r, d + o_mtid, mtid, mtid_bytes, at, total); if (rc1) return rc1; }
    }
    const UvcClipMateLists lists_dev{ (const int32_t *)(d + o_lists), (const int32_t *)(d + o_lists) + n_sites, mtid ? (const int32_t *)(d + o_mtid) : nullptr, (int)n_sites, (int)n_left };
    long long *d_rows = (long long *)(d + o_rows), *d_totals = (long long *)(d + o_totals);
    int32_t *d_ints = (int32_t *)(d + o_ints);
    HIP_OK(hipMemsetAsync(d_rows, 0, L.bytes - o_rows, r->stream));   // the site rows, the totals and the per-site ints
    // with profiling on, up to five more entries of uvcgpu_region_kernel_times (accumulate starts the list anew)
    int pi = uvc_prof_begin(&r->prof, "k_clipmates_count", r->stream);
    uvc_launch_clipmates_count(&r->W, n_alns, &lists_dev, req, d_rows, d_totals, d_ints, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, d_totals, totals_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipMemcpyAsync(h + totals_bytes, uvc_clipmates_n_witnesses_at(d_ints, n_sites), sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipMemcpyAsync(h + totals_bytes + 4, uvc_clipmates_n_rank_blocks_at(d_ints, n_sites), sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipMemcpyAsync(h + head_bytes, d_rows, rows_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipStreamSynchronize(r->stream));
    int64_t tot[UVC_CLIPMATE_NTOTAL];
    int32_t n_wit = 0, n_blocks = 0, n_clus = 0, n_kept = 0;
    memcpy(tot, h, totals_bytes); memcpy(&n_wit, h + totals_bytes, sizeof n_wit); memcpy(&n_blocks, h + totals_bytes + 4, sizeof n_blocks);
    if (tot[UVC_CLIPMTOTAL_facing] > INT32_MAX) return fail(UVCGPU_EUNSUPPORTED, "clip_mates: " + std::to_string(tot[UVC_CLIPMTOTAL_facing]) + " facing (alignment, site) items, more than one call takes (2^31 - 1): pass the sites in several calls");
    Pool tmp(r);
    unsigned long long *d_key = nullptr, *d_okey = nullptr; int32_t *d_wit = nullptr, *d_clus = nullptr; long long *d_crow = nullptr, *d_out = nullptr; UvcClipMate *d_reads = nullptr;
    if (n_wit > 0) {
        const int64_t wit_ints = uvc_clipmates_witness_ints(n_wit);
        if (!tmp.get(&d_key, (size_t)n_wit) || !tmp.get(&d_okey, (size_t)n_wit) || !tmp.get(&d_wit, (size_t)wit_ints)) return fail(UVCGPU_ENOMEM, "clip_mates: hipMalloc(" + std::to_string(n_wit) + " witnesses) failed");
        pi = uvc_prof_begin(&r->prof, "k_clipmates_scatter", r->stream);
        uvc_launch_clipmates_scatter(&r->W, n_alns, &lists_dev, req, d_ints, n_wit, d_key, d_wit, r->stream);
        uvc_prof_end(&r->prof, pi, r->stream);
        pi = uvc_prof_begin(&r->prof, "k_clipmates_rank", r->stream);
        uvc_launch_clipmates_rank(&lists_dev, d_ints, n_wit, n_blocks, d_key, d_okey, d_wit, r->stream);
        uvc_prof_end(&r->prof, pi, r->stream);
        pi = uvc_prof_begin(&r->prof, "k_clipmates_cut", r->stream);
        uvc_launch_clipmates_cut(&lists_dev, req, d_ints, n_wit, d_okey, d_wit, r->stream);
        uvc_prof_end(&r->prof, pi, r->stream);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h, uvc_clipmates_n_clusters_at(d_wit, n_wit), sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipStreamSynchronize(r->stream));
        memcpy(&n_clus, h, sizeof n_clus);   // (at least 1: the first witness begins a cluster)
        const int64_t clus_ints = uvc_clipmates_cluster_ints(n_clus);
        const size_t crow_bytes = sizeof(int64_t) * UVC_CLIPMATE_ROW * (size_t)n_clus;
        if (!tmp.get(&d_crow, (size_t)UVC_CLIPMATE_ROW * n_clus) || !tmp.get(&d_out, (size_t)UVC_CLIPMATE_ROW * n_clus) || !tmp.get(&d_clus, (size_t)clus_ints) || (req->want_reads && !tmp.get(&d_reads, (size_t)n_wit)))
            return fail(UVCGPU_ENOMEM, "clip_mates: hipMalloc(" + std::to_string(n_clus) + " clusters) failed");
        HIP_OK(hipMemsetAsync(d_crow, 0, crow_bytes, r->stream));
        pi = uvc_prof_begin(&r->prof, "k_clipmates_reduce", r->stream);
        uvc_launch_clipmates_reduce(&r->W, &lists_dev, req, n_wit, n_clus, d_okey, d_wit, d_crow, d_rows, d_out, d_reads, d_clus, r->stream);
        uvc_prof_end(&r->prof, pi, r->stream);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h, uvc_clipmates_n_kept_at(d_clus, n_clus), sizeof(int32_t), hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipMemcpyAsync(h + head_bytes, d_rows, rows_bytes, hipMemcpyDeviceToHost, r->stream));
        HIP_OK(hipStreamSynchronize(r->stream));
        memcpy(&n_kept, h, sizeof n_kept);
    }
    memcpy(site_rows, h + head_bytes, rows_bytes);
    tot[UVC_CLIPMTOTAL_clusters] = n_clus; tot[UVC_CLIPMTOTAL_clusters_kept] = n_kept; tot[UVC_CLIPMTOTAL_sites_kept] = 0;
    for (int64_t k = 0; k < n_sites; k++) {
        int64_t *row = site_rows + k * UVC_CLIPMATE_SITE_ROW;
        row[UVC_CLIPMSITE_site] = k;
        row[UVC_CLIPMSITE_facing] = row[UVC_CLIPMSITE_concordant] + row[UVC_CLIPMSITE_other_contig] + row[UVC_CLIPMSITE_same_strand] + row[UVC_CLIPMSITE_far];   // (the device adds the class counters alone)
        tot[UVC_CLIPMTOTAL_sites_kept] += (site_rows[k * UVC_CLIPMATE_SITE_ROW + UVC_CLIPMSITE_clusters_kept] > 0);
    }
    memcpy(totals, tot, totals_bytes);
    *n_clusters = n_kept; *n_reads = n_wit;
    if (n_kept > cluster_capacity) return fail(UVCGPU_ENOMEM, "clip_mates: " + std::to_string(n_kept) + " kept clusters, room for " + std::to_string(cluster_capacity));
    if (req->want_reads && n_wit > read_capacity) return fail(UVCGPU_ENOMEM, "clip_mates: " + std::to_string(n_wit) + " witness rows, room for " + std::to_string(read_capacity));
    const size_t out_bytes = sizeof(int64_t) * UVC_CLIPMATE_ROW * (size_t)n_kept, reads_bytes = req->want_reads ? sizeof(UvcClipMate) * (size_t)n_wit : 0;
    if (out_bytes + reads_bytes == 0) return 0;
    { int rc1 = report_buffers(r, 0, out_bytes + reads_bytes, "clip mates"); if (rc1) return rc1; }
    h = r->h_report;
    if (out_bytes) HIP_OK(hipMemcpyAsync(h, d_out, out_bytes, hipMemcpyDeviceToHost, r->stream));
    if (reads_bytes) HIP_OK(hipMemcpyAsync(h + out_bytes, d_reads, reads_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_OK(hipStreamSynchronize(r->stream));
    if (out_bytes) memcpy(clusters, h, out_bytes);
    if (reads_bytes) memcpy(reads, h + out_bytes, reads_bytes);
    return 0;
}
int uvcgpu_region_clip_mates(uvcgpu_region_t *r, const int64_t *sites, int64_t n_sites, const int32_t *mtid, const UvcClipMatesRequest *req, int64_t *totals, int64_t *site_rows,
                             int64_t *clusters, int64_t cluster_capacity, int64_t *n_clusters, UvcClipMate *reads, int64_t read_capacity, int64_t *n_reads) {
    return guarded("uvcgpu_region_clip_mates", [&] { return uvcgpu_region_clip_mates_impl(r, sites, n_sites, mtid, req, totals, site_rows, clusters, cluster_capacity, n_clusters, reads, read_capacity, n_reads); });
}
const char *uvcgpu_clip_mate_site_name(int32_t id) { return uvc_clipmates_site_name(id); }
const char *uvcgpu_clip_mate_cluster_name(int32_t id) { return uvc_clipmates_cluster_name(id); }
const char *uvcgpu_clip_mate_class_name(int32_t klass) { return uvc_clipmates_class_name(klass); }

// ---- callable-region intervals of ranges (uvc_callable.hip): [table] [block counts] [mask bytes] [runs, one per position at worst] ----
// Sizes first: the count and the scan run, the host reads the number of runs (4 bytes), and only a call with enough room launches the emit
// and copies 16 bytes per run.
static int uvcgpu_region_callable_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcCallableRequest *req, UvcCallableRun *runs, int64_t run_capacity, int64_t *n_runs) {
    { int rc1 = report_guard(r, "callable", "classify"); if (rc1) return rc1; }
    if (!ranges || !req || !n_runs) return fail(UVCGPU_EINVAL, "callable: ranges, req and n_runs must not be NULL");
    if (run_capacity < 0) return fail(UVCGPU_EINVAL, "callable: run_capacity " + std::to_string(run_capacity) + " is negative");
    if (!runs && run_capacity > 0) return fail(UVCGPU_EINVAL, "callable: runs is NULL with run_capacity " + std::to_string(run_capacity));
    for (int32_t k = 0; k < UVC_NCOV; k++)
        if (req->min_depth[k] < 0) return fail(UVCGPU_EINVAL, std::string("callable: min_depth[") + uvc_coverage_name(k) + "] is negative (" + std::to_string(req->min_depth[k]) + ")");
    if (req->max_aDP < 0) return fail(UVCGPU_EINVAL, "callable: max_aDP is negative (" + std::to_string(req->max_aDP) + ")");
    { int rc1 = range_count("callable", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "callable", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const int64_t n_blocks = uvc_callable_blocks(n_total);
    ReportLayout L;
    const size_t o_tab = L.take(sizeof(UvcRangeRow) * tab.size()), o_blocks = L.take(sizeof(int32_t) * (size_t)(n_blocks + 1)), o_mask = L.take((size_t)n_total);
    const size_t o_runs = L.take(sizeof(UvcCallableRun) * (size_t)n_total);   // every position can be its own run
    { int rc1 = report_begin(r, L, 64, "callable runs", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
    const UvcRangeRow *d_tab = (const UvcRangeRow *)(r->d_report + o_tab);
    int *d_blocks = (int *)(r->d_report + o_blocks);
    unsigned char *d_mask = (unsigned char *)(r->d_report + o_mask);
    UvcCallableRun *d_runs = (UvcCallableRun *)(r->d_report + o_runs);
    // with profiling on, two more entries of uvcgpu_region_kernel_times (accumulate starts the list anew): the host reads the count between them
    int pi = uvc_prof_begin(&r->prof, "k_callable_count", r->stream);
    uvc_launch_callable_count(&r->R, d_tab, (int)n_ranges, n_total, req, d_mask, d_blocks, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    int32_t n = 0;
    { int rc1 = report_result(r, d_blocks + n_blocks, &n, sizeof(int32_t), true); if (rc1) return rc1; }
    *n_runs = n;
    if (n > run_capacity) return fail(UVCGPU_ENOMEM, "callable: " + std::to_string(n) + " runs, room for " + std::to_string(run_capacity));
    const size_t out_bytes = sizeof(UvcCallableRun) * (size_t)n;
    { int rc1 = report_buffers(r, 0, out_bytes, "callable runs"); if (rc1) return rc1; }
    pi = uvc_prof_begin(&r->prof, "k_callable_emit", r->stream);
    uvc_launch_callable_emit(&r->R, d_tab, (int)n_ranges, n_total, d_mask, d_blocks, d_runs, r->stream);
    uvc_prof_end(&r->prof, pi, r->stream);
    return report_result(r, d_runs, runs, out_bytes, true);
}
int uvcgpu_region_callable(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcCallableRequest *req, UvcCallableRun *runs, int64_t run_capacity, int64_t *n_runs) {
    return guarded("uvcgpu_region_callable", [&] { return uvcgpu_region_callable_impl(r, ranges, n_ranges, req, runs, run_capacity, n_runs); });
}
const char *uvcgpu_callable_bit_name(int32_t bit) { return uvc_callable_name(bit); }

// ---- microsatellite loci of ranges (uvc_msi.hip): [table] [block counts] [head list, `room` ints] [rows, `room` x UVC_MSI_ROW ints] ----
// Sizes first, in one pass where the buffer allows: every kernel is launched with the room the device buffer has (at most the caller's),
// the kernels read the number of loci on the device, and the host reads it (4 bytes) when all have run.  A call whose room was too small
// for loci the caller has room for lays the buffer out for that number and runs once more; a call without room runs the count alone.
static int uvcgpu_region_msi_impl(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcMsiRequest *req, int32_t *loci, int64_t locus_capacity, int64_t *n_loci) {
    { int rc1 = report_guard(r, "msi", "search"); if (rc1) return rc1; }
    if (!ranges || !req || !n_loci) return fail(UVCGPU_EINVAL, "msi: ranges, req and n_loci must not be NULL");
    if (locus_capacity < 0) return fail(UVCGPU_EINVAL, "msi: locus_capacity " + std::to_string(locus_capacity) + " is negative");
    if (!loci && locus_capacity > 0) return fail(UVCGPU_EINVAL, "msi: loci is NULL with locus_capacity " + std::to_string(locus_capacity));
    if (req->min_tracklen < 1) return fail(UVCGPU_EINVAL, "msi: min_tracklen " + std::to_string(req->min_tracklen) + " must be at least 1");
    if (req->min_units < 1) return fail(UVCGPU_EINVAL, "msi: min_units " + std::to_string(req->min_units) + " must be at least 1");
    if (req->max_unitlen < 1) return fail(UVCGPU_EINVAL, "msi: max_unitlen " + std::to_string(req->max_unitlen) + " must be at least 1");
    { int rc1 = range_count("msi", n_ranges, INT32_MAX >> 1); if (rc1) return rc1; }
    std::vector<UvcRangeRow> tab; int64_t n_total;
    { int rc1 = range_table(r, "msi", ranges, n_ranges, tab, n_total); if (rc1) return rc1; }
    const int64_t n_blocks = uvc_msi_blocks(n_total);
    const size_t row_bytes = sizeof(int32_t) * UVC_MSI_ROW;
    ReportLayout L0;
    const size_t o_tab = L0.take(sizeof(UvcRangeRow) * tab.size()), o_blocks = L0.take(sizeof(int32_t) * (size_t)(n_blocks + 1));
    // the loci the buffer as it is has room for behind the fixed pieces (never more than the positions of the call, each of which can be a head)
    int64_t room = 0;
    if (locus_capacity > 0 && r->d_report.cap > L0.bytes + 128) room = std::min({ locus_capacity, n_total, (int64_t)((r->d_report.cap - L0.bytes - 128) / (row_bytes + sizeof(int32_t))) });
    // the allele pipeline of the accumulate ran on the side stream: behind it, as gap_tables waits for it (no host wait here)
    if (r->side) HIP_OK(hipStreamWaitEvent(r->stream, r->e_fork2, 0));
    int32_t n = 0;
    int32_t *d_rows = nullptr;
    for (;;) {
        ReportLayout L = L0;
        const size_t o_heads = L.take(sizeof(int32_t) * (size_t)room), o_rows = L.take(row_bytes * (size_t)room);
        { int rc1 = report_begin(r, L, 64, "msi loci", tab.data(), sizeof(UvcRangeRow) * tab.size()); if (rc1) return rc1; }
        int *d_blocks = (int *)(r->d_report + o_blocks);
        d_rows = (int32_t *)(r->d_report + o_rows);
        if (room) HIP_OK(hipMemsetAsync(d_rows, 0, row_bytes * (size_t)room, r->stream));
        // with profiling on, one more entry of uvcgpu_region_kernel_times (accumulate starts the list anew); a call that runs twice adds two
        const int pi = uvc_prof_begin(&r->prof, "k_msi", r->stream);
        uvc_launch_msi(&r->R, (const UvcRangeRow *)(r->d_report + o_tab), (int)n_ranges, n_total, req, d_blocks, (int32_t *)(r->d_report + o_heads), d_rows, room, r->stream);
        uvc_prof_end(&r->prof, pi, r->stream);
        { int rc1 = report_result(r, d_blocks + n_blocks, &n, sizeof(int32_t), true); if (rc1) return rc1; }
        if (n <= room || n > locus_capacity) break;
        room = n;
    }
    *n_loci = n;
    if (n > locus_capacity) return fail(UVCGPU_ENOMEM, "msi: " + std::to_string(n) + " loci, room for " + std::to_string(locus_capacity));
    if (n == 0) return 0;
    const size_t out_bytes = row_bytes * (size_t)n;
    { int rc1 = report_buffers(r, 0, out_bytes, "msi loci"); if (rc1) return rc1; }
    return report_result(r, d_rows, loci, out_bytes, true);
}
int uvcgpu_region_msi(uvcgpu_region_t *r, const UvcCoverageRange *ranges, int64_t n_ranges, const UvcMsiRequest *req, int32_t *loci, int64_t locus_capacity, int64_t *n_loci) {
    return guarded("uvcgpu_region_msi", [&] { return uvcgpu_region_msi_impl(r, ranges, n_ranges, req, loci, locus_capacity, n_loci); });
}
const char *uvcgpu_msi_section_name(int32_t id) { return uvc_msi_name(id); }

int uvcgpu_region_create(uvcgpu_region_t **out, const UvcParams *params, int32_t tid, int32_t beg, int32_t end, const char *refseq) { return guarded("uvcgpu_region_create", [&] { return uvcgpu_region_create_impl(out, params, tid, beg, end, refseq); }); }
int uvcgpu_region_reset(uvcgpu_region_t *r, int32_t tid, int32_t beg, int32_t end, const char *refseq) { return guarded("uvcgpu_region_reset", [&] { return uvcgpu_region_reset_impl(r, tid, beg, end, refseq); }); }
int uvcgpu_region_set_reads(uvcgpu_region_t *r, const UvcReadSoA *in) { return guarded("uvcgpu_region_set_reads", [&] { return uvcgpu_region_set_reads_impl(r, in); }); }
int uvcgpu_region_set_reads_device(uvcgpu_region_t *r, const UvcReadSoA *in) { return guarded("uvcgpu_region_set_reads_device", [&] { return uvcgpu_region_set_reads_device_impl(r, in); }); }
int uvcgpu_region_correct_bq(uvcgpu_region_t *r) { return guarded("uvcgpu_region_correct_bq", [&] { return uvcgpu_region_correct_bq_impl(r); }); }
int uvcgpu_region_accumulate(uvcgpu_region_t *r) { return guarded("uvcgpu_region_accumulate", [&] { return uvcgpu_region_accumulate_impl(r); }); }
int uvcgpu_region_fetch(uvcgpu_region_t *r, int32_t g, void *dst, int64_t dst_bytes) { return guarded("uvcgpu_region_fetch", [&] { return uvcgpu_region_fetch_impl(r, g, dst, dst_bytes); }); }
int uvcgpu_region_fetch_columns(uvcgpu_region_t *r, const int32_t *refpos, int64_t n, int64_t *dst) { return guarded("uvcgpu_region_fetch_columns", [&] { return uvcgpu_region_fetch_columns_impl(r, refpos, n, dst); }); }
int uvcgpu_region_indel_alleles(uvcgpu_region_t *r, UvcGapRow *rows, int64_t row_capacity, int64_t *n_rows, uint8_t *seq, int64_t seq_capacity, int64_t *seq_bytes) { return guarded("uvcgpu_region_indel_alleles", [&] { return uvcgpu_region_indel_alleles_impl(r, rows, row_capacity, n_rows, seq, seq_capacity, seq_bytes); }); }
int uvcgpu_region_hap_links(uvcgpu_region_t *r, UvcHapLink *links, int64_t link_capacity, int64_t *n_links, int32_t *muts, int64_t mut_capacity, int64_t *n_mut_ints) { return guarded("uvcgpu_region_hap_links", [&] { return uvcgpu_region_hap_links_impl(r, links, link_capacity, n_links, muts, mut_capacity, n_mut_ints); }); }
int uvcgpu_region_score(uvcgpu_region_t *r, const UvcScoreRequest *req, UvcScoreOut *out) { return guarded("uvcgpu_region_score", [&] { return uvcgpu_region_score_impl(r, req, nullptr, 0, out); }); }
int uvcgpu_region_score_ranges(uvcgpu_region_t *r, const UvcScoreRequest *req, const UvcScoreRange *ranges, int64_t n_ranges, UvcScoreOut *out) {
    return guarded("uvcgpu_region_score_ranges", [&] { return ranges ? uvcgpu_region_score_impl(r, req, ranges, n_ranges, out) : fail(UVCGPU_EINVAL, "score_ranges: ranges is NULL"); });
}

void uvcgpu_region_destroy(uvcgpu_region_t *r) {
    if (!r) return;
    quiesce(r);
    stream_destroy(r);   // an open score stream ends here: its temporaries, row sets and page-locked buffers (the streams are still there)
    for (hipEvent_t *e : r->events()) if (*e) { hipEventDestroy(*e); *e = nullptr; }
    for (hipStream_t *s : r->streams()) if (*s) { hipStreamDestroy(*s); *s = nullptr; }
    delete r;   // the buffers and the pool free what they own (nothing is in flight, and no stream is left to wait for)
    { const hipError_t stale = hipGetLastError(); if (stale != hipSuccess && getenv("UVCGPU_DEBUG")) fprintf(stderr, "[uvcgpu] uvcgpu_region_destroy left HIP error: %s\n", hipGetErrorString(stale)); }
}

}  // extern "C"
