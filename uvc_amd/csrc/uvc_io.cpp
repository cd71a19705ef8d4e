// uvc_io.cpp -- libuvcio.so: BGZF / BAM / BAI and FASTA / .fai readers on zlib (include/uvcio.h).
// Written against the SAM/BAM specification (SAMv1.pdf: section 4.1 BGZF, 4.2 BAM, 5.1-5.3 BAI binning scheme); no htslib.
// Host code only: it feeds the family assignment (include/uvcgroup.h) and uvcgpu_region_set_reads.
#include "uvcio.h"
#include "uvcgpu.h"
#include "uvc_cpus.h"
#include "uvc_inflate_fast.h"

#include <zlib.h>

#include <algorithm>
#include <climits>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <tuple>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <vector>

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
extern "C" const char *uvcio_last_error(void) { return g_err.c_str(); }
namespace { uint32_t block_crc32(const uint8_t *p, size_t n); }
// test entry: one raw DEFLATE stream of known output size through the fast decoder (1 = decoded, 0 = declined)
extern "C" int uvcio_inflate_raw_fast(const void *in, int64_t in_len, void *out, int64_t out_len) {
    return (in && out && in_len >= 0 && out_len >= 0 && uvc_fast_inflate::inflate((const uint8_t *)in, (size_t)in_len, (uint8_t *)out, (size_t)out_len)) ? 1 : 0;
}
namespace { extern void *(*g_col_alloc)(size_t); extern void (*g_col_free)(void *); }
namespace { uvcio_inflate_fn g_inflate_fn = nullptr; void *g_inflate_ctx = nullptr; int32_t g_inflate_min = 0; }
extern "C" void uvcio_set_inflate(uvcio_inflate_fn fn, void *ctx, int32_t min_blocks) { g_inflate_fn = fn; g_inflate_ctx = ctx; g_inflate_min = min_blocks; }
extern "C" void uvcio_set_column_allocator(void *(*alloc_fn)(size_t), void (*free_fn)(void *)) { g_col_alloc = alloc_fn; g_col_free = free_fn; }
extern "C" uint32_t uvcio_crc32(const void *p, int64_t n) { return (p && n > 0) ? block_crc32((const uint8_t *)p, (size_t)n) : 0u; }

namespace {
uint32_t block_crc32(const uint8_t *p, size_t n);   // CRC-32 of a BGZF block (carry-less multiplication where the CPU has it), defined below

inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }

// ---- BGZF: a series of gzip members, each with a 'BC' extra subfield that holds the member size (SAMv1 4.1) ----
struct Bgzf {
    FILE *fp = nullptr;
    int64_t block_addr = -1;        // file offset of the block in `buf`
    int64_t next_addr = 0;          // file offset of the next block
    std::vector<uint8_t> buf;       // inflated block
    size_t off = 0;                 // read position inside buf
    bool eof = false;

    bool load(int64_t addr) {       // reads and inflates the block at file offset addr
        if (fseeko(fp, (off_t)addr, SEEK_SET) != 0) return false;
        uint8_t h[18];
        const size_t got = fread(h, 1, 18, fp);
        if (got == 0) { eof = true; buf.clear(); off = 0; block_addr = addr; next_addr = addr; return true; }
        if (got < 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return false;
        const int xlen = le16(h + 10);
        std::vector<uint8_t> extra((size_t)xlen);
        memcpy(extra.data(), h + 12, std::min(6, xlen));
        if (xlen > 6 && fread(extra.data() + 6, 1, (size_t)xlen - 6, fp) != (size_t)xlen - 6) return false;
        int bsize = -1;
        for (int i = 0; i + 4 <= xlen;) {
            const int slen = le16(extra.data() + i + 2);
            if (extra[i] == 'B' && extra[i + 1] == 'C' && slen == 2) bsize = le16(extra.data() + i + 4);
            i += 4 + slen;
        }
        if (bsize < 0) return false;
        const int cdata = bsize - xlen - 19;   // BSIZE = total block size - 1
        if (cdata < 0) return false;
        if (xlen < 6 && fseeko(fp, (off_t)(addr + 12 + xlen), SEEK_SET) != 0) return false;
        std::vector<uint8_t> comp((size_t)cdata + 8);
        if (fread(comp.data(), 1, comp.size(), fp) != comp.size()) return false;
        const uint32_t isize = le32(comp.data() + cdata + 4);
        buf.assign(isize, 0);
        if (isize) {
            z_stream zs; memset(&zs, 0, sizeof(zs));
            if (inflateInit2(&zs, -15) != Z_OK) return false;
            zs.next_in = comp.data(); zs.avail_in = (uInt)cdata; zs.next_out = buf.data(); zs.avail_out = isize;
            const int rc = inflate(&zs, Z_FINISH);
            inflateEnd(&zs);
            if (rc != Z_STREAM_END || zs.total_out != isize) return false;
            if (block_crc32(buf.data(), isize) != le32(comp.data() + cdata)) return false;
        }
        block_addr = addr; next_addr = addr + bsize + 1; off = 0; eof = false;
        return true;
    }
    bool seek(uint64_t voffset) {   // virtual file offset: coffset << 16 | uoffset
        const int64_t c = (int64_t)(voffset >> 16); const size_t u = (size_t)(voffset & 0xFFFF);
        if (c != block_addr && !load(c)) return false;
        if (u > buf.size()) return false;
        off = u;
        return true;
    }
    uint64_t tell() const { return off < buf.size() || buf.empty() ? (((uint64_t)block_addr << 16) | off) : ((uint64_t)next_addr << 16); }
    // reads n bytes across block boundaries; returns the number read (less than n only at the end of the file)
    size_t read(void *dst, size_t n) {
        size_t done = 0;
        while (done < n) {
            if (off >= buf.size()) {
                if (eof) break;
                if (!load(next_addr)) { eof = true; break; }
                if (buf.empty()) { if (eof) break; continue; }   // an empty block (e.g. the EOF marker): keep going
            }
            const size_t k = std::min(n - done, buf.size() - off);
            memcpy((uint8_t *)dst + done, buf.data() + off, k);
            off += k; done += k;
        }
        return done;
    }
};

// grow-only byte buffer without value initialisation (a fresh std::vector of tens of MB costs its page faults on every query)
struct RawBuf {
    uint8_t *p = nullptr; size_t cap = 0;
    // nullptr when the memory is not there (the old block stays valid and is freed by the destructor)
    uint8_t *need(size_t n) { if (n > cap) { const size_t c2 = n + n / 4 + 4096; uint8_t *q = (uint8_t *)realloc(p, c2); if (!q) return nullptr; p = q; cap = c2; } return p; }
    ~RawBuf() { free(p); }
};
// The two large columns of a batch (one byte per base each) live in memory from the caller's allocator when one is set
// (uvcio_set_column_allocator: uvc1-mi355x hands in uvcgpu_host_alloc, so that uvcgpu_region_set_reads copies them at DMA speed instead of
// through the runtime's pageable staging path, which serialises the worker threads).  Grow-only, no value initialisation, contents kept.
void *(*g_col_alloc)(size_t) = nullptr; void (*g_col_free)(void *) = nullptr;
struct ColBuf {
    uint8_t *p = nullptr; size_t n = 0, cap = 0; bool hooked = false;
    uint8_t *data() { return p; }
    size_t size() const { return n; }
    void clear() { n = 0; }
    void resize(size_t m) {
        if (m > cap) {
            const size_t ncap = m + m / 4 + 65536;
            const bool use_hook = (g_col_alloc && g_col_free);
            uint8_t *q = (uint8_t *)(use_hook ? g_col_alloc(ncap) : malloc(ncap));
            if (!q) throw std::bad_alloc();
            if (n) memcpy(q, p, n);
            release();
            p = q; cap = ncap; hooked = use_hook;
        }
        n = m;
    }
    void release() { if (p) { if (hooked) g_col_free(p); else free(p); } p = nullptr; cap = 0; }
    ~ColBuf() { release(); }
};
struct Chunk { uint64_t beg, end; };
struct RefIndex { std::map<uint32_t, std::vector<Chunk>> bins; std::vector<uint64_t> linear; };

// SAMv1 5.3: bins that may hold alignments overlapping [beg, end)
void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t> &list) {
    --end;
    list.push_back(0);
    for (int64_t k = 1 + (beg >> 26); k <= 1 + (end >> 26); ++k) list.push_back((uint32_t)k);
    for (int64_t k = 9 + (beg >> 23); k <= 9 + (end >> 23); ++k) list.push_back((uint32_t)k);
    for (int64_t k = 73 + (beg >> 20); k <= 73 + (end >> 20); ++k) list.push_back((uint32_t)k);
    for (int64_t k = 585 + (beg >> 17); k <= 585 + (end >> 17); ++k) list.push_back((uint32_t)k);
    for (int64_t k = 4681 + (beg >> 14); k <= 4681 + (end >> 14); ++k) list.push_back((uint32_t)k);
}

}  // namespace

struct uvcio_bam {
    Bgzf z;
    std::vector<std::string> ref_names; std::vector<int64_t> ref_lens;
    uint64_t first_record = 0;      // virtual offset behind the header
    bool has_index = false;
    std::vector<RefIndex> idx;
    // batch storage
    std::vector<int32_t> tid, pos, endpos, mtid, mpos, isize, nm, l_qseq, n_cigar;
    std::vector<uint16_t> flag; std::vector<uint8_t> mapq;
    std::vector<int64_t> seq_off, cigar_off, qname_off;
    ColBuf bases, quals; std::vector<uint32_t> cigars; std::vector<char> qnames;
    RawBuf comp, infl;             // compressed / inflated bytes of the current batch (kept between queries)
};

static bool load_bai(uvcio_bam *b, const std::string &path) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    std::vector<uint8_t> d;
    { uint8_t tmp[1 << 16]; size_t k; while ((k = fread(tmp, 1, sizeof(tmp), fp)) > 0) d.insert(d.end(), tmp, tmp + k); }
    fclose(fp);
    size_t o = 0;
    auto need = [&](size_t n) { return o + n <= d.size(); };
    if (!need(8) || memcmp(d.data(), "BAI\1", 4) != 0) return false;
    const uint32_t n_ref = le32(d.data() + 4); o = 8;
    b->idx.assign(n_ref, RefIndex());
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!need(4)) return false;
        const uint32_t n_bin = le32(d.data() + o); o += 4;
        for (uint32_t i = 0; i < n_bin; i++) {
            if (!need(8)) return false;
            const uint32_t bin = le32(d.data() + o), n_chunk = le32(d.data() + o + 4); o += 8;
            if (!need((size_t)n_chunk * 16)) return false;
            std::vector<Chunk> &v = b->idx[r].bins[bin];
            for (uint32_t c = 0; c < n_chunk; c++) { v.push_back(Chunk{ le64(d.data() + o), le64(d.data() + o + 8) }); o += 16; }
        }
        if (!need(4)) return false;
        const uint32_t n_intv = le32(d.data() + o); o += 4;
        if (!need((size_t)n_intv * 8)) return false;
        for (uint32_t i = 0; i < n_intv; i++) { b->idx[r].linear.push_back(le64(d.data() + o)); o += 8; }
    }
    return true;
}

extern "C" int uvcio_bam_open(uvcio_bam_t **out, const char *path) {
    if (!out || !path) return fail(UVCGPU_EINVAL, "null argument");
    uvcio_bam *b = new uvcio_bam();
    b->z.fp = fopen(path, "rb");
    if (!b->z.fp) { delete b; return fail(UVCGPU_EINVAL, std::string("cannot open ") + path); }
    if (!b->z.load(0) || b->z.eof) { fclose(b->z.fp); delete b; return fail(UVCGPU_EINVAL, std::string(path) + " is not a BGZF file"); }
    uint8_t h[8];
    auto bad = [&](const char *why) { fclose(b->z.fp); delete b; return fail(UVCGPU_EINVAL, std::string(path) + ": " + why); };
    if (b->z.read(h, 8) != 8 || memcmp(h, "BAM\1", 4) != 0) return bad("not a BAM file");
    const uint32_t l_text = le32(h + 4);
    std::vector<uint8_t> text(l_text);
    if (b->z.read(text.data(), l_text) != l_text) return bad("truncated header");
    if (b->z.read(h, 4) != 4) return bad("truncated header");
    const uint32_t n_ref = le32(h);
    for (uint32_t i = 0; i < n_ref; i++) {
        if (b->z.read(h, 4) != 4) return bad("truncated reference list");
        const uint32_t l_name = le32(h);
        std::vector<char> nm(l_name);
        if (b->z.read(nm.data(), l_name) != l_name || b->z.read(h, 4) != 4) return bad("truncated reference list");
        b->ref_names.push_back(std::string(nm.data(), l_name ? l_name - 1 : 0)); b->ref_lens.push_back((int64_t)le32(h));
    }
    b->first_record = b->z.tell();
    std::string p(path);
    b->has_index = load_bai(b, p + ".bai");
    if (!b->has_index && p.size() > 4 && p.substr(p.size() - 4) == ".bam") b->has_index = load_bai(b, p.substr(0, p.size() - 4) + ".bai");
    if (b->has_index && b->idx.size() != b->ref_names.size()) { b->has_index = false; b->idx.clear(); }
    *out = b;
    return 0;
}
extern "C" int32_t uvcio_bam_n_refs(const uvcio_bam_t *b) { return b ? (int32_t)b->ref_names.size() : 0; }
extern "C" const char *uvcio_bam_ref_name(const uvcio_bam_t *b, int32_t tid) { return (b && tid >= 0 && tid < (int32_t)b->ref_names.size()) ? b->ref_names[tid].c_str() : nullptr; }
extern "C" int64_t uvcio_bam_ref_len(const uvcio_bam_t *b, int32_t tid) { return (b && tid >= 0 && tid < (int32_t)b->ref_lens.size()) ? b->ref_lens[tid] : -1; }
extern "C" int uvcio_bam_has_index(const uvcio_bam_t *b) { return b && b->has_index; }
extern "C" void uvcio_bam_close(uvcio_bam_t *b) { if (!b) return; if (b->z.fp) fclose(b->z.fp); delete b; }

// ---- region query: compressed blocks are read in batches, inflated in parallel (BGZF blocks are independent), the records of a
// batch are located by one sequential walk over their size fields and decoded in parallel into the output columns ----
namespace {

struct BlockRef { int64_t addr; uint32_t csize /* whole block */, isize; size_t in_off /* in the batch's compressed buffer */, out_off /* in its inflated buffer */; };
struct RecRef { const uint8_t *r; uint32_t size; int32_t endpos; int64_t base_off, cig_off, name_off; };

int n_threads() {
    static const int n = [] { const char *e = getenv("UVCIO_THREADS"); int v = e ? atoi(e) : uvc_effective_cpus(); return std::max(1, std::min(v, 64)); }();
    return n;
}
// One pool of helper threads for the whole process (UVCIO_THREADS of them, default: the cores the process may use, uvc_cpus.h).
// The command line keeps several tiles in flight, one reader each: with a pool per call every reader owned cores/readers threads and
// those cores idled while its worker was in a single-threaded stage; with one queue the slices of every reader go to whichever core is
// free.  The calling thread works on the queue too until its own slices are done, so a call never waits for a busy pool (and a
// process that forked after the pool was made still finishes, on its own thread).
struct SliceGroup { std::mutex m; std::condition_variable cv; size_t left = 0; };
struct Slice { const std::function<void(size_t, size_t)> *f; size_t a, b; SliceGroup *g; };
struct Pool {
    std::mutex m; std::condition_variable cv; std::deque<Slice> q;
    explicit Pool(int n) { for (int i = 0; i < n; i++) std::thread([this] { for (;;) { Slice s; { std::unique_lock<std::mutex> l(m); cv.wait(l, [this] { return !q.empty(); }); s = q.front(); q.pop_front(); } run(s); } }).detach(); }
    static void run(const Slice &s) { (*s.f)(s.a, s.b); std::lock_guard<std::mutex> l(s.g->m); if (--s.g->left == 0) s.g->cv.notify_all(); }
    bool try_pop(Slice &s) { std::lock_guard<std::mutex> l(m); if (q.empty()) return false; s = q.front(); q.pop_front(); return true; }
};
Pool *pool() { static Pool *p = new Pool(std::max(0, n_threads() - 1)); return p; }   // never destroyed: its threads sleep on it until the process ends
template <class F> void parallel_for(size_t n, F f) {   // f(first, last) on contiguous slices
    const size_t nt = std::min<size_t>((size_t)n_threads() * 2, std::max<size_t>(n / 64, 1));
    if (nt <= 1 || n_threads() <= 1) { f((size_t)0, n); return; }
    const std::function<void(size_t, size_t)> fn = f;
    SliceGroup g; g.left = nt;
    Pool *P = pool();
    { std::lock_guard<std::mutex> l(P->m); for (size_t t = 1; t < nt; t++) P->q.push_back(Slice{ &fn, n * t / nt, n * (t + 1) / nt, &g }); }
    P->cv.notify_all();
    Pool::run(Slice{ &fn, 0, n / nt, &g });
    for (;;) {
        { std::lock_guard<std::mutex> l(g.m); if (g.left == 0) break; }
        Slice s;
        if (P->try_pop(s)) { Pool::run(s); continue; }   // ours or another reader's: either way a core does useful work
        std::unique_lock<std::mutex> l(g.m); g.cv.wait(l, [&] { return g.left == 0; }); break;
    }
}
// CRC-32 of a block with carry-less multiplication (the folding scheme of Intel's "Fast CRC computation using PCLMULQDQ", constants
// for the reflected polynomial 0xEDB88320): zlib 1.2.11's table walk does 1.1 GB/s, a quarter of the time of inflating a BGZF block.
#if defined(__x86_64__)
__attribute__((target("pclmul,sse4.1"))) static uint32_t crc32_fold(const uint8_t *buf, size_t len, uint32_t crc) {   // len >= 64, multiple of 16; crc = ~running value
    alignas(16) static const uint64_t k1k2[2] = { 0x0154442bd4ULL, 0x01c6e41596ULL };
    alignas(16) static const uint64_t k3k4[2] = { 0x01751997d0ULL, 0x00ccaa009eULL };
    alignas(16) static const uint64_t k5k0[2] = { 0x0163cd6124ULL, 0x0000000000ULL };
    alignas(16) static const uint64_t poly[2] = { 0x01db710641ULL, 0x01f7011641ULL };
    __m128i x0, x1, x2, x3, x4, x5, x6, x7, x8, y5, y6, y7, y8;
    x1 = _mm_loadu_si128((const __m128i *)(buf + 0x00)); x2 = _mm_loadu_si128((const __m128i *)(buf + 0x10));
    x3 = _mm_loadu_si128((const __m128i *)(buf + 0x20)); x4 = _mm_loadu_si128((const __m128i *)(buf + 0x30));
    x1 = _mm_xor_si128(x1, _mm_cvtsi32_si128((int)crc));
    x0 = _mm_load_si128((const __m128i *)k1k2);
    buf += 64; len -= 64;
    while (len >= 64) {   // four lanes of 16 bytes folded over 64 bytes
        x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x6 = _mm_clmulepi64_si128(x2, x0, 0x00); x7 = _mm_clmulepi64_si128(x3, x0, 0x00); x8 = _mm_clmulepi64_si128(x4, x0, 0x00);
        x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x2 = _mm_clmulepi64_si128(x2, x0, 0x11); x3 = _mm_clmulepi64_si128(x3, x0, 0x11); x4 = _mm_clmulepi64_si128(x4, x0, 0x11);
        y5 = _mm_loadu_si128((const __m128i *)(buf + 0x00)); y6 = _mm_loadu_si128((const __m128i *)(buf + 0x10));
        y7 = _mm_loadu_si128((const __m128i *)(buf + 0x20)); y8 = _mm_loadu_si128((const __m128i *)(buf + 0x30));
        x1 = _mm_xor_si128(_mm_xor_si128(x1, x5), y5); x2 = _mm_xor_si128(_mm_xor_si128(x2, x6), y6);
        x3 = _mm_xor_si128(_mm_xor_si128(x3, x7), y7); x4 = _mm_xor_si128(_mm_xor_si128(x4, x8), y8);
        buf += 64; len -= 64;
    }
    x0 = _mm_load_si128((const __m128i *)k3k4);   // the four lanes into one
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x2), x5);
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x3), x5);
    x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x4), x5);
    while (len >= 16) {
        x2 = _mm_loadu_si128((const __m128i *)buf);
        x5 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_clmulepi64_si128(x1, x0, 0x11); x1 = _mm_xor_si128(_mm_xor_si128(x1, x2), x5);
        buf += 16; len -= 16;
    }
    x2 = _mm_clmulepi64_si128(x1, x0, 0x10);   // 128 -> 64 bits
    x3 = _mm_setr_epi32(~0, 0, ~0, 0);
    x1 = _mm_srli_si128(x1, 8); x1 = _mm_xor_si128(x1, x2);
    x0 = _mm_loadl_epi64((const __m128i *)k5k0);
    x2 = _mm_srli_si128(x1, 4); x1 = _mm_and_si128(x1, x3); x1 = _mm_clmulepi64_si128(x1, x0, 0x00); x1 = _mm_xor_si128(x1, x2);
    x0 = _mm_load_si128((const __m128i *)poly);   // Barrett reduction to 32 bits
    x2 = _mm_and_si128(x1, x3); x2 = _mm_clmulepi64_si128(x2, x0, 0x10); x2 = _mm_and_si128(x2, x3); x2 = _mm_clmulepi64_si128(x2, x0, 0x00);
    x1 = _mm_xor_si128(x1, x2);
    return (uint32_t)_mm_extract_epi32(x1, 1);
}
static const bool g_have_pclmul = __builtin_cpu_supports("pclmul") && __builtin_cpu_supports("sse4.1");
#else
static const bool g_have_pclmul = false;
static uint32_t crc32_fold(const uint8_t *, size_t, uint32_t c) { return c; }
#endif
uint32_t block_crc32(const uint8_t *p, size_t n) {
    if (!g_have_pclmul || n < 64) return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)n);
    const size_t body = n & ~(size_t)15;
    const uint32_t c = ~crc32_fold(p, body, ~0u);
    return (n > body) ? (uint32_t)crc32(c, p + body, (uInt)(n - body)) : c;
}
const bool g_fast_inflate = (getenv("UVCIO_ZLIB") == nullptr);   // UVCIO_ZLIB=1: every block through zlib (A/B)
bool inflate_block(const uint8_t *blk, uint32_t csize, uint8_t *dst, uint32_t isize) {
    const int xlen = le16(blk + 10);
    const uint8_t *cdata = blk + 12 + xlen;
    const int clen = (int)csize - xlen - 20;
    if (clen < 0) return false;
    if (isize == 0) return true;
    // the decoder of uvc_inflate_fast.h first; zlib looks at whatever it declines or gets wrong (the CRC-32 of the block decides)
    if (g_fast_inflate && uvc_fast_inflate::inflate(cdata, (size_t)clen, dst, isize) && block_crc32(dst, isize) == le32(blk + csize - 8)) return true;
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t *>(cdata); zs.avail_in = (uInt)clen; zs.next_out = dst; zs.avail_out = isize;
    const int rc = inflate(&zs, Z_FINISH);
    inflateEnd(&zs);
    return rc == Z_STREAM_END && zs.total_out == isize && block_crc32(dst, isize) == le32(blk + csize - 8);
}
const uint8_t NT16_INT[16] = { 4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4 };   // seq_nt16_int of htslib: =ACMGRSVTWYHKDBN

// NM aux tag of the record at r (bam_aux_get + bam_aux2i), -1 if absent; false on a corrupt aux area
bool aux_nm(const uint8_t *r, size_t bs, size_t o, int32_t &nm) {
    nm = -1;
    while (o + 3 <= bs) {
        const char t0 = (char)r[o], t1 = (char)r[o + 1], ty = (char)r[o + 2];
        o += 3;
        size_t sz = 0; long long val = 0; bool is_int = true;
        switch (ty) {
            case 'A': sz = 1; is_int = false; break;
            case 'c': sz = 1; if (o + 1 <= bs) val = (int8_t)r[o]; break;
            case 'C': sz = 1; if (o + 1 <= bs) val = r[o]; break;
            case 's': sz = 2; if (o + 2 <= bs) val = (int16_t)le16(r + o); break;
            case 'S': sz = 2; if (o + 2 <= bs) val = le16(r + o); break;
            case 'i': sz = 4; if (o + 4 <= bs) val = (int32_t)le32(r + o); break;
            case 'I': sz = 4; if (o + 4 <= bs) val = le32(r + o); break;
            case 'f': sz = 4; is_int = false; break;
            case 'Z': case 'H': { size_t k = o; while (k < bs && r[k]) k++; sz = k - o + 1; is_int = false; break; }
            case 'B': {
                if (o + 5 > bs) return false;
                const char sub = (char)r[o]; const uint32_t cnt = le32(r + o + 1);
                const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                sz = 5 + es * (size_t)cnt; is_int = false; break;
            }
            default: return false;
        }
        if (o + sz > bs) return false;
        if (t0 == 'N' && t1 == 'M' && is_int) nm = (int32_t)val;
        o += sz;
    }
    return true;
}

}  // namespace

static int bam_fetch_impl(uvcio_bam_t *b, int32_t tid, int64_t beg, int64_t end, UvcBamBatch *out);
// no exception crosses the C boundary: a column that cannot grow is UVCGPU_ENOMEM
extern "C" int uvcio_bam_fetch(uvcio_bam_t *b, int32_t tid, int64_t beg, int64_t end, UvcBamBatch *out) {
    try { return bam_fetch_impl(b, tid, beg, end, out); }
    catch (const std::bad_alloc &) { return fail(UVCGPU_ENOMEM, "uvcio_bam_fetch: out of host memory"); }
    catch (const std::exception &e) { return fail(UVCGPU_EINVAL, std::string("uvcio_bam_fetch: ") + e.what()); }
}
static int bam_fetch_impl(uvcio_bam_t *b, int32_t tid, int64_t beg, int64_t end, UvcBamBatch *out) {
    if (!b || !out) return fail(UVCGPU_EINVAL, "null argument");
    if (tid < 0 || tid >= (int32_t)b->ref_names.size()) return fail(UVCGPU_EINVAL, "tid out of range");
    if (beg < 0) beg = 0;
    if (end > b->ref_lens[tid]) end = b->ref_lens[tid];
    b->tid.clear(); b->pos.clear(); b->endpos.clear(); b->mtid.clear(); b->mpos.clear(); b->isize.clear(); b->nm.clear(); b->l_qseq.clear(); b->n_cigar.clear();
    b->flag.clear(); b->mapq.clear(); b->seq_off.clear(); b->cigar_off.clear(); b->qname_off.clear(); b->bases.clear(); b->quals.clear(); b->cigars.clear(); b->qnames.clear();
    if (end > beg) {
        std::vector<Chunk> chunks;
        if (b->has_index) {
            const RefIndex &ri = b->idx[tid];
            const size_t w = (size_t)(beg >> 14);
            const uint64_t min_off = ri.linear.empty() ? 0 : ri.linear[std::min(w, ri.linear.size() - 1)];
            std::vector<uint32_t> bins; reg2bins(beg, end, bins);
            for (uint32_t bin : bins) { auto it = ri.bins.find(bin); if (it != ri.bins.end()) for (const Chunk &c : it->second) if (c.end > min_off) chunks.push_back(Chunk{ std::max(c.beg, min_off), c.end }); }
            std::sort(chunks.begin(), chunks.end(), [](const Chunk &a, const Chunk &c) { return a.beg < c.beg; });
            std::vector<Chunk> merged;
            // chunks that continue in the block behind the previous one are read as one run (an index written record by record ends every
            // chunk at its block's end; what lies between is at most one block of records, which the overlap test drops again)
            for (const Chunk &c : chunks) { if (!merged.empty() && (int64_t)(c.beg >> 16) <= (int64_t)(merged.back().end >> 16) + 65536) merged.back().end = std::max(merged.back().end, c.end); else merged.push_back(c); }
            chunks.swap(merged);
        } else chunks.push_back(Chunk{ b->first_record, ~0ull });
        // compressed bytes per batch (UVCIO_BATCH_BYTES: tests use small batches to exercise records that straddle two)
        const char *be = getenv("UVCIO_BATCH_BYTES");
        const size_t BATCH = (be && atol(be) >= (1 << 16)) ? (size_t)atol(be) : ((size_t)64 << 20);
        const bool timing = (getenv("UVCIO_TIMING") != nullptr);
        double t_read = 0, t_inf = 0, t_walk = 0, t_dec = 0;
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        std::vector<uint8_t> carry;
        int64_t file_size = -1;
        if (fseeko(b->z.fp, 0, SEEK_END) == 0) file_size = (int64_t)ftello(b->z.fp);
        std::vector<BlockRef> blocks;
        std::vector<RecRef> recs;
        bool past = false;
        for (const Chunk &c : chunks) {
            if (past) break;
            int64_t addr = (int64_t)(c.beg >> 16);
            size_t skip = (size_t)(c.beg & 0xFFFF);            // bytes of the first block that lie in front of the chunk
            const int64_t last_addr = (c.end == ~0ull ? INT64_MAX : (int64_t)(c.end >> 16));
            const size_t last_u = (size_t)(c.end & 0xFFFF);
            carry.clear();
            bool chunk_done = false;
            while (!chunk_done && !past) {
                // 1. read whole blocks of this batch
                double t0 = now();
                if (fseeko(b->z.fp, (off_t)addr, SEEK_SET) != 0) return fail(UVCGPU_EINVAL, "seek failed");
                // no more than the chunk (plus its last block) or the rest of the file
                size_t want = BATCH + (1 << 16);
                if (last_addr != INT64_MAX) want = std::min<size_t>(want, (size_t)(last_addr - addr) + (1 << 16) + 18);
                if (file_size >= 0) want = std::min<size_t>(want, (size_t)std::max<int64_t>(file_size - addr, 0));
                uint8_t *const cbuf = b->comp.need(std::max<size_t>(want, 1));
                if (!cbuf) return fail(UVCGPU_ENOMEM, "uvcio_bam_fetch: no memory for the compressed batch");
                const size_t got = fread(cbuf, 1, want, b->z.fp);
                const bool at_eof = (file_size >= 0 ? (addr + (int64_t)got >= file_size) : (got < want));
                blocks.clear();
                size_t o = 0, out_bytes = 0;
                bool hit_last = false;
                while (o + 18 <= got && !hit_last) {
                    const uint8_t *h = cbuf + o;
                    if (h[0] != 31 || h[1] != 139 || !(h[3] & 4)) return fail(UVCGPU_EINVAL, "not a BGZF block where the index points");
                    const int xlen = le16(h + 10);
                    if (o + 12 + (size_t)xlen > got) break;
                    int bsize = -1;
                    for (int i = 0; i + 4 <= xlen;) { const int slen = le16(h + 12 + i + 2); if (h[12 + i] == 'B' && h[12 + i + 1] == 'C' && slen == 2) bsize = le16(h + 12 + i + 4); i += 4 + slen; }
                    if (bsize < 0) return fail(UVCGPU_EINVAL, "BGZF block without a BC field");
                    const size_t csize = (size_t)bsize + 1;
                    if (o + csize > got) break;                 // incomplete block: next batch starts here
                    const uint32_t isize = le32(h + csize - 4);
                    blocks.push_back(BlockRef{ addr + (int64_t)o, (uint32_t)csize, isize, o, out_bytes });
                    out_bytes += isize; o += csize;
                    if (addr + (int64_t)(o - csize) >= last_addr) hit_last = true;   // the block that holds the chunk end
                    if (o >= BATCH) break;
                }
                if (blocks.empty()) { if (got >= 18 && o == 0 && !at_eof && got == want) return fail(UVCGPU_EINVAL, "BGZF block larger than the batch"); chunk_done = true; break; }
                t_read += now() - t0; t0 = now();
                // 2. inflate in parallel
                const size_t infl_size = carry.size() + out_bytes;
                uint8_t *const ibuf = b->infl.need(std::max<size_t>(infl_size, 1));
                if (!ibuf) return fail(UVCGPU_ENOMEM, "uvcio_bam_fetch: no memory for the inflated batch");
                if (!carry.empty()) memcpy(ibuf, carry.data(), carry.size());
                std::atomic<bool> ok{ true }; bool done = false;   // (flags written from the pool's threads are atomics)
                if (g_inflate_fn && (int64_t)blocks.size() >= (int64_t)g_inflate_min) {   // somewhere else (the device); the CRC-32 of every block is checked here
                    const size_t nb2 = blocks.size();
                    std::vector<int64_t> in_off(nb2), out_off(nb2); std::vector<int32_t> in_len(nb2), out_len(nb2);
                    bool sane = true;
                    for (size_t i = 0; i < nb2; i++) {
                        const uint8_t *blk = cbuf + blocks[i].in_off;
                        const int xlen = le16(blk + 10), clen = (int)blocks[i].csize - xlen - 20;
                        if (clen < 0) { sane = false; break; }
                        in_off[i] = (int64_t)blocks[i].in_off + 12 + xlen; in_len[i] = clen; out_off[i] = (int64_t)(carry.size() + blocks[i].out_off); out_len[i] = (int32_t)blocks[i].isize;
                    }
                    if (sane && g_inflate_fn(g_inflate_ctx, cbuf, (int64_t)o, in_off.data(), in_len.data(), out_off.data(), out_len.data(), (int64_t)nb2, ibuf, (int64_t)infl_size) == 0) {
                        std::atomic<bool> crc_ok{ true };
                        parallel_for(nb2, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) if (blocks[i].isize && block_crc32(ibuf + out_off[i], blocks[i].isize) != le32(cbuf + blocks[i].in_off + blocks[i].csize - 8)) crc_ok = false; });
                        done = crc_ok;
                    }
                }
                if (!done) parallel_for(blocks.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) if (!inflate_block(cbuf + blocks[i].in_off, blocks[i].csize, ibuf + carry.size() + blocks[i].out_off, blocks[i].isize)) ok = false; });
                if (!ok) return fail(UVCGPU_EINVAL, "corrupt BGZF block (inflate / CRC)");
                t_inf += now() - t0; t0 = now();
                // the usable byte range of this batch
                size_t lo = (carry.empty() ? skip : 0), hi = infl_size;
                skip = 0;
                if (hit_last) { const BlockRef &L = blocks.back(); if (L.addr == last_addr) hi = carry.size() + L.out_off + std::min<size_t>(last_u, L.isize); chunk_done = true; }
                if (at_eof && o >= got - std::min<size_t>(got, 17)) chunk_done = true;   // end of file
                // 3. Which records overlap, where their outputs go.  The chain of record sizes is one dependent load per record through
                // memory that other cores have just written (~100 ns each: as long as the parallel inflate when walked by one thread).
                // htslib starts a new BGZF block rather than let a record straddle two (bgzf_flush_try in bam_write1), so in the files it
                // wrote every block begins with a record: the blocks are walked in parallel, twice (sizes, then offsets).  A block whose
                // walk does not end on its last byte disproves that for this file, and the batch is walked the sequential way.
                recs.clear();
                size_t p = lo;
                int64_t nb = (int64_t)b->bases.size(), nc = (int64_t)b->cigars.size(), nq = (int64_t)b->qnames.size();
                // one record at ibuf + q: 0 = behind the query (stop), 1 = skip, 2 = keep; sizes of a kept record in *e .. *ln
                auto classify = [&](size_t q, uint32_t bs, int32_t *e_out, int32_t *lseq, int32_t *ncig, int32_t *ln, bool *bad) -> int {
                    const uint8_t *r = ibuf + q + 4;
                    const int32_t rt = (int32_t)le32(r), rp = (int32_t)le32(r + 4);
                    const int l_name = r[8], n_cig = le16(r + 12); const int32_t l_seq = (int32_t)le32(r + 16);
                    if (rt > tid || rt < 0 || (rt == tid && rp >= end)) return 0;
                    if (rt != tid) return 1;
                    const size_t o_cig = 32 + (size_t)l_name;
                    if (l_seq < 0 || o_cig + 4 * (size_t)n_cig + ((size_t)l_seq + 1) / 2 + (size_t)l_seq > bs) { *bad = true; return 0; }
                    int64_t e = rp;
                    for (int k = 0; k < n_cig; k++) { const uint32_t cg = le32(r + o_cig + 4 * (size_t)k); const int op = (int)(cg & 0xF); if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) e += (int64_t)(cg >> 4); }
                    if (e == rp) e = rp + 1;
                    if (!(rp < end && e > beg)) return 1;
                    *e_out = (int32_t)e; *lseq = l_seq; *ncig = n_cig; *ln = l_name + ((l_name == 0 || r[32 + l_name - 1] != 0) ? 1 : 0);
                    return 2;
                };
                bool walked = false;
                if (carry.empty() && blocks.size() >= 4 && n_threads() > 1 && !getenv("UVCIO_SERIAL_WALK")) {
                    struct BlockWalk { size_t stop; int64_t n, sb, sc, sq; bool aligned, past, bad, size_bad; };
                    const int32_t n_refs = (int32_t)b->ref_names.size();
                    std::vector<BlockWalk> bw(blocks.size());
                    auto walk_block = [&](size_t k, RecRef *dst, int64_t ob, int64_t oc, int64_t oq) {   // dst == nullptr: count only
                        const size_t s0 = std::max(blocks[k].out_off, lo), e0 = std::min(blocks[k].out_off + (size_t)blocks[k].isize, hi);
                        BlockWalk w = { s0, 0, 0, 0, 0, true, false, false, false };
                        size_t q = s0;
                        while (q + 4 <= e0) {
                            const uint32_t bs = le32(ibuf + q);
                            if (bs < 32 || bs > (1u << 28)) { w.size_bad = true; break; }
                            if (q + 4 + bs > e0) break;
                            {   // bytes that only look like a record (a block that does begin inside one) must not pass: what every record has
                                const uint8_t *r = ibuf + q + 4;
                                const int32_t rt = (int32_t)le32(r), rp = (int32_t)le32(r + 4); const int l_name = r[8];
                                if (rt < -1 || rt >= n_refs || rp < -1 || l_name < 1 || 32 + (uint32_t)l_name > bs || r[32 + l_name - 1] != 0) { w.size_bad = true; break; }
                            }
                            int32_t e = 0, ls = 0, ncg = 0, ln = 0;
                            const int c = classify(q, bs, &e, &ls, &ncg, &ln, &w.bad);
                            if (c == 0) { w.past = !w.bad; break; }
                            if (c == 2) {
                                if (dst) dst[w.n] = RecRef{ ibuf + q + 4, bs, e, ob + w.sb, oc + w.sc, oq + w.sq };
                                w.n++; w.sb += ls; w.sc += ncg; w.sq += ln;
                            }
                            q += 4 + bs;
                        }
                        w.stop = q;
                        // the walk must end on the block's last byte (the last block of the query may end at the chunk's end instead)
                        w.aligned = (w.past || w.bad || w.size_bad || q == e0 || s0 >= e0);
                        if (!dst) bw[k] = w;
                    };
                    parallel_for(blocks.size(), [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; k++) walk_block(k, nullptr, 0, 0, 0); });
                    bool all_aligned = true;
                    for (size_t k = 0; k + 1 < blocks.size(); k++) if (!bw[k].aligned) { all_aligned = false; break; }   // (the last block may hold the first part of a record)
                    for (const BlockWalk &w : bw) if (w.size_bad || w.bad) all_aligned = false;   // not records there: the sequential walk decides what the file is
                    if (all_aligned) {
                        // up to the first block that reaches the end of the query
                        size_t k_end = blocks.size();
                        for (size_t k = 0; k < blocks.size(); k++) {
                            if (bw[k].past) { k_end = k + 1; past = true; break; }
                        }
                        std::vector<int64_t> off_n(k_end + 1, 0), off_b(k_end + 1, nb), off_c(k_end + 1, nc), off_q(k_end + 1, nq);
                        for (size_t k = 0; k < k_end; k++) { off_n[k + 1] = off_n[k] + bw[k].n; off_b[k + 1] = off_b[k] + bw[k].sb; off_c[k + 1] = off_c[k] + bw[k].sc; off_q[k + 1] = off_q[k] + bw[k].sq; }
                        recs.resize((size_t)off_n[k_end]);
                        parallel_for(k_end, [&](size_t k0, size_t k1) { for (size_t k = k0; k < k1; k++) walk_block(k, recs.data() + off_n[k], off_b[k], off_c[k], off_q[k]); });
                        nb = off_b[k_end]; nc = off_c[k_end]; nq = off_q[k_end];
                        p = bw[k_end - 1].stop;
                        walked = true;
                    }
                }
                if (!walked) while (p + 4 <= hi) {
                    const uint32_t bs = le32(ibuf + p);
                    if (bs < 32 || bs > (1u << 28)) return fail(UVCGPU_EINVAL, "implausible BAM record size");
                    if (p + 4 + bs > hi) break;
                    int32_t e = 0, ls = 0, ncg = 0, ln = 0; bool bad = false;
                    const int c = classify(p, bs, &e, &ls, &ncg, &ln, &bad);
                    if (bad) return fail(UVCGPU_EINVAL, "corrupt BAM record");
                    if (c == 0) { past = true; break; }
                    if (c == 2) { recs.push_back(RecRef{ ibuf + p + 4, bs, e, nb, nc, nq }); nb += ls; nc += ncg; nq += ln; }
                    p += 4 + bs;
                }
                t_walk += now() - t0; t0 = now();
                // 4. decode in parallel
                const size_t r0 = b->pos.size(), nr = recs.size();
                b->tid.resize(r0 + nr); b->pos.resize(r0 + nr); b->endpos.resize(r0 + nr); b->mtid.resize(r0 + nr); b->mpos.resize(r0 + nr); b->isize.resize(r0 + nr); b->nm.resize(r0 + nr);
                b->l_qseq.resize(r0 + nr); b->n_cigar.resize(r0 + nr); b->flag.resize(r0 + nr); b->mapq.resize(r0 + nr); b->seq_off.resize(r0 + nr); b->cigar_off.resize(r0 + nr); b->qname_off.resize(r0 + nr);
                b->bases.resize((size_t)nb); b->quals.resize((size_t)nb); b->cigars.resize((size_t)nc); b->qnames.resize((size_t)nq);
                std::atomic<bool> aux_ok{ true };
                parallel_for(nr, [&](size_t i0, size_t i1) {
                    for (size_t i = i0; i < i1; i++) {
                        const RecRef &q = recs[i]; const uint8_t *r = q.r; const size_t k = r0 + i;
                        const int l_name = r[8], n_cig = le16(r + 12); const int32_t l_seq = (int32_t)le32(r + 16);
                        const size_t o_cig = 32 + (size_t)l_name, o_seq = o_cig + 4 * (size_t)n_cig, o_qual = o_seq + ((size_t)l_seq + 1) / 2, o_aux = o_qual + (size_t)l_seq;
                        b->tid[k] = (int32_t)le32(r); b->pos[k] = (int32_t)le32(r + 4); b->endpos[k] = q.endpos; b->mapq[k] = r[9]; b->flag[k] = le16(r + 14);
                        b->mtid[k] = (int32_t)le32(r + 20); b->mpos[k] = (int32_t)le32(r + 24); b->isize[k] = (int32_t)le32(r + 28);
                        b->l_qseq[k] = l_seq; b->n_cigar[k] = n_cig; b->seq_off[k] = q.base_off; b->cigar_off[k] = q.cig_off; b->qname_off[k] = q.name_off;
                        int32_t nm; if (!aux_nm(r, q.size, o_aux, nm)) aux_ok = false;
                        b->nm[k] = nm;
                        for (int c = 0; c < n_cig; c++) b->cigars[(size_t)q.cig_off + c] = le32(r + o_cig + 4 * (size_t)c);
                        uint8_t *bd = b->bases.data() + q.base_off;
                        for (int32_t j = 0; j < l_seq; j++) { const uint8_t by = r[o_seq + (size_t)(j >> 1)]; bd[j] = NT16_INT[(j & 1) ? (by & 0xF) : (by >> 4)]; }
                        memcpy(b->quals.data() + q.base_off, r + o_qual, (size_t)l_seq);
                        memcpy(b->qnames.data() + q.name_off, r + 32, (size_t)l_name);
                        if (l_name == 0 || r[32 + l_name - 1] != 0) b->qnames[(size_t)q.name_off + l_name] = '\0';
                    }
                });
                if (!aux_ok) return fail(UVCGPU_EINVAL, "corrupt aux fields in a BAM record");
                t_dec += now() - t0;
                // 5. what is left of a record that continues in the next batch
                if (!chunk_done && !past) { std::vector<uint8_t> rest(ibuf + p, ibuf + hi); carry.swap(rest); addr = blocks.back().addr + blocks.back().csize; }
                else if (!past && p < hi && hit_last && blocks.back().addr == last_addr) { /* the chunk ends inside a record only in a broken index */ }
            }
        }
        if (timing) fprintf(stderr, "[uvcio fetch] threads %d: read+headers %.3f s, inflate %.3f s, record walk %.3f s, decode %.3f s\n", n_threads(), t_read, t_inf, t_walk, t_dec);
    }
    out->n_alns = (int64_t)b->pos.size();
    out->tid = b->tid.data(); out->pos = b->pos.data(); out->endpos = b->endpos.data(); out->mtid = b->mtid.data(); out->mpos = b->mpos.data(); out->isize = b->isize.data();
    out->flag = b->flag.data(); out->mapq = b->mapq.data(); out->nm = b->nm.data(); out->l_qseq = b->l_qseq.data(); out->n_cigar = b->n_cigar.data();
    out->seq_off = b->seq_off.data(); out->cigar_off = b->cigar_off.data(); out->qname_off = b->qname_off.data();
    out->n_bases = (int64_t)b->bases.size(); out->bases = b->bases.data(); out->quals = b->quals.data();
    out->n_cigar_ops = (int64_t)b->cigars.size(); out->cigars = b->cigars.data(); out->n_qname_bytes = (int64_t)b->qnames.size(); out->qnames = b->qnames.data();
    return 0;
}

// ---------------------------------------------------------------- FASTA + .fai ----------------
struct FaiEntry { int64_t len, offset, linebases, linewidth; };
struct uvcio_fasta { FILE *fp = nullptr; std::map<std::string, FaiEntry> seqs; };

extern "C" int uvcio_fasta_open(uvcio_fasta_t **out, const char *path) {
    if (!out || !path) return fail(UVCGPU_EINVAL, "null argument");
    FILE *fi = fopen((std::string(path) + ".fai").c_str(), "r");
    if (!fi) return fail(UVCGPU_EINVAL, std::string("cannot open ") + path + ".fai (samtools faidx layout: name, length, offset, linebases, linewidth)");
    uvcio_fasta *f = new uvcio_fasta();
    char name[4096]; long long a, o, lb, lw;
    char line[8192];
    while (fgets(line, sizeof(line), fi)) if (sscanf(line, "%4095s %lld %lld %lld %lld", name, &a, &o, &lb, &lw) == 5 && lb > 0 && lw >= lb) f->seqs[name] = FaiEntry{ a, o, lb, lw };
    fclose(fi);
    f->fp = fopen(path, "rb");
    if (!f->fp || f->seqs.empty()) { if (f->fp) fclose(f->fp); delete f; return fail(UVCGPU_EINVAL, std::string("cannot open ") + path + " or empty .fai"); }
    *out = f;
    return 0;
}
extern "C" int64_t uvcio_fasta_seq_len(const uvcio_fasta_t *f, const char *name) {
    if (!f || !name) return -1;
    auto it = f->seqs.find(name);
    return it == f->seqs.end() ? -1 : it->second.len;
}
extern "C" int uvcio_fasta_fetch(uvcio_fasta_t *f, const char *name, int64_t beg, int64_t end, char *dst) {
    if (!f || !name || !dst) return fail(UVCGPU_EINVAL, "null argument");
    auto it = f->seqs.find(name);
    if (it == f->seqs.end()) return fail(UVCGPU_EINVAL, std::string("sequence not in the .fai: ") + name);
    const FaiEntry &e = it->second;
    if (beg < 0 || end > e.len || end < beg) return fail(UVCGPU_EINVAL, "FASTA range outside the sequence");
    int64_t i = beg;
    while (i < end) {
        const int64_t line = i / e.linebases, col = i % e.linebases;
        const int64_t k = std::min(end - i, e.linebases - col);
        if (fseeko(f->fp, (off_t)(e.offset + line * e.linewidth + col), SEEK_SET) != 0 || fread(dst + (i - beg), 1, (size_t)k, f->fp) != (size_t)k) return fail(UVCGPU_EINVAL, "short read from the FASTA file");
        i += k;
    }
    for (int64_t k = 0; k < end - beg; k++) if (dst[k] >= 'a' && dst[k] <= 'z') dst[k] = (char)(dst[k] - 32);
    return 0;
}
extern "C" void uvcio_fasta_close(uvcio_fasta_t *f) { if (!f) return; if (f->fp) fclose(f->fp); delete f; }

// ---- BGZF writer (SAMv1 section 4.1): what the reference writes its VCF through (bgzf_open / bgzf_write / bgzf_flush, main.cpp:1196-1215) ----
struct uvcio_bgzf_writer { FILE *fp = nullptr; std::vector<uint8_t> pending; int level = 6; };
namespace {
const size_t BGZF_INPUT_BLOCK = 0xff00;   // uncompressed bytes per block, as htslib
int bgzf_put_block(uvcio_bgzf_writer *w, const uint8_t *src, size_t n) {
    uint8_t out[65536 + 64];
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, w->level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return fail(UVCGPU_EINVAL, "deflateInit2 failed");
    zs.next_in = const_cast<uint8_t *>(src); zs.avail_in = (uInt)n; zs.next_out = out + 18; zs.avail_out = (uInt)(sizeof(out) - 18 - 8);
    const int rc = deflate(&zs, Z_FINISH);
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END || clen + 26 > 65536) return fail(UVCGPU_EINVAL, "BGZF block does not fit 64 KiB");
    const uint8_t head[18] = { 31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, 0, 0 };
    memcpy(out, head, 18);
    const uint32_t bsize = (uint32_t)(clen + 26 - 1);
    out[16] = (uint8_t)(bsize & 0xFF); out[17] = (uint8_t)(bsize >> 8);
    const uint32_t crc = block_crc32(src, n), isize = (uint32_t)n;
    uint8_t *t = out + 18 + clen;
    for (int i = 0; i < 4; i++) { t[i] = (uint8_t)(crc >> (8 * i)); t[4 + i] = (uint8_t)(isize >> (8 * i)); }
    if (fwrite(out, 1, clen + 26, w->fp) != clen + 26) return fail(UVCGPU_EINVAL, "short write");
    return 0;
}
}
extern "C" int uvcio_bgzf_write_open(uvcio_bgzf_writer_t **out, const char *path, int32_t level) {
    if (!out || !path) return fail(UVCGPU_EINVAL, "null argument");
    uvcio_bgzf_writer *w = new uvcio_bgzf_writer();
    w->fp = fopen(path, "wb");
    if (!w->fp) { delete w; return fail(UVCGPU_EINVAL, std::string("cannot create ") + path); }
    w->level = (level < 0 || level > 9) ? 6 : level;
    *out = w;
    return 0;
}
extern "C" int uvcio_bgzf_write(uvcio_bgzf_writer_t *w, const void *data, int64_t n) {
    if (!w || (n > 0 && !data) || n < 0) return fail(UVCGPU_EINVAL, "bad argument");
    const uint8_t *p = (const uint8_t *)data;
    w->pending.insert(w->pending.end(), p, p + n);
    size_t at = 0;
    while (w->pending.size() - at >= BGZF_INPUT_BLOCK) { const int rc = bgzf_put_block(w, w->pending.data() + at, BGZF_INPUT_BLOCK); if (rc) return rc; at += BGZF_INPUT_BLOCK; }
    w->pending.erase(w->pending.begin(), w->pending.begin() + (ptrdiff_t)at);
    return 0;
}
// flushes the pending bytes as a (short) block and appends the 28-byte end-of-file marker block
extern "C" int uvcio_bgzf_write_close(uvcio_bgzf_writer_t *w) {
    if (!w) return 0;
    int rc = 0;
    if (!w->pending.empty()) rc = bgzf_put_block(w, w->pending.data(), w->pending.size());
    if (!rc) rc = bgzf_put_block(w, nullptr, 0);
    if (fclose(w->fp) != 0 && !rc) rc = fail(UVCGPU_EINVAL, "close failed");
    delete w;
    return rc;
}

// ---- the region planner: SamIter::iternext without a BED file (grouping.cpp:225-312) over the alignment columns in file order ----
// A block of the reference is cut when the contig changes (flag 16), the next read starts more than 2 * MAX_STR_N_BASES behind the
// running end (8), the block's estimated memory exceeds the per-thread budget (4, check_if_sub_is_over_mem_lim, grouping.cpp:49-67) or
// the file ends (2); check_if_is_over_mem_lim (grouping.cpp:28-47) closes a batch of blocks, which drops the read that triggered the
// cut from the running end of the next block exactly as the reference's early return does.
namespace {
const int64_t PLAN_BYTES_PER_REF_POS = 1024 * 8, PLAN_BYTES_PER_READ = 512, PLAN_MAX_STR_N_BASES = 100, PLAN_UNITS_PER_THREAD = 8;
bool plan_batch_over(int64_t n_reads, int64_t reads_sq, int64_t n_rposs, int64_t rposs_sq, int64_t nthreads, int64_t mem_mb) {
    const uint64_t by_reads = (uint64_t)(std::min<uint64_t>((uint64_t)(reads_sq / std::max<int64_t>(1, n_reads)) * (uint64_t)nthreads, (uint64_t)n_reads) * (uint64_t)PLAN_BYTES_PER_READ);
    const uint64_t by_rposs = (uint64_t)((std::min<uint64_t>((uint64_t)(rposs_sq / std::max<int64_t>(1, n_rposs)) * (uint64_t)nthreads, (uint64_t)n_rposs) + (uint64_t)(2 * PLAN_MAX_STR_N_BASES * nthreads)) * (uint64_t)PLAN_BYTES_PER_REF_POS);
    const uint64_t by_vcf = (uint64_t)n_rposs * 1024;
    return (by_reads + by_rposs + by_vcf) > (uint64_t)(1024 * 1024) * (uint64_t)mem_mb * (uint64_t)nthreads;
}
bool plan_block_over(int64_t n_reads, int64_t n_rposs, int64_t mem_mb, int64_t curr_beg, int64_t running_end) {
    const uint64_t used = (uint64_t)(n_reads * PLAN_BYTES_PER_READ) + (uint64_t)(n_rposs * (PLAN_BYTES_PER_REF_POS + 1024));
    const uint64_t memfree = (uint64_t)((1024 * 1024) / PLAN_UNITS_PER_THREAD) * (uint64_t)mem_mb;
    const uint64_t ovl = (uint64_t)std::min<int64_t>(running_end > curr_beg ? running_end - curr_beg : 0, 150);   // size_t arithmetic in the reference: both are non-negative here
    return used > memfree + memfree * ovl / 150;
}
}
// The planner as a stream: the walk keeps a handful of scalars between alignments, so a caller that reads a whole genome feeds it window by
// window and holds no per-alignment column (uvc1-mi355x; uvcio_plan_regions below is the one-call form of the same code).
struct uvcio_planner {
    int64_t nthreads, mem_mb; std::vector<int64_t> target_len;
    int64_t block_tid = -1, block_beg = -1, block_running_end = -1;   // last_it_* (grouping.hpp)
    int64_t total_reads = 0, total_rposs = 0, total_reads_sq = 0, total_rposs_sq = 0;   // of the current iternext() call
    int64_t region_reads = 0, region_rposs = 0, region_rposs_add = 0;
    int32_t batch = 0;
    bool any = false, last_unmapped = false, done = false;
    bool cur_valid = false;   // this iternext() call has read a record (the end of the file is only processed on a record the call itself holds)
    int64_t last_tid = 0, last_pos = 0, last_end = 0;
    std::vector<UvcRegionCut> cuts;   // cuts that have not been taken yet
    void new_call() { cur_valid = false; total_reads = total_rposs = total_reads_sq = total_rposs_sq = 0; region_reads = region_rposs = region_rposs_add = 0; batch++; }
    // the body of iternext's read loop for one record (ret = 0) or for the end of the file (ret = -1, on the last record read)
    void step(int64_t curr_tid, int64_t curr_beg, int64_t curr_end, int ret) {
        const bool sub_over = plan_block_over(region_reads, region_rposs + region_rposs_add, mem_mb, curr_beg, block_running_end < 0 ? 0 : block_running_end);
        const bool tmpl_changed = (curr_tid != block_tid);
        const bool far_jumped = ((curr_tid == block_tid) && (block_running_end + (PLAN_MAX_STR_N_BASES * 2) < curr_beg));
        const int32_t rflag = (tmpl_changed ? 16 : 0) + (far_jumped ? 8 : 0) + (sub_over ? 4 : 0) + ((-1 == ret) ? 2 : 0);
        if (rflag) {
            const bool first = (-1 == block_tid);
            const int64_t tlen = first ? (int64_t)INT32_MAX : ((block_tid < (int64_t)target_len.size()) ? target_len[(size_t)block_tid] : (int64_t)INT32_MAX);
            const int64_t norm_end = std::min(block_running_end, tlen);
            const bool zero = (block_beg >= norm_end);
            if (!first && !zero) {
                cuts.push_back(UvcRegionCut{ (int32_t)block_tid, (int32_t)block_beg, (int32_t)norm_end, rflag, batch, region_reads });
                const int64_t s_rposs = region_rposs + region_rposs_add;
                total_reads += region_reads; total_rposs += s_rposs; total_reads_sq += region_reads * region_reads; total_rposs_sq += s_rposs * s_rposs;
                region_rposs = 0; region_rposs_add = 0; region_reads = 0;
            }
            block_tid = curr_tid;
            const int64_t new_beg = std::max(block_beg, curr_beg);
            block_beg = (tmpl_changed ? curr_beg : std::max(new_beg, norm_end));
            if (plan_batch_over(total_reads, total_reads_sq, total_rposs, total_rposs_sq, nthreads, mem_mb)) {
                block_running_end = std::max(block_beg, norm_end);
                new_call();   // iternext returns here: the record that closed the batch is not counted (the reference drops it the same way)
                return;
            }
        }
        if (tmpl_changed) { block_beg = curr_beg; block_running_end = curr_end; region_rposs_add += region_rposs; }
        else block_running_end = std::max(block_running_end, curr_end);
        region_reads++;
        region_rposs = block_running_end - block_beg;
    }
};
extern "C" int uvcio_planner_open(uvcio_planner_t **out, const int64_t *target_len, int32_t n_targets, int32_t nthreads, int64_t mem_per_thread_mb) {
    if (!out || nthreads < 1 || mem_per_thread_mb < 1 || n_targets < 0) return fail(UVCGPU_EINVAL, "bad argument");
    uvcio_planner *p = new uvcio_planner();
    p->nthreads = nthreads; p->mem_mb = mem_per_thread_mb;
    if (target_len) p->target_len.assign(target_len, target_len + n_targets);
    *out = p;
    return 0;
}
extern "C" int uvcio_planner_feed(uvcio_planner_t *p, const int32_t *tid, const int32_t *pos, const int32_t *endpos, const uint16_t *flag, int64_t n) {
    if (!p || n < 0 || (n > 0 && (!tid || !pos || !endpos || !flag)) || p->done) return fail(UVCGPU_EINVAL, "bad argument");
    for (int64_t i = 0; i < n; i++) {
        p->any = true; p->cur_valid = true; p->last_unmapped = (flag[i] & 0x4) != 0; p->last_tid = tid[i]; p->last_pos = pos[i]; p->last_end = endpos[i];
        if (flag[i] & 0x4) continue;   // BAM_FUNMAP
        p->step(tid[i], pos[i], endpos[i], 0);
    }
    return 0;
}
extern "C" int uvcio_planner_finish(uvcio_planner_t *p) {   // the end of the file: the read call fails and the loop body runs once more on the record it still holds
    if (!p) return fail(UVCGPU_EINVAL, "bad argument");
    if (!p->done && p->any && p->cur_valid && !p->last_unmapped) p->step(p->last_tid, p->last_pos, p->last_end, -1);
    p->done = true;
    return 0;
}
extern "C" int64_t uvcio_planner_take(uvcio_planner_t *p, UvcRegionCut *out, int64_t capacity) {   // moves up to `capacity` finished cuts out, in order
    if (!p || capacity < 0 || (capacity > 0 && !out)) return 0;
    const int64_t n = std::min<int64_t>(capacity, (int64_t)p->cuts.size());
    for (int64_t k = 0; k < n; k++) out[k] = p->cuts[(size_t)k];
    p->cuts.erase(p->cuts.begin(), p->cuts.begin() + n);
    return n;
}
extern "C" int64_t uvcio_planner_pending(const uvcio_planner_t *p) { return p ? (int64_t)p->cuts.size() : 0; }
extern "C" void uvcio_planner_close(uvcio_planner_t *p) { delete p; }

extern "C" int uvcio_plan_regions(const int32_t *tid, const int32_t *pos, const int32_t *endpos, const uint16_t *flag, int64_t n,
                                  const int64_t *target_len, int32_t n_targets, int32_t nthreads, int64_t mem_per_thread_mb,
                                  UvcRegionCut *out, int64_t capacity, int64_t *n_out) {
    if (!n_out || n < 0 || (n > 0 && (!tid || !pos || !endpos || !flag)) || nthreads < 1 || mem_per_thread_mb < 1) return fail(UVCGPU_EINVAL, "bad argument");
    uvcio_planner_t *p = nullptr;
    if (uvcio_planner_open(&p, target_len, target_len ? n_targets : 0, nthreads, mem_per_thread_mb)) return UVCGPU_EINVAL;
    uvcio_planner_feed(p, tid, pos, endpos, flag, n);
    uvcio_planner_finish(p);
    *n_out = uvcio_planner_pending(p);
    int rc = 0;
    if (*n_out > capacity || (!out && *n_out > 0)) rc = fail(UVCGPU_ENOMEM, "destination too small");
    else uvcio_planner_take(p, out, *n_out);
    uvcio_planner_close(p);
    return rc;
}

// ---- region shards: cost estimate, contiguous balanced partition, concatenation of the shard outputs ----
extern "C" int64_t uvcio_bam_region_bytes(const uvcio_bam_t *b, int32_t tid, int64_t beg, int64_t end) {
    if (!b || !b->has_index || tid < 0 || tid >= (int32_t)b->idx.size() || end <= beg) return 0;
    const std::vector<uint64_t> &lin = b->idx[(size_t)tid].linear;
    if (lin.empty()) return 0;
    // a virtual offset = compressed offset of the block << 16 | offset inside the inflated block; inside one block only the second part
    // moves (small files), so it counts too, at the usual ~4:1 ratio.  Windows without alignments carry offset 0 in files written by
    // some tools: take the nearest filled window in front.
    auto filled = [&](size_t w) { if (w >= lin.size()) w = lin.size() - 1; while (w > 0 && lin[w] == 0) w--; return (int64_t)(lin[w] >> 16) + (int64_t)(lin[w] & 0xFFFF) / 4; };
    // the index knows the offset of the first alignment that overlaps each 16 kb window: between two windows interpolate
    auto at = [&](int64_t p) { p = std::max<int64_t>(p, 0); const size_t w = (size_t)(p >> 14); const int64_t lo = filled(w), hi = std::max(lo, filled(w + 1)); return lo + (hi - lo) * (p & 16383) / 16384; };
    const int64_t a = at(beg), z = at(end);
    return z > a ? z - a : 0;
}
extern "C" int uvcio_plan_shards(const int64_t *cost, int64_t n, int32_t n_shards, int32_t *shard_of) {
    if (n < 0 || n_shards < 1 || (n > 0 && (!cost || !shard_of))) return fail(UVCGPU_EINVAL, "bad argument");
    long double total = 0;
    for (int64_t i = 0; i < n; i++) { if (cost[i] < 0) return fail(UVCGPU_EINVAL, "negative cost"); total += (long double)cost[i]; }
    long double run = 0;
    int32_t prev = 0;
    for (int64_t i = 0; i < n; i++) {
        int32_t s = (total > 0) ? (int32_t)(((run + (long double)cost[i] / 2) * n_shards) / total) : (int32_t)((i * n_shards) / std::max<int64_t>(n, 1));
        s = std::min(std::max(s, prev), n_shards - 1);
        shard_of[i] = s; prev = s; run += (long double)cost[i];
    }
    return 0;
}
// BED lines in file order -> the batches of consecutive lines that become one device region (uvc1-mi355x --merge-regions), see uvcio.h
extern "C" int uvcio_plan_bed_batches(const int32_t *tid, const int64_t *beg, const int64_t *end, int64_t n_lines, int64_t merge_distance, int64_t max_span,
                                      UvcBedPiece *out, int64_t capacity, int64_t *n_pieces) {
    if (n_lines < 0 || (n_lines > 0 && (!tid || !beg || !end)) || merge_distance < 0 || max_span < 1 || !n_pieces || capacity < 0 || (capacity > 0 && !out))
        return fail(UVCGPU_EINVAL, "plan_bed_batches: bad argument");
    int64_t n = 0, batch = -1, batch_beg = 0, prev_end = 0; int32_t batch_tid = -1;
    bool open = false;   // the last batch may take another line (it is not a piece of a cut line)
    auto put = [&](int64_t line, int64_t b, int64_t e) { if (n < capacity) out[n] = UvcBedPiece{ line, batch, b, e }; n++; };
    for (int64_t i = 0; i < n_lines; i++) {
        if (beg[i] < 0 || tid[i] < 0) return fail(UVCGPU_EINVAL, "plan_bed_batches: line " + std::to_string(i) + " has a negative begin or contig");
        if (end[i] <= beg[i]) continue;   // nothing to call
        if (end[i] - beg[i] > max_span) {   // cut into tiles as without merging; every piece is a batch of its own
            for (int64_t b = beg[i]; b < end[i]; b += max_span) { batch++; put(i, b, std::min(b + max_span, end[i])); }
            open = false;
            continue;
        }
        const bool joins = open && tid[i] == batch_tid && beg[i] >= prev_end + 1 && beg[i] - prev_end <= merge_distance && end[i] - batch_beg <= max_span;
        if (!joins) { batch++; batch_tid = tid[i]; batch_beg = beg[i]; open = true; }
        put(i, beg[i], end[i]);
        prev_end = end[i];
    }
    *n_pieces = n;
    return n > capacity ? fail(UVCGPU_ENOMEM, "plan_bed_batches: capacity too small") : 0;
}
extern "C" int uvcio_bgzf_concat(const char *out_path, const char *const *in_paths, int32_t n_in) {
    if (!out_path || n_in < 0 || (n_in > 0 && !in_paths)) return fail(UVCGPU_EINVAL, "bad argument");
    static const uint8_t eof_marker[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    FILE *fo = fopen(out_path, "wb");
    if (!fo) return fail(UVCGPU_EINVAL, std::string("cannot create ") + out_path);
    std::vector<uint8_t> buf;
    for (int32_t k = 0; k < n_in; k++) {
        FILE *fi = fopen(in_paths[k], "rb");
        if (!fi) { fclose(fo); return fail(UVCGPU_EINVAL, std::string("cannot open ") + in_paths[k]); }
        fseeko(fi, 0, SEEK_END); const int64_t sz = (int64_t)ftello(fi); fseeko(fi, 0, SEEK_SET);
        buf.resize((size_t)sz);
        if (sz && fread(buf.data(), 1, (size_t)sz, fi) != (size_t)sz) { fclose(fi); fclose(fo); return fail(UVCGPU_EINVAL, std::string("short read of ") + in_paths[k]); }
        fclose(fi);
        int64_t keep = sz;
        if (sz >= 28 && !memcmp(buf.data() + sz - 28, eof_marker, 28)) keep = sz - 28;
        if (keep && fwrite(buf.data(), 1, (size_t)keep, fo) != (size_t)keep) { fclose(fo); return fail(UVCGPU_EINVAL, "write failed"); }
    }
    const bool ok = (fwrite(eof_marker, 1, 28, fo) == 28);
    if (fclose(fo) != 0 || !ok) return fail(UVCGPU_EINVAL, "write failed");
    return 0;
}
extern "C" int uvcio_read_text_file(const char *path, char **out, int64_t *len) {
    if (!path || !out || !len) return fail(UVCGPU_EINVAL, "bad argument");
    gzFile g = gzopen(path, "rb");   // zlib reads multi-member gzip (= BGZF) and plain files alike
    if (!g) return fail(UVCGPU_EINVAL, std::string("cannot open ") + path);
    gzbuffer(g, 1 << 20);
    size_t cap = (size_t)1 << 22, n = 0;
    char *b = (char *)malloc(cap);
    if (!b) { gzclose(g); return fail(UVCGPU_ENOMEM, "malloc"); }
    for (;;) {
        if (cap - n < ((size_t)1 << 20)) { cap *= 2; char *nb = (char *)realloc(b, cap); if (!nb) { free(b); gzclose(g); return fail(UVCGPU_ENOMEM, "realloc"); } b = nb; }
        const int got = gzread(g, b + n, (unsigned)std::min<size_t>(cap - n - 1, (size_t)1 << 30));
        if (got < 0) { free(b); gzclose(g); return fail(UVCGPU_EINVAL, std::string("cannot inflate ") + path); }
        if (got == 0) break;
        n += (size_t)got;
    }
    gzclose(g);
    b[n] = 0; *out = b; *len = (int64_t)n;
    return 0;
}

// ---- the tumor VCF of a T/N pair: rescue_variants_from_vcf (main.cpp:183-398) on plain text ----
namespace {
struct TumorRec { int32_t tid; UvcTumorKey k; std::string col, ra; int64_t ord; };
}
struct uvcio_tumor_vcf {
    std::string sample;
    // a file-backed handle (uvcio_tumor_vcf_open): sorted once, never changed; fetch returns pointers into these vectors
    std::vector<int32_t> tid;                   // per record, parallel to keys
    std::vector<UvcTumorKey> keys;              // sorted by (tid, refpos, symbol); records of one key keep their file order
    std::vector<std::string> cols_text;         // sample column of each record
    std::vector<const char *> cols;             // c_str() of the above
    std::vector<std::string> ra_text;           // "REF\tALT" of each record (TumorKeyInfo::ref_alt)
    std::vector<const char *> ras;
    std::vector<int64_t> tid_first;             // [n_contigs + 1] first record of each tid
    // an in-memory store (uvcio_tumor_vcf_create): per tid, the records ordered by (refpos, symbol, add order); map nodes never move, so the
    // strings a fetch points at stay put while other threads add
    bool is_store = false;
    int32_t is_tumor_format_retrieved = 1;
    std::map<std::string, int32_t> tid_of;
    std::vector<std::map<std::tuple<int32_t, int32_t, int64_t>, TumorRec>> by_tid;
    int64_t n_added = 0;
    struct FetchBuf { std::vector<UvcTumorKey> keys; std::vector<const char *> cols, ras; };
    std::map<std::thread::id, FetchBuf> fetch_buf;   // what the last fetch of each thread returned
    mutable std::mutex mu;
};
namespace {
// the comma-separated integers of one FORMAT value ("." = missing -> none)
int parse_ints(const char *p, const char *e, int32_t *out, int cap) {
    int n = 0;
    while (p < e) {
        const char *q = p; while (q < e && *q != ',') q++;
        if (q - p == 1 && *p == '.') return -1;
        if (n < cap) out[n] = (int32_t)strtol(std::string(p, q).c_str(), nullptr, 10);
        n++;
        p = (q < e ? q + 1 : q);
    }
    return n;
}
// The record lines of `text` -> recs (ord = their index), in text order.  Header lines are skipped; `sample` (if not null)
// takes the last column of the #CHROM line.  Returns the error text ("" = none).
std::string parse_tumor_lines(const char *text, int64_t len, const std::map<std::string, int32_t> &tid_of, int32_t is_tumor_format_retrieved,
                              std::string *sample, std::vector<TumorRec> &recs) {
    std::string err;
    const char *p = text, *end = text + len;
    int64_t lineno = 0;
    while (p < end && err.empty()) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl : end;
        const char *line = p; p = nl ? nl + 1 : end; lineno++;
        if (le > line && le[-1] == '\r') le--;
        if (le == line) continue;
        if (line[0] == '#') {
            if (sample && le - line > 6 && !strncmp(line, "#CHROM", 6)) { const char *t = le; int tabs = 0; for (const char *q = line; q < le; q++) if (*q == '\t') tabs++; while (t > line && t[-1] != '\t') t--; *sample = (tabs >= 9 ? std::string(t, le) : std::string()); }
            continue;
        }
        const char *f[11]; int nf = 0; f[nf++] = line;
        for (const char *q = line; q < le && nf < 11; q++) if (*q == '\t') f[nf++] = q + 1;
        if (nf < 10) continue;   // no sample column: nothing to rescue
        auto fld = [&](int i) { return std::string(f[i], (i + 1 < nf ? f[i + 1] - 1 : le)); };
        const std::string chrom = fld(0), ref = fld(3), alt = fld(4), fmt = fld(8), smp = fld(9);
        auto ti = tid_of.find(chrom);
        if (ti == tid_of.end()) continue;   // a contig the BAM does not have can never be asked for
        // symbolic alleles: only <NON_REF> and <ADDITIONAL_INDEL_CANDIDATE> pass, and only when the tumor FORMAT is carried over (main.cpp:265-272)
        bool skip = false;
        {   size_t a = 0;
            while (a <= alt.size()) { size_t c = alt.find(',', a); if (c == std::string::npos) c = alt.size();
                const std::string one = alt.substr(a, c - a);
                if (!one.empty() && one[0] == '<' && ((one != "<NON_REF>" && one != "<ADDITIONAL_INDEL_CANDIDATE>") || !is_tumor_format_retrieved)) skip = true;
                a = c + 1; } }
        if (skip) continue;
        // FORMAT keys -> sample values
        std::vector<std::pair<const char *, const char *>> keys, vals;
        { const char *a = fmt.data(), *z = a + fmt.size(); while (a <= z) { const char *c = a; while (c < z && *c != ':') c++; keys.emplace_back(a, c); a = c + 1; } }
        { const char *a = smp.data(), *z = a + smp.size(); while (a <= z) { const char *c = a; while (c < z && *c != ':') c++; vals.emplace_back(a, c); a = c + 1; } }
        auto get = [&](const char *name, int32_t *dst, int cap) -> int {   // number of values, 0 = tag absent, -1 = "."
            const size_t nl2 = strlen(name);
            for (size_t k = 0; k < keys.size() && k < vals.size(); k++) if ((size_t)(keys[k].second - keys[k].first) == nl2 && !memcmp(keys[k].first, name, nl2)) return parse_ints(vals[k].first, vals[k].second, dst, cap);
            return 0;
        };
        int32_t a2[4];
        if (get("VTI", a2, 4) != 2) continue;   // valsize <= 0 -> continue (main.cpp:275)
        TumorRec r; memset(&r.k, 0, sizeof(r.k));
        r.tid = ti->second; r.ord = (int64_t)recs.size(); r.col = smp; r.ra = ref + "\t" + alt;
        const int symbol = a2[1];
        const long pos0 = strtol(fld(1).c_str(), nullptr, 10) - 1;   // line->pos
        const bool at_pos = (symbol <= UVC_BASE_NN || symbol == UVC_MGVCF_SYMBOL || symbol == UVC_ADDITIONAL_INDEL_CANDIDATE_SYMBOL);   // isSymbolSubstitution covers BASE_A .. BASE_NN
        r.k.refpos = (int32_t)(at_pos ? pos0 : pos0 + 1); r.k.symbol = symbol;
        if (symbol != UVC_MGVCF_SYMBOL && symbol != UVC_ADDITIONAL_INDEL_CANDIDATE_SYMBOL) {
            auto need = [&](const char *name, int n_expect, int32_t *dst) { if (get(name, dst, 4) != n_expect && err.empty()) err = std::string("FORMAT/") + name + " of line " + std::to_string(lineno) + " does not have " + std::to_string(n_expect) + " integers (main.cpp:294-372 asserts it)"; };
            need("BDPb", 2, a2); r.k.BDP = a2[0] + a2[1];
            need("bDPf", 2, a2); r.k.bDP = a2[1]; need("bDPr", 2, a2); r.k.bDP += a2[1];
            need("CDP1x", 1, a2); r.k.CDP1x = a2[0]; need("cDP1x", 2, a2); r.k.cDP1x = a2[1];
            need("cVQ1", 2, a2); r.k.cVQ1 = a2[1]; need("cPCQ1", 2, a2); r.k.cPCQ1 = a2[1];
            need("CDP2x", 1, a2); r.k.CDP2x = a2[0]; need("cDP2x", 2, a2); r.k.cDP2x = a2[1];
            need("cVQ2", 2, a2); r.k.cVQ2 = a2[1]; need("cPCQ2", 2, a2); r.k.cPCQ2 = a2[1];
            need("bNMQ", 2, a2); r.k.bNMQ = a2[1]; need("vHGQ", 1, a2); r.k.vHGQ = a2[0];
            need("CDP1b", 2, a2); r.k.tDP = a2[0] + a2[1];
            need("cDP1f", 2, a2); r.k.tAD0 = a2[0]; r.k.tAD1 = a2[1]; need("cDP1r", 2, a2); r.k.tAD0 += a2[0]; r.k.tAD1 += a2[1];
            need("CDP2b", 2, a2); r.k.t2DP = a2[0] + a2[1];
            if (symbol >= UVC_LINK_D3P && symbol <= UVC_LINK_I1)   // the InDel string of the record: REF / ALT without their common head (main.cpp:867-880)
                r.k.indel_len = (int32_t)(ref.size() > alt.size() ? ref.size() - alt.size() : alt.size() - ref.size());
        }
        for (size_t k = 0; k < keys.size(); k++) if ((keys[k].second - keys[k].first) == 5 && !memcmp(keys[k].first, "_C2XP", 5)) r.k.tier2 = 1;   // enable_tier2_consensus_format_tags, main.cpp:386-388
        recs.push_back(std::move(r));
    }
    return err;
}
}
extern "C" int uvcio_tumor_vcf_open(uvcio_tumor_vcf_t **out, const char *path, const char *const *contig_names, int32_t n_contigs, int32_t is_tumor_format_retrieved) {
    if (!out || !path || n_contigs < 0 || (n_contigs > 0 && !contig_names)) return fail(UVCGPU_EINVAL, "bad argument");
    char *text = nullptr; int64_t len = 0;
    int rc = uvcio_read_text_file(path, &text, &len);
    if (rc) return rc;
    std::map<std::string, int32_t> tid_of;
    for (int32_t i = 0; i < n_contigs; i++) tid_of[contig_names[i]] = i;
    uvcio_tumor_vcf *v = new uvcio_tumor_vcf();
    std::vector<TumorRec> recs;
    const std::string err = parse_tumor_lines(text, len, tid_of, is_tumor_format_retrieved, &v->sample, recs);
    free(text);
    if (!err.empty()) { delete v; return fail(UVCGPU_EINVAL, err); }
    std::stable_sort(recs.begin(), recs.end(), [](const TumorRec &a, const TumorRec &b) {
        if (a.tid != b.tid) return a.tid < b.tid;
        if (a.k.refpos != b.k.refpos) return a.k.refpos < b.k.refpos;
        return a.k.symbol < b.k.symbol; });
    v->tid_first.assign((size_t)n_contigs + 1, 0);
    for (const TumorRec &r : recs) { v->tid.push_back(r.tid); v->keys.push_back(r.k); v->cols_text.push_back(r.col); v->ra_text.push_back(r.ra); v->tid_first[(size_t)r.tid + 1]++; }
    for (int32_t i = 0; i < n_contigs; i++) v->tid_first[(size_t)i + 1] += v->tid_first[(size_t)i];
    for (const std::string &s : v->cols_text) v->cols.push_back(s.c_str());
    for (const std::string &s : v->ra_text) v->ras.push_back(s.c_str());
    *out = v;
    return 0;
}
extern "C" int uvcio_tumor_vcf_create(uvcio_tumor_vcf_t **out, const char *sample_name, const char *const *contig_names, int32_t n_contigs, int32_t is_tumor_format_retrieved) {
    if (!out || n_contigs < 0 || (n_contigs > 0 && !contig_names)) return fail(UVCGPU_EINVAL, "bad argument");
    uvcio_tumor_vcf *v = new uvcio_tumor_vcf();
    v->is_store = true; v->is_tumor_format_retrieved = is_tumor_format_retrieved;
    v->sample = sample_name ? sample_name : "";
    for (int32_t i = 0; i < n_contigs; i++) v->tid_of[contig_names[i]] = i;
    v->by_tid.resize((size_t)n_contigs);
    *out = v;
    return 0;
}
extern "C" int uvcio_tumor_vcf_add_lines(uvcio_tumor_vcf_t *v, const char *text, int64_t len) {
    if (!v || !v->is_store || len < 0 || (len > 0 && !text)) return fail(UVCGPU_EINVAL, "bad argument");
    std::vector<TumorRec> recs;   // parsed outside the lock; `ord` is assigned under it
    const std::string err = parse_tumor_lines(text, len, v->tid_of, v->is_tumor_format_retrieved, nullptr, recs);
    if (!err.empty()) return fail(UVCGPU_EINVAL, err);
    std::lock_guard<std::mutex> g(v->mu);
    const int64_t base = v->n_added;
    for (TumorRec &r : recs) {
        r.ord += base;
        v->by_tid[(size_t)r.tid].emplace(std::make_tuple(r.k.refpos, r.k.symbol, r.ord), std::move(r));
    }
    v->n_added += (int64_t)recs.size();
    return 0;
}
extern "C" const char *uvcio_tumor_vcf_sample_name(const uvcio_tumor_vcf_t *v) { return v ? v->sample.c_str() : ""; }
extern "C" int64_t uvcio_tumor_vcf_n_records(const uvcio_tumor_vcf_t *v) {
    if (!v) return 0;
    if (!v->is_store) return (int64_t)v->keys.size();
    std::lock_guard<std::mutex> g(v->mu);
    return v->n_added;
}
extern "C" int uvcio_tumor_vcf_fetch(const uvcio_tumor_vcf_t *v, int32_t tid, int32_t pos_beg, int32_t pos_end, const UvcTumorKey **keys, const char *const **cols, const char *const **ref_alts, int64_t *n) {
    if (!v || !n) return fail(UVCGPU_EINVAL, "bad argument");
    *n = 0; if (keys) *keys = nullptr; if (cols) *cols = nullptr; if (ref_alts) *ref_alts = nullptr;
    if (v->is_store) {   // a copy into this thread's buffers of the handle: the maps may grow under other threads
        uvcio_tumor_vcf *w = const_cast<uvcio_tumor_vcf *>(v);
        std::lock_guard<std::mutex> g(w->mu);
        if (tid < 0 || (size_t)tid >= w->by_tid.size()) return 0;
        uvcio_tumor_vcf::FetchBuf &fb = w->fetch_buf[std::this_thread::get_id()];
        fb.keys.clear(); fb.cols.clear(); fb.ras.clear();
        const auto &m = w->by_tid[(size_t)tid];
        for (auto it = m.lower_bound(std::make_tuple(pos_beg, INT32_MIN, INT64_MIN)); it != m.end() && std::get<0>(it->first) <= pos_end; ++it) {
            fb.keys.push_back(it->second.k); fb.cols.push_back(it->second.col.c_str()); fb.ras.push_back(it->second.ra.c_str());
        }
        *n = (int64_t)fb.keys.size();
        if (*n > 0) { if (keys) *keys = fb.keys.data(); if (cols) *cols = fb.cols.data(); if (ref_alts) *ref_alts = fb.ras.data(); }
        return 0;
    }
    if (tid < 0 || (size_t)tid + 1 >= v->tid_first.size()) return 0;
    const int64_t lo0 = v->tid_first[(size_t)tid], hi0 = v->tid_first[(size_t)tid + 1];
    const auto b = v->keys.begin();
    const int64_t lo = std::lower_bound(b + lo0, b + hi0, pos_beg, [](const UvcTumorKey &k, int32_t p) { return k.refpos < p; }) - b;
    const int64_t hi = std::upper_bound(b + lo, b + hi0, pos_end, [](int32_t p, const UvcTumorKey &k) { return p < k.refpos; }) - b;
    *n = hi - lo;
    if (*n > 0) { if (keys) *keys = v->keys.data() + lo; if (cols) *cols = v->cols.data() + lo; if (ref_alts) *ref_alts = v->ras.data() + lo; }
    return 0;
}
extern "C" void uvcio_tumor_vcf_close(uvcio_tumor_vcf_t *v) { delete v; }

// ---- force-output sites (uvc1-mi355x --force-sites): a BED or a VCF reduced to (tid, zerobased_pos) ----
struct uvcio_sites {
    std::vector<int32_t> pos;         // zerobased_pos values, sorted and unique within a contig
    std::vector<int64_t> tid_first;   // [n_contigs + 1] first site of each tid
};
namespace {
bool parse_nonneg(const std::string &t, int64_t &v) {
    if (t.empty() || t.size() > 18) return false;
    v = 0;
    for (char c : t) { if (c < '0' || c > '9') return false; v = v * 10 + (c - '0'); }
    return true;
}
std::string sites_parse(const char *text, int64_t len, const std::string &path, const std::map<std::string, int32_t> &tid_of, std::vector<std::pair<int32_t, int32_t>> &out) {
    // VCF: the first line is ##fileformat=VCF... or #CHROM (what every VCF writer puts first); anything else is read as BED
    const bool vcf = (len >= 12 && !strncmp(text, "##fileformat", 12)) || (len >= 6 && !strncmp(text, "#CHROM", 6));
    const int64_t max_sites = (int64_t)1 << 30;
    int64_t lineno = 0, n_expanded = 0;
    for (int64_t at = 0; at < len;) {
        const char *nl = (const char *)memchr(text + at, '\n', (size_t)(len - at));
        const int64_t e = nl ? nl - text : len;
        std::string line(text + at, (size_t)(e - at));
        at = e + 1; lineno++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        if (!vcf && (!line.compare(0, 5, "track") || !line.compare(0, 7, "browser"))) continue;
        std::vector<std::string> f;
        for (size_t p = 0; p <= line.size() && f.size() < 3;) {   // VCF: tab-separated; BED: tabs or blanks
            size_t q = p;
            while (q < line.size() && line[q] != '\t' && (vcf || line[q] != ' ')) q++;
            if (q > p || vcf) f.push_back(line.substr(p, q - p));
            p = q + 1;
            while (!vcf && p < line.size() && line[p] == ' ') p++;
        }
        const std::string where = path + " line " + std::to_string(lineno) + ": ";
        if (f.size() < (vcf ? 2u : 3u)) return where + (vcf ? "a VCF record needs CHROM and POS" : "a BED line needs chrom, start and end");
        const auto it = tid_of.find(f[0]);
        if (it == tid_of.end()) return where + "contig '" + f[0] + "' is not in the BAM header";
        if (vcf) {
            int64_t p = 0;
            if (!parse_nonneg(f[1], p) || p < 1 || p > INT32_MAX - 1) return where + "POS '" + f[1] + "' is not a positive integer";
            out.emplace_back(it->second, (int32_t)p);                  // VCF POS p = the records of zerobased_pos p
            n_expanded++;
        } else {
            int64_t b = 0, en = 0;
            if (!parse_nonneg(f[1], b) || !parse_nonneg(f[2], en) || b > en || en > INT32_MAX - 1) return where + "start '" + f[1] + "' and end '" + f[2] + "' are not 0 <= start <= end";
            n_expanded += en - b;
            if (n_expanded > max_sites) return where + "more than 2^30 sites in all";
            for (int64_t x = b; x < en; x++) out.emplace_back(it->second, (int32_t)(x + 1));   // base x (0-based) = VCF POS x + 1
        }
    }
    return std::string();
}
}
extern "C" int uvcio_sites_open(uvcio_sites_t **out, const char *path, const char *const *contig_names, int32_t n_contigs) {
    if (!out || !path || n_contigs < 0 || (n_contigs > 0 && !contig_names)) return fail(UVCGPU_EINVAL, "bad argument");
    *out = nullptr;
    char *text = nullptr; int64_t len = 0;
    int rc = uvcio_read_text_file(path, &text, &len);
    if (rc) return rc;
    std::map<std::string, int32_t> tid_of;
    for (int32_t i = 0; i < n_contigs; i++) tid_of[contig_names[i]] = i;
    std::vector<std::pair<int32_t, int32_t>> s;
    const std::string err = sites_parse(text, len, path, tid_of, s);
    free(text);
    if (!err.empty()) return fail(UVCGPU_EINVAL, err);
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    uvcio_sites *v = new uvcio_sites();
    v->tid_first.assign((size_t)n_contigs + 1, 0);
    for (const auto &p : s) { v->pos.push_back(p.second); v->tid_first[(size_t)p.first + 1]++; }
    for (int32_t i = 0; i < n_contigs; i++) v->tid_first[(size_t)i + 1] += v->tid_first[(size_t)i];
    *out = v;
    return 0;
}
extern "C" int64_t uvcio_sites_count(const uvcio_sites_t *v) { return v ? (int64_t)v->pos.size() : 0; }
extern "C" int uvcio_sites_fetch(const uvcio_sites_t *v, int32_t tid, int64_t pos_beg, int64_t pos_end, const int32_t **sites, int64_t *n) {
    if (!v || !sites || !n) return fail(UVCGPU_EINVAL, "bad argument");
    *sites = nullptr; *n = 0;
    if (tid < 0 || (size_t)tid + 1 >= v->tid_first.size() || pos_end <= pos_beg) return 0;
    const int32_t *b = v->pos.data() + v->tid_first[(size_t)tid], *e = v->pos.data() + v->tid_first[(size_t)tid + 1];
    const int32_t *lo = std::lower_bound(b, e, (int64_t)std::max<int64_t>(pos_beg, INT32_MIN), [](int32_t a, int64_t k) { return (int64_t)a < k; });
    const int32_t *hi = std::lower_bound(lo, e, (int64_t)std::min<int64_t>(pos_end, (int64_t)INT32_MAX + 1), [](int32_t a, int64_t k) { return (int64_t)a < k; });
    *sites = lo; *n = hi - lo;
    return 0;
}
extern "C" void uvcio_sites_close(uvcio_sites_t *v) { delete v; }

// ---------------------------------------------------------------- the report stores ----
// What the stores of --coverage-out, --error-profile-out, --family-stats-out, --callable-out, --read-profile-out, --msi-out, --fragment-profile-out and --site-reads-out share: a store collects what the tiles
// report under its mutex and writes the whole file at the end.
// a target as the stores with target lines keep it; a BED line without a name is "."
struct ReportTarget { std::string chrom, name; int64_t beg, end; };
static ReportTarget report_target(const char *chrom, const char *name, int64_t beg, int64_t end) { return ReportTarget{ chrom, (name && *name) ? name : ".", beg, end }; }
// `text` as the file `path`, block-gzipped when the name ends in .gz
static int write_text(const char *path, const std::string &text) {
    const std::string p = path;
    if (p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0) {
        uvcio_bgzf_writer_t *zw = nullptr;
        if (uvcio_bgzf_write_open(&zw, path, 6)) return fail(UVCGPU_EINVAL, std::string("cannot create ") + path);
        const int rc = uvcio_bgzf_write(zw, text.data(), (int64_t)text.size());
        const int rc2 = uvcio_bgzf_write_close(zw);
        if (rc || rc2) return fail(UVCGPU_EINVAL, std::string("cannot write ") + path);
        return 0;
    }
    FILE *fo = fopen(path, "wb");
    if (!fo) return fail(UVCGPU_EINVAL, std::string("cannot create ") + path);
    const bool ok = (fwrite(text.data(), 1, text.size(), fo) == text.size());
    if (fclose(fo) != 0 || !ok) return fail(UVCGPU_EINVAL, std::string("cannot write ") + path);
    return 0;
}

// ---------------------------------------------------------------- the per-target coverage report ----
struct uvcio_coverage {
    std::vector<std::string> measures; std::vector<int32_t> thr;
    struct Target : ReportTarget { int64_t len, covered; };
    std::vector<Target> targets;
    std::vector<int64_t> rows;   // [target][measure][3 + n_thr]: sum, min, max, counts
    std::mutex mu;
    size_t width() const { return measures.size() * (3 + thr.size()); }
};
extern "C" int uvcio_coverage_open(uvcio_coverage_t **out, const char *const *measure_names, int32_t n_measures, const int32_t *thresholds, int32_t n_thresholds) {
    if (!out || !measure_names || n_measures < 1 || n_thresholds < 0 || n_thresholds > 8 || (n_thresholds > 0 && !thresholds)) return fail(UVCGPU_EINVAL, "coverage report: bad argument");
    uvcio_coverage *c = new uvcio_coverage;
    for (int32_t m = 0; m < n_measures; m++) c->measures.push_back(measure_names[m] ? measure_names[m] : "");
    c->thr.assign(thresholds, thresholds + n_thresholds);
    *out = c;
    return 0;
}
extern "C" int64_t uvcio_coverage_add_target(uvcio_coverage_t *c, const char *chrom, int64_t beg, int64_t end, const char *name, int64_t len) {
    if (!c || !chrom || len < 0) return fail(UVCGPU_EINVAL, "coverage report: bad target");
    std::lock_guard<std::mutex> g(c->mu);
    c->targets.push_back(uvcio_coverage::Target{ report_target(chrom, name, beg, end), len, 0 });
    c->rows.resize(c->targets.size() * c->width(), 0);
    return (int64_t)c->targets.size() - 1;
}
extern "C" int uvcio_coverage_add_piece(uvcio_coverage_t *c, int64_t target, int64_t piece_len, const int64_t *row) {
    if (!c || !row || piece_len < 1) return fail(UVCGPU_EINVAL, "coverage report: bad piece");
    std::lock_guard<std::mutex> g(c->mu);
    if (target < 0 || target >= (int64_t)c->targets.size()) return fail(UVCGPU_EINVAL, "coverage report: piece of target " + std::to_string(target) + ", which does not exist");
    uvcio_coverage::Target &t = c->targets[(size_t)target];
    if (t.covered + piece_len > t.len) return fail(UVCGPU_EINVAL, "coverage report: the pieces of target " + std::to_string(target) + " are longer than the target (pieces must be disjoint)");
    const size_t nt = c->thr.size(), w = 3 + nt;
    int64_t *dst = &c->rows[(size_t)target * c->width()];
    for (size_t m = 0; m < c->measures.size(); m++) {
        const int64_t *src = row + m * 11;
        dst[m * w + 0] += src[0];
        dst[m * w + 1] = (t.covered == 0 ? src[1] : std::min(dst[m * w + 1], src[1]));
        dst[m * w + 2] = (t.covered == 0 ? src[2] : std::max(dst[m * w + 2], src[2]));
        for (size_t k = 0; k < nt; k++) dst[m * w + 3 + k] += src[3 + k];
    }
    t.covered += piece_len;
    return 0;
}
extern "C" int uvcio_coverage_write(const uvcio_coverage_t *c, const char *path) {
    if (!c || !path || !*path) return fail(UVCGPU_EINVAL, "coverage report: bad argument");
    std::string text = "#chrom\tbeg\tend\tname\tlen";
    for (const std::string &m : c->measures) {
        text += "\t" + m + "_sum\t" + m + "_min\t" + m + "_max";
        for (int32_t t : c->thr) text += "\t" + m + "_ge" + std::to_string(t);
    }
    text += "\n";
    const size_t nt = c->thr.size(), w = 3 + nt;
    for (size_t q = 0; q < c->targets.size(); q++) {
        const uvcio_coverage::Target &t = c->targets[q];
        text += t.chrom + "\t" + std::to_string(t.beg) + "\t" + std::to_string(t.end) + "\t" + t.name + "\t" + std::to_string(t.len);
        const int64_t *row = &c->rows[q * c->width()];
        const int64_t bare = t.len - t.covered;   // positions no tile reported: depth 0
        for (size_t m = 0; m < c->measures.size(); m++) {
            text += "\t" + std::to_string(row[m * w]) + "\t" + std::to_string(bare > 0 ? std::min<int64_t>(row[m * w + 1], 0) : row[m * w + 1]) + "\t" + std::to_string(row[m * w + 2]);
            for (size_t k = 0; k < nt; k++) text += "\t" + std::to_string(row[m * w + 3 + k] + (c->thr[k] <= 0 ? bare : 0));
        }
        text += "\n";
    }
    return write_text(path, text);
}
extern "C" void uvcio_coverage_close(uvcio_coverage_t *c) { delete c; }

// ---------------------------------------------------------------- the background error profile ----
// the row layout is that of uvcgpu_region_error_profile (UVC_ERR_*, UvcErrCounter of uvcgpu.h); the reserved counter is not written
enum { EP_NCOUNTERS = UVC_ERRC_no_context + 1 };
struct uvcio_errprofile {
    std::vector<std::string> levels; int32_t min_depth, max_alt_permille;
    std::vector<int64_t> sum;   // [level][UVC_ERR_ROW]
    std::mutex mu;
};
extern "C" int uvcio_errprofile_open(uvcio_errprofile_t **out, const char *const *level_names, int32_t n_levels, int32_t min_depth, int32_t max_alt_permille) {
    if (!out || !level_names || n_levels < 1) return fail(UVCGPU_EINVAL, "error profile: bad argument");
    uvcio_errprofile *e = new uvcio_errprofile;
    for (int32_t l = 0; l < n_levels; l++) e->levels.push_back(level_names[l] ? level_names[l] : "");
    e->min_depth = min_depth; e->max_alt_permille = max_alt_permille;
    e->sum.assign((size_t)n_levels * UVC_ERR_ROW, 0);
    *out = e;
    return 0;
}
extern "C" int uvcio_errprofile_add(uvcio_errprofile_t *e, const int64_t *profile) {
    if (!e || !profile) return fail(UVCGPU_EINVAL, "error profile: bad argument");
    std::lock_guard<std::mutex> g(e->mu);
    for (size_t i = 0; i < e->sum.size(); i++) e->sum[i] += profile[i];
    return 0;
}
extern "C" int uvcio_errprofile_write(const uvcio_errprofile_t *e, const char *path) {
    if (!e || !path || !*path) return fail(UVCGPU_EINVAL, "error profile: bad argument");
    static const char *const COUNTERS[EP_NCOUNTERS] = { "BASE_counted", "BASE_low_depth", "BASE_high_alt", "LINK_counted", "LINK_low_depth", "LINK_high_alt", "no_context" };
    static const char *const BASE_SYM[UVC_ERR_NBASE] = { "A", "C", "G", "T" };
    static const char *const LINK_SYM[UVC_ERR_NLINK] = { "M", "D3P", "D2", "D1", "I3P", "I2", "I1" };
    std::string text = "##error_profile_min_depth=" + std::to_string(e->min_depth) + "\n##error_profile_max_alt_permille=" + std::to_string(e->max_alt_permille) + "\n#level\tcounter\tcount\n";
    for (size_t l = 0; l < e->levels.size(); l++)
        for (int k = 0; k < EP_NCOUNTERS; k++) text += e->levels[l] + "\t" + COUNTERS[k] + "\t" + std::to_string(e->sum[l * UVC_ERR_ROW + UVC_ERR_COUNTERS + k]) + "\n";
    text += "#level\tkind\tcontext\tsymbol\tcount\tref_count\n";
    for (size_t l = 0; l < e->levels.size(); l++)
        for (int kind = 0; kind < 2; kind++) {
            const int n = (kind == 0 ? UVC_ERR_NBASE : UVC_ERR_NLINK);
            const int64_t *bins = &e->sum[l * UVC_ERR_ROW + (kind == 0 ? 0 : UVC_ERR_LINK_BINS)];
            for (int ctx = 0; ctx < UVC_ERR_NCTX; ctx++) {
                const int64_t *b = bins + ctx * n;
                bool any = false;
                for (int j = 0; j < n; j++) any = any || b[j] != 0;
                if (!any) continue;
                const int ref = (kind == 0 ? (ctx >> 2) & 3 : 0);
                const std::string head = e->levels[l] + (kind == 0 ? "\tBASE\t" : "\tLINK\t") + BASE_SYM[ctx >> 4] + BASE_SYM[(ctx >> 2) & 3] + BASE_SYM[ctx & 3] + "\t";
                for (int j = 0; j < n; j++) text += head + (kind == 0 ? BASE_SYM[j] : LINK_SYM[j]) + "\t" + std::to_string(b[j]) + "\t" + std::to_string(b[ref]) + "\n";
            }
        }
    return write_text(path, text);
}
extern "C" void uvcio_errprofile_close(uvcio_errprofile_t *e) { delete e; }

// ---------------------------------------------------------------- the family concordance report ----
// the row layout is that of uvcgpu_region_family_concordance (UVC_FAMCONC_* of uvcgpu.h, include/uvc_famconcord.def); the reserved counters are not written
struct uvcio_famconcord {
    std::vector<int64_t> sum;   // [UVC_FAMCONC_ROW]
    std::mutex mu;
};
extern "C" int uvcio_famconcord_open(uvcio_famconcord_t **out) {
    if (!out) return fail(UVCGPU_EINVAL, "family concordance report: bad argument");
    uvcio_famconcord *f = new uvcio_famconcord;
    f->sum.assign((size_t)UVC_FAMCONC_ROW, 0);
    *out = f;
    return 0;
}
extern "C" int uvcio_famconcord_add(uvcio_famconcord_t *f, const int64_t *row) {
    if (!f || !row) return fail(UVCGPU_EINVAL, "family concordance report: bad argument");
    std::lock_guard<std::mutex> g(f->mu);
    for (size_t i = 0; i < f->sum.size(); i++) f->sum[i] += row[i];
    return 0;
}
extern "C" int uvcio_famconcord_write(const uvcio_famconcord_t *f, const char *path) {
    if (!f || !path || !*path) return fail(UVCGPU_EINVAL, "family concordance report: bad argument");
    static const struct { const char *name; int first, words; } SECTIONS[] = {
#define UVC_FAMCONC(name, first, words) { #name, first, words },
#include "uvc_famconcord.def"
#undef UVC_FAMCONC
    };
    static const char *const COUNTERS[UVC_FAMCONCC_reserved] = { "units_seen", "unit_positions", "base_no_vote", "link_no_vote", "base_no_ref", "duplex_no_vote", "duplex_base_no_ref" };
    static const char *const BINS[UVC_FAMCONC_NBIN] = { "1", "2", "3", "4", "5-7", "8-15", "16-31", "32+" };
    static const char *const BASE_SYM[UVC_FAMCONC_NBASE + 1] = { "A", "C", "G", "T", "N", "NN", "NONE" };
    static const char *const LINK_SYM[UVC_FAMCONC_NLINK + 1] = { "M", "D3P", "D2", "D1", "I3P", "I2", "I1", "NN", "NONE" };
    static const char *const REFCLASS[2] = { "REF", "ALT" };
    const int64_t *v = f->sum.data();
    const int NB = UVC_FAMCONC_NBASE, NL = UVC_FAMCONC_NLINK, NK = UVC_FAMCONC_NBIN;
    std::string text = "##family_concordance_sections=";
    for (size_t k = 0; k < sizeof(SECTIONS) / sizeof(SECTIONS[0]); k++) text += std::string(k ? "," : "") + SECTIONS[k].name + ":" + std::to_string(SECTIONS[k].first) + ":" + std::to_string(SECTIONS[k].words);
    text += "\n##family_concordance_bins=";
    for (int k = 0; k < NK; k++) text += std::string(k ? "," : "") + BINS[k];
    text += "\n#counter\tcount\n";
    for (int k = 0; k < UVC_FAMCONCC_reserved; k++) text += std::string(COUNTERS[k]) + "\t" + std::to_string(v[UVC_FAMCONC_COUNTERS + k]) + "\n";
    text += "#summary\tkind\tbin\tminority_votes\tvotes\n";
    for (int k = 0; k < NK; k++) {   // the minority share of a bin as two integers
        int64_t all = 0, diag = 0;
        for (int rc = 0; rc < 2; rc++) for (int cs = 0; cs < NB; cs++) for (int s = 0; s < NB; s++) {
            const int64_t c = v[UVC_FAMCONC_BASE + ((rc * NK + k) * NB + cs) * NB + s];
            all += c; if (cs == s) diag += c;
        }
        text += std::string("#summary\tBASE\t") + BINS[k] + "\t" + std::to_string(all - diag) + "\t" + std::to_string(all) + "\n";
    }
    for (int k = 0; k < NK; k++) {
        int64_t all = 0, diag = 0;
        for (int cs = 0; cs < NL; cs++) for (int s = 0; s < NL; s++) { const int64_t c = v[UVC_FAMCONC_LINK + (k * NL + cs) * NL + s]; all += c; if (cs == s) diag += c; }
        text += std::string("#summary\tLINK\t") + BINS[k] + "\t" + std::to_string(all - diag) + "\t" + std::to_string(all) + "\n";
    }
    text += "#BASE\trefclass\tbin\tconsensus\tvote\tcount\n#BASE_POS\trefclass\tbin\tpositions\tunanimous\n#LINK\tbin\tconsensus\tvote\tcount\n#LINK_POS\tbin\tpositions\tunanimous\n"
            "#DUPLEX_BASE\tref\tstrand0\tstrand1\tcount\n#DUPLEX_LINK\tstrand0\tstrand1\tcount\n";
    for (int rc = 0; rc < 2; rc++) for (int k = 0; k < NK; k++) for (int cs = 0; cs < NB; cs++) for (int s = 0; s < NB; s++) {
        const int64_t c = v[UVC_FAMCONC_BASE + ((rc * NK + k) * NB + cs) * NB + s];
        if (c) text += std::string("BASE\t") + REFCLASS[rc] + "\t" + BINS[k] + "\t" + BASE_SYM[cs] + "\t" + BASE_SYM[s] + "\t" + std::to_string(c) + "\n";
    }
    for (int rc = 0; rc < 2; rc++) for (int k = 0; k < NK; k++) {
        const int64_t *c = v + UVC_FAMCONC_BASE_POS + (rc * NK + k) * 2;
        if (c[0] || c[1]) text += std::string("BASE_POS\t") + REFCLASS[rc] + "\t" + BINS[k] + "\t" + std::to_string(c[0]) + "\t" + std::to_string(c[1]) + "\n";
    }
    for (int k = 0; k < NK; k++) for (int cs = 0; cs < NL; cs++) for (int s = 0; s < NL; s++) {
        const int64_t c = v[UVC_FAMCONC_LINK + (k * NL + cs) * NL + s];
        if (c) text += std::string("LINK\t") + BINS[k] + "\t" + LINK_SYM[cs] + "\t" + LINK_SYM[s] + "\t" + std::to_string(c) + "\n";
    }
    for (int k = 0; k < NK; k++) {
        const int64_t *c = v + UVC_FAMCONC_LINK_POS + k * 2;
        if (c[0] || c[1]) text += std::string("LINK_POS\t") + BINS[k] + "\t" + std::to_string(c[0]) + "\t" + std::to_string(c[1]) + "\n";
    }
    for (int r = 0; r < 4; r++) for (int a = 0; a <= NB; a++) for (int b = 0; b <= NB; b++) {
        const int64_t c = v[UVC_FAMCONC_DUP_BASE + (r * (NB + 1) + a) * (NB + 1) + b];
        if (c) text += std::string("DUPLEX_BASE\t") + BASE_SYM[r] + "\t" + BASE_SYM[a] +"\t" + BASE_SYM[b] + "\t" + std::to_string(c) + "\n";
    }
    for (int a = 0; a <= NL; a++) for (int b = 0; b <= NL; b++) {
        const int64_t c = v[UVC_FAMCONC_DUP_LINK + a * (NL + 1) + b];
        if (c) text += std::string("DUPLEX_LINK\t") + LINK_SYM[a] + "\t" + LINK_SYM[b] + "\t" + std::to_string(c) + "\n";
    }
    return write_text(path, text);
}
extern "C" void uvcio_famconcord_close(uvcio_famconcord_t *f) { delete f; }

// ---------------------------------------------------------------- the read profile ----
// the row layout is that of uvcgpu_region_read_profile (UVC_READPROF_* of uvcgpu.h, include/uvc_readprofile.def); the reserved words are not written
struct uvcio_readprofile {
    std::string classes[UVC_READPROF_NCLASS]; int32_t min_mapq, min_depth, max_alt_permille;
    int64_t sum[UVC_READPROF_ROW];
    std::mutex mu;
};
extern "C" int uvcio_readprofile_open(uvcio_readprofile_t **out, const char *const *class_names, int32_t min_mapq, int32_t min_depth, int32_t max_alt_permille) {
    if (!out || !class_names) return fail(UVCGPU_EINVAL, "read profile: bad argument");
    uvcio_readprofile *p = new uvcio_readprofile;
    for (int c = 0; c < UVC_READPROF_NCLASS; c++) p->classes[c] = class_names[c] ? class_names[c] : "";
    p->min_mapq = min_mapq; p->min_depth = min_depth; p->max_alt_permille = max_alt_permille;
    memset(p->sum, 0, sizeof(p->sum));
    *out = p;
    return 0;
}
extern "C" int uvcio_readprofile_add(uvcio_readprofile_t *p, const int64_t *row) {
    if (!p || !row) return fail(UVCGPU_EINVAL, "read profile: bad argument");
    std::lock_guard<std::mutex> g(p->mu);
    for (int i = 0; i < UVC_READPROF_ROW; i++) p->sum[i] += row[i];
    return 0;
}
extern "C" int uvcio_readprofile_write(const uvcio_readprofile_t *p, const char *path) {
    if (!p || !path || !*path) return fail(UVCGPU_EINVAL, "read profile: bad argument");
    static const char *const COUNTERS[] = {
#define UVC_READPROF(name, first, words) #name,
#include "uvc_readprofile.def"
#undef UVC_READPROF
    };
    static const char *const BASE_SYM[4] = { "A", "C", "G", "T" };
    std::string text = "##read_profile_min_mapq=" + std::to_string(p->min_mapq) + "\n##read_profile_min_depth=" + std::to_string(p->min_depth) + "\n##read_profile_max_alt_permille=" + std::to_string(p->max_alt_permille)
                       + "\n##empirical_quality=-10*log10((mismatch+1)/(match+mismatch+2))\n#counter\tcount\n";
    for (int k = UVC_READPROF_bases_low_mapq; k < UVC_READPROF_reserved; k++) text += std::string(COUNTERS[k]) + "\t" + std::to_string(p->sum[UVC_READPROF_COUNTERS + k - UVC_READPROF_bases_low_mapq]) + "\n";
    auto lines = [&](const char *head, int first, int bins, int width) {   // one line per (class, bin) with a non-zero word
        text += head;
        for (int c = 0; c < UVC_READPROF_NCLASS; c++)
            for (int b = 0; b < bins; b++) {
                const int64_t *v = p->sum + first + (c * bins + b) * width;
                bool any = false;
                for (int j = 0; j < width; j++) any = any || v[j] != 0;
                if (!any) continue;
                text += p->classes[c] + "\t" + std::to_string(b);
                for (int j = 0; j < width; j++) text += "\t" + std::to_string(v[j]);
                text += "\n";
            }
    };
    lines("#class\tquality\tmatch\tmismatch\n", UVC_READPROF_Q_BINS, UVC_READPROF_NQUAL, 2);
    lines("#class\tcycle\tmatch\tmismatch\tins\tdel\tclip\n", UVC_READPROF_CYC_BINS, UVC_READPROF_NCYCLE, UVC_READPROF_NKIND);
    text += "#class\tref\tread\tcount\n";
    for (int c = 0; c < UVC_READPROF_NCLASS; c++)
        for (int k = 0; k < 16; k++) {
            const int64_t v = p->sum[UVC_READPROF_SUB_BINS + c * 16 + k];
            if (v) text += p->classes[c] + "\t" + BASE_SYM[k >> 2] + "\t" + BASE_SYM[k & 3] + "\t" + std::to_string(v) + "\n";
        }
    return write_text(path, text);
}
extern "C" void uvcio_readprofile_close(uvcio_readprofile_t *p) { delete p; }

// ---------------------------------------------------------------- the UMI family report ----
// the row layout is that of uvcgpu_region_family_stats (UVC_FAMSTAT_* of uvcgpu.h, include/uvc_famstats.def); the reserved word is not written
struct uvcio_famstats {
    struct Target : ReportTarget { int64_t c[4]; };
    std::vector<Target> targets;
    int64_t first[UVC_FAMSTAT_ROW];   // the FIRST blocks of all pieces, summed (words below UVC_FAMSTAT_FIRST stay 0)
    std::mutex mu;
};
extern "C" int uvcio_famstats_open(uvcio_famstats_t **out) {
    if (!out) return fail(UVCGPU_EINVAL, "family report: bad argument");
    uvcio_famstats *f = new uvcio_famstats;
    memset(f->first, 0, sizeof(f->first));
    *out = f;
    return 0;
}
extern "C" int64_t uvcio_famstats_add_target(uvcio_famstats_t *f, const char *chrom, int64_t beg, int64_t end, const char *name) {
    if (!f || !chrom) return fail(UVCGPU_EINVAL, "family report: bad target");
    std::lock_guard<std::mutex> g(f->mu);
    f->targets.push_back(uvcio_famstats::Target{ report_target(chrom, name, beg, end), { 0, 0, 0, 0 } });
    return (int64_t)f->targets.size() - 1;
}
extern "C" int uvcio_famstats_add_piece(uvcio_famstats_t *f, int64_t target, const int64_t *row) {
    if (!f || !row) return fail(UVCGPU_EINVAL, "family report: bad piece");
    std::lock_guard<std::mutex> g(f->mu);
    if (target < 0 || target >= (int64_t)f->targets.size()) return fail(UVCGPU_EINVAL, "family report: piece of target " + std::to_string(target) + ", which does not exist");
    for (int k = 0; k < 4; k++) f->targets[(size_t)target].c[k] += row[UVC_FAMSTAT_TARGET + k];
    for (int k = UVC_FAMSTAT_FIRST; k < UVC_FAMSTAT_ROW; k++) f->first[k] += row[k];
    return 0;
}
static int64_t fs_ratio(int64_t num, int64_t den) { return den ? 1000 * num / den : 0; }
extern "C" int uvcio_famstats_write(const uvcio_famstats_t *f, const char *path) {
    if (!f || !path || !*path) return fail(UVCGPU_EINVAL, "family report: bad argument");
    static const char *const NAMES[7] = { "families", "fragments", "alignments", "families_both_strands", "families_umi", "families_duplex_tag", "families_amplicon" };
    const int64_t *c = f->first + UVC_FAMSTAT_FIRST;
    std::string text = "##family_stats=1\n##summary and histograms: every family that overlaps a target, counted once; target lines: every family that overlaps the target\n#summary\n";
    for (int k = 0; k < 7; k++) text += std::string(NAMES[k]) + "\t" + std::to_string(c[k]) + "\n";
    text += "duplication_permille\t" + std::to_string(fs_ratio(c[1] - c[0], c[1])) + "\nmean_family_size_x1000\t" + std::to_string(fs_ratio(c[1], c[0])) + "\nboth_strands_permille\t" + std::to_string(fs_ratio(c[3], c[0])) + "\n";
    text += "#family_size\tfamilies\n";
    for (int k = 0; k < UVC_FAMSTAT_NSIZE; k++) text += std::to_string(k + 1) + (k + 1 == UVC_FAMSTAT_NSIZE ? "+" : "") + "\t" + std::to_string(f->first[UVC_FAMSTAT_SIZE + k]) + "\n";
    text += "#strand0_size\tstrand1_size\tfamilies\n";
    auto label = [](int v) { return std::to_string(v) + (v == UVC_FAMSTAT_STRAND_CAP ? "+" : ""); };
    for (int a = 0; a <= UVC_FAMSTAT_STRAND_CAP; a++)
        for (int b = 0; b <= UVC_FAMSTAT_STRAND_CAP; b++) {
            const int64_t v = f->first[UVC_FAMSTAT_STRANDS + a * (UVC_FAMSTAT_STRAND_CAP + 1) + b];
            if (v) text += label(a) + "\t" + label(b) + "\t" + std::to_string(v) + "\n";
        }
    text += "#chrom\tbeg\tend\tname\tfamilies\tfragments\talignments\tfamilies_both_strands\tmean_family_size_x1000\tboth_strands_permille\n";
    for (const uvcio_famstats::Target &t : f->targets)
        text += t.chrom + "\t" + std::to_string(t.beg) + "\t" + std::to_string(t.end) + "\t" + t.name + "\t" + std::to_string(t.c[0]) + "\t" + std::to_string(t.c[1]) + "\t" + std::to_string(t.c[2]) + "\t"
                + std::to_string(t.c[3]) + "\t" + std::to_string(fs_ratio(t.c[1], t.c[0])) + "\t" + std::to_string(fs_ratio(t.c[3], t.c[0])) + "\n";
    return write_text(path, text);
}
extern "C" void uvcio_famstats_close(uvcio_famstats_t *f) { delete f; }

// ---------------------------------------------------------------- the fragment length and end-motif profile ----
// the layouts are those of uvcgpu_region_fragment_profile (UVC_FRAGPROF_* of uvcgpu.h); the sections and their names: include/uvc_fragprofile.def
struct FragProfSection { const char *name; int first, words; };
static const FragProfSection FRAGPROF_SECTIONS[UVC_NFRAGPROF] = {
#define UVC_FRAGPROF(name, first, words) { #name, first, words },
#include "uvc_fragprofile.def"
#undef UVC_FRAGPROF
};
struct uvcio_fragprofile {
    UvcFragmentProfileRequest req;
    struct Target : ReportTarget { int64_t c[UVC_FRAGPROF_TARGET_ROW]; };
    std::vector<Target> targets;
    int64_t prof[UVC_FRAGPROF_ROW];   // the profile rows of all calls, summed
    std::mutex mu;
};
extern "C" int uvcio_fragprofile_open(uvcio_fragprofile_t **out, int32_t min_mapq, int32_t short_lo, int32_t short_hi, int32_t long_lo, int32_t long_hi) {
    if (!out) return fail(UVCGPU_EINVAL, "fragment profile: bad argument");
    uvcio_fragprofile *f = new uvcio_fragprofile;
    f->req = UvcFragmentProfileRequest{ min_mapq, short_lo, short_hi, long_lo, long_hi };
    memset(f->prof, 0, sizeof(f->prof));
    *out = f;
    return 0;
}
extern "C" int64_t uvcio_fragprofile_add_target(uvcio_fragprofile_t *f, const char *chrom, int64_t beg, int64_t end, const char *name) {
    if (!f || !chrom) return fail(UVCGPU_EINVAL, "fragment profile: bad target");
    std::lock_guard<std::mutex> g(f->mu);
    f->targets.push_back(uvcio_fragprofile::Target{ report_target(chrom, name, beg, end), {} });
    return (int64_t)f->targets.size() - 1;
}
extern "C" int uvcio_fragprofile_add_piece(uvcio_fragprofile_t *f, int64_t target, const int64_t *row) {
    if (!f || !row) return fail(UVCGPU_EINVAL, "fragment profile: bad piece");
    std::lock_guard<std::mutex> g(f->mu);
    if (target < 0 || target >= (int64_t)f->targets.size()) return fail(UVCGPU_EINVAL, "fragment profile: piece of target " + std::to_string(target) + ", which does not exist");
    for (int k = 0; k < UVC_FRAGPROF_TARGET_ROW; k++) f->targets[(size_t)target].c[k] += row[k];
    return 0;
}
extern "C" int uvcio_fragprofile_add_profile(uvcio_fragprofile_t *f, const int64_t *profile) {
    if (!f || !profile) return fail(UVCGPU_EINVAL, "fragment profile: bad profile");
    std::lock_guard<std::mutex> g(f->mu);
    for (int k = 0; k < UVC_FRAGPROF_ROW; k++) f->prof[k] += profile[k];
    return 0;
}
extern "C" int uvcio_fragprofile_write(const uvcio_fragprofile_t *f, const char *path) {
    if (!f || !path || !*path) return fail(UVCGPU_EINVAL, "fragment profile: bad argument");
    auto range = [](int32_t a, int32_t b) { return std::to_string(a) + "-" + std::to_string(b); };
    std::string text = "##fragment_profile=1\n##fragment_profile_min_mapq=" + std::to_string(f->req.min_mapq) + "\n##fragment_profile_short=" + range(f->req.short_lo, f->req.short_hi)
                       + "\n##fragment_profile_long=" + range(f->req.long_lo, f->req.long_hi)
                       + "\n##summary, lengths and end motifs: every fragment and family that overlaps a target, counted once; target lines: every fragment and family that overlaps the target\n#summary\n";
    auto is_counter = [](const FragProfSection &s) { return s.words == 1 && s.first < UVC_FRAGPROF_NCOUNTER && strncmp(s.name, "reserved", 8) != 0; };
    for (const FragProfSection &s : FRAGPROF_SECTIONS) if (is_counter(s)) text += std::string(s.name) + "\t" + std::to_string(f->prof[s.first]) + "\n";
    text += "#length\tfragments\tfamilies\n";
    for (int k = 0; k < UVC_FRAGPROF_NLEN; k++)
        text += std::to_string(k) + (k + 1 == UVC_FRAGPROF_NLEN ? "+" : "") + "\t" + std::to_string(f->prof[UVC_FRAGPROF_LEN_BINS + k]) + "\t" + std::to_string(f->prof[UVC_FRAGPROF_FAMLEN_BINS + k]) + "\n";
    text += "#end_motif\tcount\n";
    for (int m = 0; m < UVC_FRAGPROF_NMOTIF; m++) {
        char motif[5] = { "ACGT"[(m >> 6) & 3], "ACGT"[(m >> 4) & 3], "ACGT"[(m >> 2) & 3], "ACGT"[m & 3], 0 };
        text += std::string(motif) + "\t" + std::to_string(f->prof[UVC_FRAGPROF_MOTIF_BINS + m]) + "\n";
    }
    text += "#chrom\tbeg\tend\tname";
    for (const FragProfSection &s : FRAGPROF_SECTIONS) if (is_counter(s) && s.first < UVC_FRAGPROF_TARGET_ROW) text += std::string("\t") + s.name;
    text += "\n";
    for (const uvcio_fragprofile::Target &t : f->targets) {
        text += t.chrom + "\t" + std::to_string(t.beg) + "\t" + std::to_string(t.end) + "\t" + t.name;
        for (const FragProfSection &s : FRAGPROF_SECTIONS) if (is_counter(s) && s.first < UVC_FRAGPROF_TARGET_ROW) text += "\t" + std::to_string(t.c[s.first]);
        text += "\n";
    }
    return write_text(path, text);
}
extern "C" void uvcio_fragprofile_close(uvcio_fragprofile_t *f) { delete f; }

// ---------------------------------------------------------------- the reads and families behind listed sites ----
// the rows and counts are those of uvcgpu_region_site_reads (UvcSiteRead, UVC_SITEREAD_* of uvcgpu.h).  The family and fragment ids of a row are
// local to its call: the store keeps them with the call's serial number, compares them for equality alone and writes none of them.
struct uvcio_sitereads {
    UvcSiteReadsRequest req;
    std::string kinds[UVC_SITEREAD_NKIND], classes[4];
    struct Row { int32_t kind, qual, cycle, cls, mapq, flag, strand, frag, del_len; int64_t fam; std::string qname, ins; };   // fam: call << 32 | the 32 bits of fam_id
    struct Site { std::string contig; char ref = '.'; int64_t c[UVC_SITEREAD_NCOL] = {}; std::vector<Row> rows; };
    std::map<std::pair<int32_t, int32_t>, Site> sites;   // by (tid, zero-based position)
    int64_t n_calls = 0;
    std::mutex mu;
};
extern "C" int uvcio_sitereads_open(uvcio_sitereads_t **out, const char *const *kind_names, const char *const *class_names, int32_t min_mapq, int32_t alt_only) {
    if (!out || !kind_names || !class_names) return fail(UVCGPU_EINVAL, "site reads: bad argument");
    uvcio_sitereads *f = new uvcio_sitereads;
    f->req = UvcSiteReadsRequest{ min_mapq, alt_only };
    for (int k = 0; k < UVC_SITEREAD_NKIND; k++) f->kinds[k] = kind_names[k] ? kind_names[k] : "";
    for (int c = 0; c < 4; c++) f->classes[c] = class_names[c] ? class_names[c] : "";
    *out = f;
    return 0;
}
extern "C" int uvcio_sitereads_add(uvcio_sitereads_t *f, int32_t tid, const char *contig, const int32_t *sites, const char *ref, int64_t n_sites, const int32_t *counts, const UvcSiteRead *rows, int64_t n_rows,
                                   int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *l_qseq, const int32_t *fam_id, const uint8_t *fam_strand,
                                   const int32_t *frag_id, const uint8_t *bases, const int64_t *seq_off) {
    if (!f || !contig || n_sites < 0 || (n_sites > 0 && !sites) || n_rows < 0) return fail(UVCGPU_EINVAL, "site reads: bad argument");
    if (n_rows > 0 && (!rows || !counts || !qnames || !flag || !mapq || !l_qseq || !fam_id || !fam_strand || !frag_id || !bases || !seq_off)) return fail(UVCGPU_EINVAL, "site reads: rows without the columns of their alignments");
    // what the rows keep is made outside the lock
    std::vector<std::pair<int32_t, uvcio_sitereads::Row>> made((size_t)n_rows);
    for (int64_t k = 0; k < n_rows; k++) {
        const UvcSiteRead &r = rows[k];
        if (r.site < 0 || r.site >= n_sites || r.read < 0 || r.read >= n_alns || !qnames[r.read]) return fail(UVCGPU_EINVAL, "site reads: row " + std::to_string(k) + " names site " + std::to_string(r.site) + " and alignment " + std::to_string(r.read) + ", which the call does not hold");
        const int a = r.read, L = l_qseq[a], fl = flag[a];
        uvcio_sitereads::Row w;
        w.kind = r.obs & 0xFF; w.qual = r.obs >> 8; w.cycle = (fl & 0x10) ? L - 1 - r.q : r.q; w.cls = 2 * ((fl & 0x80) != 0) + ((fl & 0x10) != 0);
        w.mapq = mapq[a]; w.flag = fl; w.fam = (int64_t)(uint32_t)fam_id[a]; w.strand = fam_strand[a]; w.frag = frag_id[a]; w.del_len = r.del_len; w.qname = qnames[a];
        if (w.kind < 0 || w.kind >= UVC_SITEREAD_NKIND) return fail(UVCGPU_EINVAL, "site reads: row " + std::to_string(k) + " has kind " + std::to_string(w.kind));
        for (int32_t j = 0; j < r.ins_len && r.ins_q >= 0 && r.ins_q + j < L; j++) { const uint8_t b = bases[seq_off[a] + r.ins_q + j]; w.ins += (b < 4 ? "ACGT"[b] : 'N'); }
        made[(size_t)k] = std::make_pair(r.site, std::move(w));
    }
    std::lock_guard<std::mutex> g(f->mu);
    for (int64_t s = 0; s < n_sites; s++) {
        uvcio_sitereads::Site &site = f->sites[std::make_pair(tid, sites[s])];
        if (site.contig.empty()) site.contig = contig;
        if (ref && ref[s]) site.ref = (char)toupper((unsigned char)ref[s]);
        if (counts) for (int c = 0; c < UVC_SITEREAD_NCOL; c++) site.c[c] += counts[s * UVC_SITEREAD_NCOL + c];
    }
    const int64_t call = f->n_calls++;
    for (auto &m : made) { m.second.fam |= call << 32; f->sites[std::make_pair(tid, sites[m.first])].rows.push_back(std::move(m.second)); }
    return 0;
}
extern "C" int uvcio_sitereads_write(const uvcio_sitereads_t *f, const char *path) {
    if (!f || !path || !*path) return fail(UVCGPU_EINVAL, "site reads: bad argument");
    typedef uvcio_sitereads::Row Row;
    std::string text = "##site_reads_min_mapq=" + std::to_string(f->req.min_mapq) + "\n##site_reads_alt_only=" + std::to_string(f->req.alt_only)
                       + "\n#S\tcontig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tDEL\tINS\tDEL_after\n#A\tcontig\tpos\tallele\treads\tfragments\tfamilies\tfamilies_both_strands\n"
                         "#R\tcontig\tpos\tobs\tqual\tcycle\tclass\tmapq\tqname\tflag\tfamily\tstrand\tins\tdel\n";
    for (const auto &kv : f->sites) {   // (the map is ordered by (tid, pos))
        const uvcio_sitereads::Site &site = kv.second;
        const std::string at = "\t" + site.contig + "\t" + std::to_string((int64_t)kv.first.second + 1);
        int64_t depth = 0;
        for (int c = 0; c < UVC_SITEREAD_NKIND; c++) depth += site.c[c];
        text += "S" + at + "\t" + site.ref + "\t" + std::to_string(depth);
        for (int c = 0; c < UVC_SITEREAD_NCOL; c++) text += "\t" + std::to_string(site.c[c]);
        text += "\n";
        if (site.rows.empty()) continue;
        // a family's rank: by the smallest (qname, flag) of its rows at this site (families of two calls that share it share the rank)
        std::map<int64_t, std::pair<std::string, int32_t>> least;
        for (const Row &r : site.rows) {
            const auto key = std::make_pair(r.qname, r.flag);
            auto it = least.find(r.fam);
            if (it == least.end()) least[r.fam] = key; else if (key < it->second) it->second = key;
        }
        std::vector<std::pair<std::string, int32_t>> keys;
        for (const auto &l : least) keys.push_back(l.second);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        std::map<int64_t, int64_t> rank;
        for (const auto &l : least) rank[l.first] = (std::lower_bound(keys.begin(), keys.end(), l.second) - keys.begin()) + 1;
        // the alleles: the kinds in their order, the insertions by their bases, the deletions by their length; a row with an event counts
        // under its event alleles and not under its base
        std::map<std::pair<int, std::string>, std::vector<const Row *>> alleles;
        auto del_key = [](int32_t n) { std::string s = std::to_string(n); return std::string(12 - std::min<size_t>(12, s.size()), '0') + s; };   // (numeric order)
        for (const Row &r : site.rows) {
            if (!r.ins.empty()) alleles[std::make_pair(UVC_SITEREAD_NKIND, r.ins)].push_back(&r);
            if (r.del_len > 0) alleles[std::make_pair(UVC_SITEREAD_NKIND + 1, del_key(r.del_len))].push_back(&r);
            if (r.ins.empty() && r.del_len <= 0) alleles[std::make_pair(r.kind, std::string())].push_back(&r);
        }
        for (const auto &al : alleles) {
            const int cls = al.first.first;
            const std::string name = cls < UVC_SITEREAD_NKIND ? f->kinds[cls] : cls == UVC_SITEREAD_NKIND ? "+" + al.first.second : "-" + std::to_string(al.second[0]->del_len);
            std::set<std::tuple<int64_t, int32_t, int32_t>> frags;
            std::map<int64_t, int> strands;   // family -> bit 0 / 1: a row of fam_strand 0 / 1
            for (const Row *r : al.second) { frags.insert(std::make_tuple(r->fam, r->strand, r->frag)); strands[r->fam] |= 1 << (r->strand & 1); }
            int64_t both = 0;
            for (const auto &s : strands) both += (s.second == 3);
            text += "A" + at + "\t" + name + "\t" + std::to_string(al.second.size()) + "\t" + std::to_string(frags.size()) + "\t" + std::to_string(strands.size()) + "\t" + std::to_string(both) + "\n";
        }
        std::vector<const Row *> order;
        for (const Row &r : site.rows) order.push_back(&r);
        std::sort(order.begin(), order.end(), [&](const Row *a, const Row *b) {
            const int64_t ra = rank[a->fam], rb = rank[b->fam];
            return std::tie(ra, a->qname, a->flag, a->cycle) < std::tie(rb, b->qname, b->flag, b->cycle);
        });
        for (const Row *r : order)
            text += "R" + at + "\t" + f->kinds[r->kind] + "\t" + std::to_string(r->qual) + "\t" + std::to_string(r->cycle) + "\t" + f->classes[r->cls] + "\t" + std::to_string(r->mapq) + "\t" + r->qname + "\t"
                    + std::to_string(r->flag) + "\t" + std::to_string(rank[r->fam]) + "\t" + std::to_string(r->strand) + "\t" + (r->ins.empty() ? std::string(".") : r->ins) + "\t" + std::to_string(r->del_len) + "\n";
    }
    return write_text(path, text);
}
extern "C" void uvcio_sitereads_close(uvcio_sitereads_t *f) { delete f; }

// ---------------------------------------------------------------- clipped-read breakpoint sites ----
// the rows are those of uvcgpu_region_clip_sites (UVC_CLIPSITE_* of uvcgpu.h, include/uvc_clipsites.def; UvcClipRead).  The family and fragment
// ids of an event are local to its call, and a site comes from one call: the store compares them inside a site alone and writes none.
namespace {
enum {
#define UVC_CLIPSITE(name, first, words) CSW_##name = first,
#include "uvc_clipsites.def"
#undef UVC_CLIPSITE
#define UVC_CLIPJUNC(name, first, words) CJW_##name = first,
#include "uvc_clipjunc.def"
#undef UVC_CLIPJUNC
#define UVC_CLIPMATE_SITE(name, first, words) CMSW_##name = first,
#define UVC_CLIPMATE_CLUSTER(name, first, words) CMCW_##name = first,
#include "uvc_clipmates.def"
#undef UVC_CLIPMATE_SITE
#undef UVC_CLIPMATE_CLUSTER
};
static_assert(CMSW_facing == 1 && CMSW_clusters_kept == UVC_CLIPMATE_SITE_ROW - 1 && CMCW_mapq_sum == CMCW_pairs + 4 && (int)CMCW_first < (int)UVC_CLIPMATE_ROW,
              "the words of a P line are facing .. clusters_kept, those of an M line pairs .. mapq_sum of include/uvc_clipmates.def");
static_assert(CJW_hist + UVC_CLIPJUNC_NHIST <= UVC_CLIPJUNC_ROW && CJW_mate < CJW_hist, "the words of a J line are query_len .. mate of include/uvc_clipjunc.def");
static_assert(CSW_VOTE == UVC_CLIPSITE_VOTE_BINS && CSW_VOTE + UVC_CLIPSITE_NCONS * UVC_CLIPSITE_NCODE == UVC_CLIPSITE_ROW && CSW_spanning == CSW_reads + 8,
              "the words of an S line are reads .. spanning of include/uvc_clipsites.def, the votes fill the row behind the counters");
}
struct uvcio_clipsites {
    UvcClipSitesRequest req;
    struct Event { std::string qname; int32_t flag, mapq, soft, hard, fam, strand, frag; };
    // junc: the site's row of uvcgpu_region_clip_junctions, when its call came with them; its mate, an index into the call's rows, as (pos, side)
    // a kept cluster of uvcgpu_region_clip_mates with what the host counts over its witnesses: fragments, families, families on both strands
    struct Mate { int64_t row[UVC_CLIPMATE_ROW], frags, fams, both; };
    struct Site { std::string contig; int64_t row[UVC_CLIPSITE_ROW]; std::vector<Event> events; bool has_junc = false; int64_t junc[UVC_CLIPJUNC_ROW], mate_pos = -1, mate_side = -1;
                  bool has_mates = false; int64_t mrow[UVC_CLIPMATE_SITE_ROW]; std::vector<Mate> mates; };
    bool junctions = false; UvcClipJunctionsRequest jreq{ 0, 0, 0, 0, 0 };   // uvcio_clipsites_set_junctions
    bool mates = false; UvcClipMatesRequest mreq{ 0, 0, 0, 0, 0, 0, 0, 0 }; std::vector<std::string> contigs;   // uvcio_clipsites_set_mates
    std::map<std::tuple<int32_t, int64_t, int64_t>, Site> sites;   // by (tid, zero-based position, side)
    std::mutex mu;
};
extern "C" int uvcio_clipsites_open(uvcio_clipsites_t **out, int32_t min_mapq, int32_t min_clip, int32_t min_reads, int32_t with_reads) {
    if (!out) return fail(UVCGPU_EINVAL, "clip sites: bad argument");
    uvcio_clipsites *f = new uvcio_clipsites;
    f->req = UvcClipSitesRequest{ min_mapq, min_clip, min_reads, with_reads };
    *out = f;
    return 0;
}
extern "C" int uvcio_clipsites_set_junctions(uvcio_clipsites_t *f, int32_t min_votes, int32_t min_len, int32_t max_mismatch, int32_t max_dist, int32_t mate_slop) {
    if (!f) return fail(UVCGPU_EINVAL, "clip sites: bad argument");
    f->junctions = true;
    f->jreq = UvcClipJunctionsRequest{ min_votes, min_len, max_mismatch, max_dist, mate_slop };
    return 0;
}
extern "C" int uvcio_clipsites_set_mates(uvcio_clipsites_t *f, int32_t window, int32_t overhang, int32_t min_dist, int32_t max_gap, int32_t min_pairs, const char *const *contig_names, int32_t n_contigs) {
    if (!f || n_contigs < 0 || (n_contigs > 0 && !contig_names)) return fail(UVCGPU_EINVAL, "clip sites: bad argument");
    f->mates = true;
    f->mreq = UvcClipMatesRequest{ 0, f->req.min_mapq, window, overhang, min_dist, max_gap, min_pairs, 1 };
    f->contigs.clear();
    for (int32_t k = 0; k < n_contigs; k++) f->contigs.push_back(contig_names[k] ? contig_names[k] : ".");
    return 0;
}
extern "C" int uvcio_clipsites_add_mates(uvcio_clipsites_t *f, int32_t tid, const char *contig, const int64_t *sites, const int64_t *junctions, int64_t n_sites, const UvcClipRead *reads, int64_t n_reads,
                                         int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *fam_id, const uint8_t *fam_strand, const int32_t *frag_id,
                                         const int64_t *site_rows, const int64_t *clusters, int64_t n_clusters, const UvcClipMate *mates, int64_t n_mates) {
    if (!f || !contig || n_sites < 0 || (n_sites > 0 && !sites) || n_reads < 0) return fail(UVCGPU_EINVAL, "clip sites: bad argument");
    if (n_reads > 0 && (!reads || !qnames || !flag || !mapq || !fam_id || !fam_strand || !frag_id)) return fail(UVCGPU_EINVAL, "clip sites: event rows without the columns of their alignments");
    // what the sites keep is made outside the lock
    std::vector<uvcio_clipsites::Site> made((size_t)n_sites);
    for (int64_t s = 0; s < n_sites; s++) {
        made[(size_t)s].contig = contig;
        memcpy(made[(size_t)s].row, sites + s * UVC_CLIPSITE_ROW, sizeof(int64_t) * UVC_CLIPSITE_ROW);
        const int64_t side = made[(size_t)s].row[CSW_side];
        if (side != UVC_CLIPSITE_LEFT && side != UVC_CLIPSITE_RIGHT) return fail(UVCGPU_EINVAL, "clip sites: site " + std::to_string(s) + " has side " + std::to_string(side));
        if (!junctions) continue;
        uvcio_clipsites::Site &m = made[(size_t)s];
        m.has_junc = true;
        memcpy(m.junc, junctions + s * UVC_CLIPJUNC_ROW, sizeof(int64_t) * UVC_CLIPJUNC_ROW);
        const int64_t mate = m.junc[CJW_mate], klass = m.junc[CJW_klass];
        if (mate >= n_sites || klass < 0 || klass >= UVC_NCLIPCLASS) return fail(UVCGPU_EINVAL, "clip sites: junction row " + std::to_string(s) + " has mate " + std::to_string(mate) + " and class " + std::to_string(klass) + ", which the call does not hold");
        if (mate >= 0) { m.mate_pos = sites[mate * UVC_CLIPSITE_ROW + CSW_pos]; m.mate_side = sites[mate * UVC_CLIPSITE_ROW + CSW_side]; }
    }
    if (site_rows) {   // the call's rows of uvcgpu_region_clip_mates: a P line per site, an M line per kept cluster
        if (n_clusters < 0 || n_mates < 0 || (n_clusters > 0 && !clusters)) return fail(UVCGPU_EINVAL, "clip sites: bad argument");
        if (n_mates > 0 && (!mates || !fam_id || !fam_strand || !frag_id)) return fail(UVCGPU_EINVAL, "clip sites: witness rows without the columns of their alignments");
        for (int64_t s = 0; s < n_sites; s++) { made[(size_t)s].has_mates = true; memcpy(made[(size_t)s].mrow, site_rows + s * UVC_CLIPMATE_SITE_ROW, sizeof(int64_t) * UVC_CLIPMATE_SITE_ROW); }
        std::vector<std::set<std::tuple<int32_t, int32_t, int32_t>>> frags((size_t)n_clusters);
        std::vector<std::map<int32_t, int>> strands((size_t)n_clusters);   // family -> bit 0 / 1: a witness of fam_strand 0 / 1
        for (int64_t k = 0; k < n_mates; k++) {
            const UvcClipMate &w = mates[k];
            if (w.cluster >= n_clusters || w.read < 0 || w.read >= n_alns) return fail(UVCGPU_EINVAL, "clip sites: witness row " + std::to_string(k) + " names cluster " + std::to_string(w.cluster) + " and alignment " + std::to_string(w.read) + ", which the call does not hold");
            if (w.cluster < 0) continue;
            const int a = w.read;
            frags[(size_t)w.cluster].insert(std::make_tuple(fam_id[a], (int32_t)fam_strand[a], frag_id[a]));
            strands[(size_t)w.cluster][fam_id[a]] |= 1 << (fam_strand[a] & 1);
        }
        for (int64_t c = 0; c < n_clusters; c++) {   // (in witness order: the M lines of a site keep it)
            uvcio_clipsites::Mate m;
            memcpy(m.row, clusters + c * UVC_CLIPMATE_ROW, sizeof m.row);
            const int64_t s = m.row[CMCW_site], strand = m.row[CMCW_mate_strand];
            if (s < 0 || s >= n_sites || strand < 0 || strand > 1) return fail(UVCGPU_EINVAL, "clip sites: cluster row " + std::to_string(c) + " has site " + std::to_string(s) + " and mate strand " + std::to_string(strand) + ", which the call does not hold");
            m.frags = (int64_t)frags[(size_t)c].size(); m.fams = (int64_t)strands[(size_t)c].size(); m.both = 0;
            for (const auto &kv : strands[(size_t)c]) m.both += (kv.second == 3);
            made[(size_t)s].mates.push_back(m);
        }
    }
    for (int64_t k = 0; k < n_reads; k++) {
        const UvcClipRead &r = reads[k];
        if (r.site < 0 || r.site >= n_sites || r.read < 0 || r.read >= n_alns || !qnames[r.read]) return fail(UVCGPU_EINVAL, "clip sites: event row " + std::to_string(k) + " names site " + std::to_string(r.site) + " and alignment " + std::to_string(r.read) + ", which the call does not hold");
        const int a = r.read;
        made[(size_t)r.site].events.push_back(uvcio_clipsites::Event{ qnames[a], flag[a], mapq[a], r.soft_len, r.hard_len, fam_id[a], fam_strand[a], frag_id[a] });
    }
    std::lock_guard<std::mutex> g(f->mu);
    for (auto &m : made) {
        const auto key = std::make_tuple(tid, m.row[CSW_pos], m.row[CSW_side]);
        auto it = f->sites.find(key);
        // a position inside two overlapping targets has two owners, which see the same alignments: the site is kept once -- the report with
        // the larger row where the two differ, the first where they are equal -- so that the text does not depend on who came first
        if (it == f->sites.end()) f->sites[key] = std::move(m);
        else if (std::lexicographical_compare(it->second.row + CSW_reads, it->second.row + UVC_CLIPSITE_ROW, m.row + CSW_reads, m.row + UVC_CLIPSITE_ROW)) it->second = std::move(m);
    }
    return 0;
}
extern "C" int uvcio_clipsites_add_junctions(uvcio_clipsites_t *f, int32_t tid, const char *contig, const int64_t *sites, const int64_t *junctions, int64_t n_sites, const UvcClipRead *reads, int64_t n_reads,
                                             int64_t n_alns, const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *fam_id, const uint8_t *fam_strand, const int32_t *frag_id) {
    return uvcio_clipsites_add_mates(f, tid, contig, sites, junctions, n_sites, reads, n_reads, n_alns, qnames, flag, mapq, fam_id, fam_strand, frag_id, nullptr, nullptr, 0, nullptr, 0);
}
extern "C" int uvcio_clipsites_add(uvcio_clipsites_t *f, int32_t tid, const char *contig, const int64_t *sites, int64_t n_sites, const UvcClipRead *reads, int64_t n_reads, int64_t n_alns,
                                   const char *const *qnames, const uint16_t *flag, const uint8_t *mapq, const int32_t *fam_id, const uint8_t *fam_strand, const int32_t *frag_id) {
    return uvcio_clipsites_add_junctions(f, tid, contig, sites, nullptr, n_sites, reads, n_reads, n_alns, qnames, flag, mapq, fam_id, fam_strand, frag_id);
}
extern "C" int uvcio_clipsites_write(const uvcio_clipsites_t *f, const char *path) {
    if (!f || !path || !*path) return fail(UVCGPU_EINVAL, "clip sites: bad argument");
    typedef uvcio_clipsites::Event Event;
    std::string text = "##clip_sites_min_mapq=" + std::to_string(f->req.min_mapq) + "\n##clip_sites_min_clip=" + std::to_string(f->req.min_clip) + "\n##clip_sites_min_reads=" + std::to_string(f->req.min_reads)
                       + "\n##clip_sites_reads=" + std::to_string(f->req.want_reads)
                       + (f->junctions ? "\n##clip_sites_junction_min_votes=" + std::to_string(f->jreq.min_votes) + "\n##clip_sites_junction_min_len=" + std::to_string(f->jreq.min_len) + "\n##clip_sites_junction_max_mismatch="
                                             + std::to_string(f->jreq.max_mismatch) + "\n##clip_sites_junction_max_dist=" + std::to_string(f->jreq.max_dist) + "\n##clip_sites_junction_slop=" + std::to_string(f->jreq.mate_slop)
                                       : std::string())
                       + (f->mates ? "\n##clip_sites_mate_window=" + std::to_string(f->mreq.window) + "\n##clip_sites_mate_overhang=" + std::to_string(f->mreq.overhang) + "\n##clip_sites_mate_min_dist="
                                         + std::to_string(f->mreq.min_dist) + "\n##clip_sites_mate_max_gap=" + std::to_string(f->mreq.max_gap) + "\n##clip_sites_mate_min_pairs=" + std::to_string(f->mreq.min_pairs)
                                   : std::string())
                       + "\n#S\tcontig\tpos\tside\treads\tfwd\tsupp\tsecondary\thard\tlen_sum\tlen_max\tmapq_sum\tspanning\tfragments\tfamilies\tfamilies_both_strands\tcons_len\tcons\n"
                         "#R\tcontig\tpos\tside\tqname\tflag\tmapq\tsoft_len\thard_len\tfamily_rank\tstrand\n";
    if (f->junctions) text += "#J\tcontig\tpos\tside\tquery_len\tcmp_len\tstatus\tbest_mm\tn_best\tsecond_mm\tpartner_pos\tstrand\tclass\tlen\tmate_pos\tmate_side\n";
    if (f->mates) text += "#P\tcontig\tpos\tside\tfacing\tconcordant\tother_contig\tsame_strand\tfar\tclusters\tclusters_kept\n"
                          "#M\tcontig\tpos\tside\tmate_contig\tmate_beg\tmate_end\tmate_strand\tpairs\tother_contig\tsame_strand\tfar\tmapq_sum\tfragments\tfamilies\tfamilies_both_strands\n";
    static const char *const classes[UVC_NCLIPCLASS] = { "NONE", "DEL", "DUP", "INV", "ADJACENT" };
    auto dot = [](int64_t v, int64_t add) { return v < 0 ? std::string(".") : std::to_string(v + add); };
    for (const auto &kv : f->sites) {   // (the map is ordered by (tid, pos, side))
        const uvcio_clipsites::Site &site = kv.second;
        const bool left = (site.row[CSW_side] == UVC_CLIPSITE_LEFT);
        const std::string at = "\t" + site.contig + "\t" + std::to_string(site.row[CSW_pos] + 1) + "\t" + (left ? "L" : "R");
        text += "S" + at;
        for (int w = CSW_reads; w <= CSW_spanning; w++) text += "\t" + std::to_string(site.row[w]);
        std::set<std::tuple<int32_t, int32_t, int32_t>> frags;
        std::map<int32_t, int> strands;   // family -> bit 0 / 1: an event of fam_strand 0 / 1
        for (const Event &e : site.events) { frags.insert(std::make_tuple(e.fam, e.strand, e.frag)); strands[e.fam] |= 1 << (e.strand & 1); }
        int64_t both = 0;
        for (const auto &s : strands) both += (s.second == 3);
        // the consensus of the votes: one letter per k with a vote, outward from the junction; a LEFT site reads in reference direction
        std::string cons;
        for (int k = 0; k < UVC_CLIPSITE_NCONS; k++) {
            const int64_t *v = site.row + CSW_VOTE + k * UVC_CLIPSITE_NCODE;
            int64_t total = 0; int win = 0;
            for (int c = 0; c < UVC_CLIPSITE_NCODE; c++) { total += v[c]; if (v[c] > v[win]) win = c; }
            if (total <= 0) continue;
            const char ch = "ACGTN"[win];
            cons += (v[win] * 3 < total * 2) ? (char)tolower((unsigned char)ch) : ch;
        }
        const size_t cons_len = cons.size();
        if (left) std::reverse(cons.begin(), cons.end());
        text += "\t" + std::to_string(frags.size()) + "\t" + std::to_string(strands.size()) + "\t" + std::to_string(both) + "\t" + std::to_string(cons_len) + "\t" + (cons.empty() ? std::string(".") : cons) + "\n";
        if (f->junctions && site.has_junc) {   // the J line directly behind the S line
            const int64_t *j = site.junc;
            text += "J" + at + "\t" + std::to_string(j[CJW_query_len]) + "\t" + std::to_string(j[CJW_cmp_len]) + "\t" + std::to_string(j[CJW_status]) + "\t" + dot(j[CJW_best_mm], 0) + "\t" + std::to_string(j[CJW_n_best])
                    + "\t" + dot(j[CJW_second_mm], 0) + "\t" + dot(j[CJW_partner], 1) + "\t" + (j[CJW_strand] < 0 ? "." : j[CJW_strand] ? "-" : "+") + "\t" + classes[j[CJW_klass]] + "\t" + dot(j[CJW_len], 0)
                    + "\t" + dot(site.mate_pos, 1) + "\t" + (site.mate_side < 0 ? "." : site.mate_side == UVC_CLIPSITE_LEFT ? "L" : "R") + "\n";
        }
        if (f->mates && site.has_mates) {   // the P line and the M lines of the kept clusters behind the S (and J) line
            text += "P" + at;
            for (int w = CMSW_facing; w <= CMSW_clusters_kept; w++) text += "\t" + std::to_string(site.mrow[w]);
            text += "\n";
            for (const uvcio_clipsites::Mate &m : site.mates) {
                const int64_t mt = m.row[CMCW_mtid];
                text += "M" + at + "\t" + (mt >= 0 && mt < (int64_t)f->contigs.size() ? f->contigs[(size_t)mt] : std::string(".")) + "\t" + std::to_string(m.row[CMCW_mpos_min] + 1) + "\t"
                        + std::to_string(m.row[CMCW_mpos_max] + 1) + "\t" + (m.row[CMCW_mate_strand] ? "-" : "+");
                for (int w = CMCW_pairs; w <= CMCW_mapq_sum; w++) text += "\t" + std::to_string(m.row[w]);
                text += "\t" + std::to_string(m.frags) + "\t" + std::to_string(m.fams) + "\t" + std::to_string(m.both) + "\n";
            }
        }
        if (!f->req.want_reads || site.events.empty()) continue;
        // a family's rank: by the smallest (qname, flag) of its events at this site
        std::map<int32_t, std::pair<std::string, int32_t>> least;
        for (const Event &e : site.events) {
            const auto key = std::make_pair(e.qname, e.flag);
            auto it = least.find(e.fam);
            if (it == least.end()) least[e.fam] = key; else if (key < it->second) it->second = key;
        }
        std::vector<std::pair<std::string, int32_t>> keys;
        for (const auto &l : least) keys.push_back(l.second);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        std::map<int32_t, int64_t> rank;
        for (const auto &l : least) rank[l.first] = (std::lower_bound(keys.begin(), keys.end(), l.second) - keys.begin()) + 1;
        std::vector<const Event *> order;
        for (const Event &e : site.events) order.push_back(&e);
        std::stable_sort(order.begin(), order.end(), [&](const Event *a, const Event *b) {
            const int64_t ra = rank[a->fam], rb = rank[b->fam];
            return std::tie(ra, a->qname, a->flag) < std::tie(rb, b->qname, b->flag);
        });
        for (const Event *e : order)
            text += "R" + at + "\t" + e->qname + "\t" + std::to_string(e->flag) + "\t" + std::to_string(e->mapq) + "\t" + std::to_string(e->soft) + "\t" + std::to_string(e->hard) + "\t" + std::to_string(rank[e->fam]) + "\t"
                    + std::to_string(e->strand) + "\n";
    }
    return write_text(path, text);
}
extern "C" void uvcio_clipsites_close(uvcio_clipsites_t *f) { delete f; }

// ---------------------------------------------------------------- the callable-region BED ----
struct uvcio_callable {
    std::vector<std::string> measures, bits; std::vector<int32_t> min_depth; int32_t max_aDP = 0;
    struct Run { int32_t target, beg, end, mask; };   // 16 bytes per run, kept to the end: the file is written in target order
    std::vector<ReportTarget> targets; std::vector<Run> runs;
    std::mutex mu;
};
extern "C" int uvcio_callable_open(uvcio_callable_t **out, const char *const *measure_names, int32_t n_measures, const int32_t *min_depth, int32_t max_aDP, const char *const *bit_names, int32_t n_bits) {
    if (!out || !measure_names || !min_depth || !bit_names || n_measures < 1 || n_measures > 29 || n_bits != n_measures + 2 || max_aDP < 0) return fail(UVCGPU_EINVAL, "callable report: bad argument");
    uvcio_callable *c = new uvcio_callable;
    for (int32_t m = 0; m < n_measures; m++) { c->measures.push_back(measure_names[m] ? measure_names[m] : ""); c->min_depth.push_back(min_depth[m]); }
    for (int32_t b = 0; b < n_bits; b++) c->bits.push_back(bit_names[b] ? bit_names[b] : "");
    c->max_aDP = max_aDP;
    *out = c;
    return 0;
}
extern "C" int64_t uvcio_callable_add_target(uvcio_callable_t *c, const char *chrom, int64_t beg, int64_t end, const char *name) {
    if (!c || !chrom || beg < 0 || end > INT32_MAX) return fail(UVCGPU_EINVAL, "callable report: bad target");
    std::lock_guard<std::mutex> g(c->mu);
    c->targets.push_back(report_target(chrom, name, beg, std::max(beg, end)));
    return (int64_t)c->targets.size() - 1;
}
extern "C" int uvcio_callable_add_runs(uvcio_callable_t *c, const int64_t *target_of_range, int64_t n_ranges, const UvcCallableRun *runs, int64_t n_runs) {
    if (!c || n_runs < 0 || n_ranges < 0 || (n_runs > 0 && (!runs || !target_of_range))) return fail(UVCGPU_EINVAL, "callable report: bad runs");
    std::lock_guard<std::mutex> g(c->mu);
    for (int64_t q = 0; q < n_runs; q++) {   // all of the call's runs or none
        const UvcCallableRun &r = runs[q];
        if (r.range < 0 || r.range >= n_ranges) return fail(UVCGPU_EINVAL, "callable report: run " + std::to_string(q) + " names range " + std::to_string(r.range) + " of " + std::to_string(n_ranges));
        const int64_t t = target_of_range[r.range];
        if (t < 0 || t >= (int64_t)c->targets.size()) return fail(UVCGPU_EINVAL, "callable report: run of target " + std::to_string(t) + ", which does not exist");
        if (r.pos_end <= r.pos_beg || r.pos_beg < c->targets[(size_t)t].beg || r.pos_end > c->targets[(size_t)t].end)
            return fail(UVCGPU_EINVAL, "callable report: run [" + std::to_string(r.pos_beg) + ", " + std::to_string(r.pos_end) + ") is empty or outside target " + std::to_string(t));
    }
    for (int64_t q = 0; q < n_runs; q++) c->runs.push_back(uvcio_callable::Run{ (int32_t)target_of_range[runs[q].range], runs[q].pos_beg, runs[q].pos_end, runs[q].mask });
    return 0;
}
extern "C" int64_t uvcio_callable_n_runs(const uvcio_callable_t *c) { return c ? (int64_t)c->runs.size() : 0; }
extern "C" int uvcio_callable_write(const uvcio_callable_t *c, const char *path) {
    if (!c || !path || !*path) return fail(UVCGPU_EINVAL, "callable report: bad argument");
    const size_t nm = c->measures.size(), nb = c->bits.size();
    std::string text = "##callable_regions=1\n#min_depth\t";
    int32_t fill = 1 << (nm + 1);   // the mask of depth 0: NO_COVERAGE and every tested LOW bit
    for (size_t m = 0; m < nm; m++) { text += (m ? "," : "") + c->measures[m] + "=" + std::to_string(c->min_depth[m]); if (c->min_depth[m] > 0) fill |= 1 << m; }
    text += "\n#max_aDP\t" + std::to_string(c->max_aDP) + "\n#chrom\tbeg\tend\tclass\ttarget\n";
    std::vector<uvcio_callable::Run> runs = c->runs;
    std::sort(runs.begin(), runs.end(), [](const uvcio_callable::Run &a, const uvcio_callable::Run &b) { return a.target != b.target ? a.target < b.target : a.beg < b.beg; });
    int64_t total = 0, callable_ = 0; std::vector<int64_t> per_bit(nb, 0);
    size_t at = 0;
    for (size_t t = 0; t < c->targets.size(); t++) {
        const ReportTarget &T = c->targets[t];
        int64_t open_beg = T.beg, open_end = T.beg; int32_t open_mask = 0;   // the line being joined: [open_beg, open_end), empty at first
        auto flush = [&]() {
            if (open_end <= open_beg) return;
            std::string cls;
            for (size_t b = 0; b < nb; b++) if (open_mask >> b & 1) { cls += (cls.empty() ? "" : ",") + c->bits[b]; per_bit[b] += open_end - open_beg; }
            if (open_mask == 0) { cls = "CALLABLE"; callable_ += open_end - open_beg; }
            total += open_end - open_beg;
            text += T.chrom + "\t" + std::to_string(open_beg) + "\t" + std::to_string(open_end) + "\t" + cls + "\t" + T.name + "\n";
        };
        auto put = [&](int64_t a, int64_t b, int32_t mask) {
            if (b <= a) return;
            if (open_end > open_beg && mask == open_mask && a == open_end) { open_end = b; return; }
            flush();
            open_beg = a; open_end = b; open_mask = mask;
        };
        int64_t pos = T.beg;
        for (; at < runs.size() && runs[at].target == (int32_t)t; at++) {
            if (runs[at].beg < pos) return fail(UVCGPU_EINVAL, "callable report: the pieces of target " + std::to_string(t) + " overlap at " + std::to_string(runs[at].beg));
            put(pos, runs[at].beg, fill);
            put(runs[at].beg, runs[at].end, runs[at].mask);
            pos = runs[at].end;
        }
        put(pos, T.end, fill);
        flush();
    }
    text += "#summary\tpositions\t" + std::to_string(total) + "\n#summary\tCALLABLE\t" + std::to_string(callable_) + "\n";
    for (size_t b = 0; b < nb; b++) text += "#summary\t" + c->bits[b] + "\t" + std::to_string(per_bit[b]) + "\n";
    return write_text(path, text);
}
extern "C" void uvcio_callable_close(uvcio_callable_t *c) { delete c; }

// ---------------------------------------------------------------- the microsatellite tally ----
struct uvcio_msi {
    int32_t min_tracklen = 0, min_units = 0, max_unitlen = 0, min_depth = 0, unstable_permille = 0;
    struct Locus { int32_t target; std::string unit; int32_t w[UVC_MSI_ROW]; };   // kept to the end: the file is written in target order
    std::vector<ReportTarget> targets; std::vector<Locus> loci;
    std::mutex mu;
};
static const char *const MSI_LEVELS[UVC_MSI_NLEVEL] = { "b", "c", "c2", "d" };   // beside bDP, cDP12, cDP2, dDP1: fragments, families, consensus families, duplex families
extern "C" int uvcio_msi_open(uvcio_msi_t **out, int32_t min_tracklen, int32_t min_units, int32_t max_unitlen, int32_t min_depth, int32_t unstable_permille) {
    if (!out || min_tracklen < 1 || min_units < 1 || max_unitlen < 1 || min_depth < 1 || unstable_permille < 0) return fail(UVCGPU_EINVAL, "msi report: bad argument");
    uvcio_msi *m = new uvcio_msi;
    m->min_tracklen = min_tracklen; m->min_units = min_units; m->max_unitlen = max_unitlen; m->min_depth = min_depth; m->unstable_permille = unstable_permille;
    *out = m;
    return 0;
}
extern "C" int64_t uvcio_msi_add_target(uvcio_msi_t *m, const char *chrom, int64_t beg, int64_t end, const char *name) {
    if (!m || !chrom || beg < 0 || end > INT32_MAX) return fail(UVCGPU_EINVAL, "msi report: bad target");
    std::lock_guard<std::mutex> g(m->mu);
    m->targets.push_back(report_target(chrom, name, beg, std::max(beg, end)));
    return (int64_t)m->targets.size() - 1;
}
extern "C" int uvcio_msi_add(uvcio_msi_t *m, const int64_t *target_of_range, int64_t n_ranges, const int32_t *loci, const char *const *units, int64_t n_loci) {
    if (!m || n_loci < 0 || n_ranges < 0 || (n_loci > 0 && (!loci || !units || !target_of_range))) return fail(UVCGPU_EINVAL, "msi report: bad loci");
    std::lock_guard<std::mutex> g(m->mu);
    for (int64_t q = 0; q < n_loci; q++) {   // all of the call's loci or none
        const int32_t *w = loci + q * UVC_MSI_ROW;
        if (w[0] < 0 || w[0] >= n_ranges) return fail(UVCGPU_EINVAL, "msi report: locus " + std::to_string(q) + " names range " + std::to_string(w[0]) + " of " + std::to_string(n_ranges));
        const int64_t t = target_of_range[w[0]];
        if (t < 0 || t >= (int64_t)m->targets.size()) return fail(UVCGPU_EINVAL, "msi report: locus of target " + std::to_string(t) + ", which does not exist");
        if (w[1] < m->targets[(size_t)t].beg || w[1] >= m->targets[(size_t)t].end || w[2] < 1 || w[3] < 1 || !units[q])
            return fail(UVCGPU_EINVAL, "msi report: locus " + std::to_string(q) + " at " + std::to_string(w[1]) + " begins outside target " + std::to_string(t) + " or has no unit");
    }
    for (int64_t q = 0; q < n_loci; q++) {
        uvcio_msi::Locus l; l.target = (int32_t)target_of_range[loci[q * UVC_MSI_ROW]]; l.unit = units[q];
        memcpy(l.w, loci + q * UVC_MSI_ROW, sizeof(l.w));
        m->loci.push_back(l);
    }
    return 0;
}
extern "C" int64_t uvcio_msi_n_loci(const uvcio_msi_t *m) { return m ? (int64_t)m->loci.size() : 0; }
extern "C" int uvcio_msi_write(const uvcio_msi_t *m, const char *path) {
    if (!m || !path || !*path) return fail(UVCGPU_EINVAL, "msi report: bad argument");
    std::string text = "##msi_loci=1\n"
        "## A tally for a downstream classifier that has a baseline, NOT an MSI call: per microsatellite of the caller's own repeat tracks the\n"
        "## smallest depth along the tract and the InDel alleles that change its length by whole units (shifted) or otherwise (other), per\n"
        "## evidence level: b fragments, c UMI families, c2 consensus families, d duplex families.  A heterozygous germline length allele counts\n"
        "## as shifted.  EDGE: the tract touches the end of the region it was seen in; nothing was counted.\n";
    text += "#min_tract\t" + std::to_string(m->min_tracklen) + "\n#min_units\t" + std::to_string(m->min_units) + "\n#max_unit\t" + std::to_string(m->max_unitlen) +
            "\n#min_depth\t" + std::to_string(m->min_depth) + "\n#unstable_permille\t" + std::to_string(m->unstable_permille) + "\n";
    text += "#chrom\tbeg\tend\tunit\tunitlen\tunits\ttarget\tflags";
    for (int l = 0; l < UVC_MSI_NLEVEL; l++) {
        const std::string L = MSI_LEVELS[l];
        text += "\t" + L + "_depth\t" + L + "_shifted\t" + L + "_other";
        for (int b = 0; b < UVC_MSI_OTHER; b++) { const int sh = b < UVC_MSI_MAXSHIFT ? b - UVC_MSI_MAXSHIFT : b - UVC_MSI_MAXSHIFT + 1; text += "\t" + L + (sh < 0 ? "_m" : "_p") + std::to_string(sh < 0 ? -sh : sh); }
    }
    text += "\n";
    std::vector<const uvcio_msi::Locus *> order;
    for (const uvcio_msi::Locus &l : m->loci) order.push_back(&l);
    std::sort(order.begin(), order.end(), [](const uvcio_msi::Locus *a, const uvcio_msi::Locus *b) { return a->target != b->target ? a->target < b->target : a->w[1] < b->w[1]; });
    int64_t n_edge = 0, assessable[UVC_MSI_NLEVEL] = { 0, 0, 0, 0 }, unstable[UVC_MSI_NLEVEL] = { 0, 0, 0, 0 };
    for (const uvcio_msi::Locus *l : order) {
        const ReportTarget &T = m->targets[(size_t)l->target];
        const int32_t *w = l->w;
        const bool edge = (w[4] & UVC_MSI_EDGE) != 0;
        n_edge += edge;
        text += T.chrom + "\t" + std::to_string(w[1]) + "\t" + std::to_string((int64_t)w[1] + w[2]) + "\t" + l->unit + "\t" + std::to_string(w[3]) + "\t" + std::to_string(w[2] / w[3]) + "\t" + T.name + "\t" + (edge ? "EDGE" : ".");
        for (int lv = 0; lv < UVC_MSI_NLEVEL; lv++) {
            const int32_t *h = w + UVC_MSI_HIST + lv * UVC_MSI_NBIN;
            int64_t shifted = 0;
            for (int b = 0; b < UVC_MSI_OTHER; b++) shifted += h[b];
            const int64_t depth = w[UVC_MSI_DEPTH + lv];
            text += "\t" + std::to_string(depth) + "\t" + std::to_string(shifted) + "\t" + std::to_string(h[UVC_MSI_OTHER]);
            for (int b = 0; b < UVC_MSI_OTHER; b++) text += "\t" + std::to_string(h[b]);
            if (!edge && depth >= m->min_depth) { assessable[lv]++; if (1000 * shifted >= (int64_t)m->unstable_permille * depth) unstable[lv]++; }
        }
        text += "\n";
    }
    text += "#summary\tloci\t" + std::to_string(order.size()) + "\n#summary\tloci_EDGE\t" + std::to_string(n_edge) + "\n";
    for (int lv = 0; lv < UVC_MSI_NLEVEL; lv++) text += std::string("#summary\t") + MSI_LEVELS[lv] + "\tassessable\t" + std::to_string(assessable[lv]) + "\tunstable\t" + std::to_string(unstable[lv]) + "\n";
    return write_text(path, text);
}
extern "C" void uvcio_msi_close(uvcio_msi_t *m) { delete m; }
