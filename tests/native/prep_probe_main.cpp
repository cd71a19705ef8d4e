// prep_probe_main.cpp -- calls the internal entry points of the device read preparation (uvc_prep_reads, uvc_prep_compact,
// uvc_sort_by_pos_cls, uvc_launch_rank_from_sorted, uvc_launch_gather4) of libuvcgpu.so with plain device buffers, for
// tests/test_gpu_prep_units.py.  The structs and prototypes come from uvc_prep.h / uvc_launch.h themselves, so the compiler
// checks every layout this file uses; the test sees columns only.
//
//   prep_probe <prep|compact|sort> DIR [DIR ...]
//
// Every DIR holds scalars.txt ("name value" lines) and the input columns as raw little-endian files in_<name>.bin; the outputs
// go to out_<name>.bin and out_scalars.txt of the same DIR.  Everything runs on the null stream with hipMalloc as the allocator.
// Exit status 0, or 1 with the message on stderr.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "uvc_prep.h"
#include "uvc_launch.h"

static void die(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt);
    fprintf(stderr, "prep_probe: "); vfprintf(stderr, fmt, ap); fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) die("%s: %s", #call, hipGetErrorString(e_)); } while (0)

static std::vector<void *> g_owned;   // everything this run allocated on the device
static void *dev_alloc(size_t bytes, bool zero) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) return nullptr;
    if (zero && hipMemset(p, 0, bytes ? bytes : 8) != hipSuccess) return nullptr;
    g_owned.push_back(p);
    return p;
}
static void *prep_alloc(void *, size_t bytes, int zero) { return dev_alloc(bytes, zero != 0); }
static void free_all() { for (void *p : g_owned) hipFree(p); g_owned.clear(); }

struct Scalars {
    std::map<std::string, long long> v;
    long long get(const char *k) const { auto it = v.find(k); if (it == v.end()) die("scalars.txt has no %s", k); return it->second; }
    long long get(const char *k, long long dflt) const { auto it = v.find(k); return it == v.end() ? dflt : it->second; }
};
static Scalars read_scalars(const std::string &dir) {
    Scalars s;
    FILE *f = fopen((dir + "/scalars.txt").c_str(), "r");
    if (!f) die("cannot open %s/scalars.txt", dir.c_str());
    char name[128]; long long val;
    while (fscanf(f, "%127s %lld", name, &val) == 2) s.v[name] = val;
    fclose(f);
    return s;
}
// in_<name>.bin -> a device array of exactly `count` elements of T (the file's size is checked)
template <class T> static T *load(const std::string &dir, const char *name, long long count) {
    const std::string path = dir + "/in_" + name + ".bin";
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die("cannot open %s", path.c_str());
    std::vector<T> h((size_t)(count > 0 ? count : 0));
    const size_t got = h.empty() ? 0 : fread(h.data(), sizeof(T), h.size(), f);
    const bool more = (fgetc(f) != EOF);
    fclose(f);
    if (got != h.size() || more) die("%s does not hold %lld elements of %zu bytes", path.c_str(), count, sizeof(T));
    T *d = (T *)dev_alloc(sizeof(T) * h.size(), false);
    if (!d) die("hipMalloc(%s)", name);
    if (!h.empty()) HIP(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return d;
}
template <class T> static std::vector<T> fetch(const T *d, long long count) {
    std::vector<T> h((size_t)(count > 0 ? count : 0));
    if (!h.empty()) HIP(hipMemcpy(h.data(), d, sizeof(T) * h.size(), hipMemcpyDeviceToHost));
    return h;
}
template <class T> static void save_host(const std::string &dir, const std::string &name, const std::vector<T> &h) {
    const std::string path = dir + "/out_" + name + ".bin";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("cannot write %s", path.c_str());
    if (!h.empty() && fwrite(h.data(), sizeof(T), h.size(), f) != h.size()) die("short write to %s", path.c_str());
    fclose(f);
}
template <class T> static void save(const std::string &dir, const std::string &name, const T *d, long long count) { save_host(dir, name, fetch(d, count)); }
// one field of an array of records as a column
template <class R, class F> static void save_field(const std::string &dir, const std::string &name, const std::vector<R> &recs, F R::*field) {
    std::vector<F> col(recs.size());
    for (size_t i = 0; i < recs.size(); i++) col[i] = recs[i].*field;
    save_host(dir, name, col);
}
template <class T> static T *filled(long long count, T value) {
    std::vector<T> h((size_t)(count > 0 ? count : 0), value);
    T *d = (T *)dev_alloc(sizeof(T) * h.size(), false);
    if (!d) die("hipMalloc");
    if (!h.empty()) HIP(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return d;
}

static void run_prep(const std::string &dir) {
    const Scalars S = read_scalars(dir);
    UvcPrepIn in; memset(&in, 0, sizeof(in));
    const long long n = S.get("n_reads");
    in.n_reads = n; in.n_bases = S.get("n_bases"); in.n_cigar_ops = S.get("n_cigar_ops"); in.n_fams = (int32_t)S.get("n_fams");
    in.pos = load<int32_t>(dir, "pos", n); in.mpos = load<int32_t>(dir, "mpos", n); in.isize = load<int32_t>(dir, "isize", n); in.nm = load<int32_t>(dir, "nm", n);
    in.l_qseq = load<int32_t>(dir, "l_qseq", n); in.n_cigar = load<int32_t>(dir, "n_cigar", n); in.frag_id = load<int32_t>(dir, "frag_id", n); in.fam_id = load<int32_t>(dir, "fam_id", n);
    in.flag = load<uint16_t>(dir, "flag", n); in.mapq = load<uint8_t>(dir, "mapq", n); in.fam_strand = load<uint8_t>(dir, "fam_strand", n);
    in.fam_dflag = load<uint8_t>(dir, "fam_dflag", in.n_fams);
    in.seq_off = load<int64_t>(dir, "seq_off", n); in.cigar_off = load<int64_t>(dir, "cigar_off", n);
    in.cigars = load<uint32_t>(dir, "cigars", in.n_cigar_ops); in.quals = load<uint8_t>(dir, "quals", in.n_bases);
    const long long zq = S.get("zero_qual", -1);   // -1: UvcPrepIn::zero_qual NULL, else the value of the device word
    in.zero_qual = (zq < 0 ? nullptr : filled<int32_t>(1, (int32_t)zq));
    // the parameters as region.default_params makes them, and the few fields the preparation reads that a case moves
    UvcParams P;
    uvcgpu_params_default(&P);
    uvcgpu_params_apply_platform(&P, (int32_t)S.get("platform"), 150, 60);
    if (S.v.count("fam_thres_dup1add")) P.fam_thres_dup1add = (int32_t)S.get("fam_thres_dup1add");
    if (S.v.count("bias_thres_interfering_indel")) P.bias_thres_interfering_indel = (int32_t)S.get("bias_thres_interfering_indel");
    const int32_t rbeg = (int32_t)S.get("rbeg"), rend = (int32_t)S.get("rend");
    const long long npos = S.get("npos");
    UvcPrepOut o; char msg[256] = "";
    const int rc = uvc_prep_reads(&in, &P, rbeg, rend, npos, prep_alloc, nullptr, (hipStream_t)0, &o, msg, (int)sizeof(msg));
    if (rc != 0) die("uvc_prep_reads: %d: %s", rc, msg);
    HIP(hipDeviceSynchronize());
    save(dir, "endpos", o.endpos, n); save(dir, "kind", o.kind, n); save(dir, "dflag_of", o.dflag_of, n); save(dir, "frag_of", o.frag_of, n); save(dir, "fs_of", o.fs_of, n);
    save(dir, "p2_first", o.p2_first, n); save(dir, "complex_ids", o.complex_ids, o.n_complex);
    save(dir, "table_off", o.table_off, n); save(dir, "item_off", o.item_off, n); save(dir, "gap_off", o.gap_off, n);
    save(dir, "frag_beg", o.frag_beg, o.n_frags); save(dir, "frag_strand", o.frag_strand, o.n_frags);
    {
        const std::vector<FragRec> f = fetch(o.frags, o.n_frags);
        save_field(dir, "frags.aln_beg", f, &FragRec::aln_beg); save_field(dir, "frags.aln_end", f, &FragRec::aln_end); save_field(dir, "frags.beg", f, &FragRec::beg);
        save_field(dir, "frags.end", f, &FragRec::end); save_field(dir, "frags.fs", f, &FragRec::fs); save_field(dir, "frags.strand", f, &FragRec::strand);
        save_field(dir, "frags.dflag", f, &FragRec::dflag); save_field(dir, "frags.normMQ", f, &FragRec::normMQ); save_field(dir, "frags.n_cov", f, &FragRec::n_cov);
        save_field(dir, "frags.n_near", f, &FragRec::n_near); save_field(dir, "frags.singleton", f, &FragRec::singleton); save_field(dir, "frags.stat_kind", f, &FragRec::stat_kind);
    }
    {
        const std::vector<FsRec> u = fetch(o.fss, o.n_fs);
        save_field(dir, "fss.frag_beg", u, &FsRec::frag_beg); save_field(dir, "fss.frag_end", u, &FsRec::frag_end); save_field(dir, "fss.beg", u, &FsRec::beg);
        save_field(dir, "fss.end", u, &FsRec::end); save_field(dir, "fss.strand", u, &FsRec::strand); save_field(dir, "fss.dflag", u, &FsRec::dflag);
        save_field(dir, "fss.fam", u, &FsRec::fam); save_field(dir, "fss.generic", u, &FsRec::generic); save_field(dir, "fss.work_off", u, &FsRec::work_off);
        save_field(dir, "fss.other_fs", u, &FsRec::other_fs);
    }
    save(dir, "generic_fs", o.generic_fs, o.n_generic); save(dir, "generic_sorted", o.generic_sorted, o.n_generic); save(dir, "sweep_frags", o.sweep_frags, o.n_sweep);
    save(dir, "dup_units", o.dup_units, o.n_dup); save(dir, "dup_off", o.dup_off, o.n_dup);
    save(dir, "p2_aln", o.p2_aln, o.n_p2); save(dir, "p2_beg", o.p2_beg, o.n_p2); save(dir, "p2_end", o.p2_end, o.n_p2); save(dir, "p2_qb", o.p2_qb, o.n_p2); save(dir, "p2_cls", o.p2_cls, o.n_p2);
    FILE *f = fopen((dir + "/out_scalars.txt").c_str(), "w");
    if (!f) die("cannot write %s/out_scalars.txt", dir.c_str());
#define SC(name) fprintf(f, "%s %lld\n", #name, (long long)o.name)
    SC(n_frags); SC(n_fs); SC(n_complex); SC(n_simple); SC(n_generic); SC(n_dup); SC(n_sweep); SC(n_frag_strand0);
    SC(max_frag_span); SC(max_unit_span); SC(max_unit_frags); SC(max_p2_span); SC(max_frag_depth); SC(any_amplicon);
    SC(p2_off[0]); SC(p2_off[1]); SC(p2_off[2]); SC(p2_off[3]); SC(p2_off[4]);
    SC(n_p2); SC(table_rows); SC(item_slots); SC(gap_slots); SC(ins_total); SC(work); SC(dup_work);
#undef SC
    fprintf(f, "zero_value_qual %d\n", uvc_prep_zero_value_qual(&P));
    fclose(f);
}

// the three offset columns of the compact input form; the packed bases and the qualities are zero bytes of the right lengths (the
// kernel that unpacks them runs behind the offsets and is not what this mode is about)
static void run_compact(const std::string &dir) {
    const Scalars S = read_scalars(dir);
    const long long n = S.get("n_reads"), n_bases = S.get("n_bases"), n_b4 = S.get("n_b4");
    const int32_t *lq = load<int32_t>(dir, "l_qseq", n), *nc = load<int32_t>(dir, "n_cigar", n);
    uint8_t *b4 = (uint8_t *)dev_alloc((size_t)n_b4, true), *quals = (uint8_t *)dev_alloc((size_t)n_bases, true), *bases = (uint8_t *)dev_alloc((size_t)n_bases, true);
    uint16_t *bq = (uint16_t *)dev_alloc(2 * (size_t)n_bases, true);
    int64_t *so = filled<int64_t>(n, -7), *co = filled<int64_t>(n, -7), *bo = filled<int64_t>(n, -7);
    int32_t *bad = (int32_t *)dev_alloc(8, true);
    const size_t tb = uvc_prep_compact_tmp_bytes(n);
    void *tmp = dev_alloc(tb, false);
    if (!b4 || !quals || !bases || !bq || !bad || !tmp) die("hipMalloc");
    const int e = uvc_prep_compact(lq, nc, n, n_bases, b4, n_b4, quals, so, nullptr, co, bo, bases, bq, bad, tmp, tb, (hipStream_t)0);
    if (e) die("uvc_prep_compact: %s", hipGetErrorString((hipError_t)e));
    HIP(hipDeviceSynchronize());
    HIP(hipGetLastError());
    save(dir, "seq_off", so, n); save(dir, "cigar_off", co, n); save(dir, "b4_off", bo, n);
    const std::vector<int32_t> hb = fetch(bad, 2);
    FILE *f = fopen((dir + "/out_scalars.txt").c_str(), "w");
    if (!f) die("cannot write %s/out_scalars.txt", dir.c_str());
    fprintf(f, "bad %d\n", hb[0]);
    fclose(f);
}

// one sort; behind it n_ranks runs of the rank scatter (n_first_<k>) and n_gathers runs of the gather (g<k>_n_alns, in_g<k>_kind,
// in_g<k>_a0 .. a3); every output the two scatters do not write keeps the sentinel the test names
static void run_sort(const std::string &dir) {
    const Scalars S = read_scalars(dir);
    const long long n = S.get("n");
    const int32_t sentinel = (int32_t)S.get("sentinel");
    const int32_t *pos = load<int32_t>(dir, "pos", n), *cls = load<int32_t>(dir, "cls", n);
    uint32_t *work = (uint32_t *)dev_alloc(sizeof(uint32_t) * 4 * (size_t)n, true);
    const size_t tb = uvc_sort32_tmp_bytes((size_t)n);
    void *tmp = dev_alloc(tb + 16, false);
    if (!work || !tmp) die("hipMalloc");
    if (uvc_sort_by_pos_cls(pos, cls, (int32_t)S.get("beg"), (int)S.get("pos_bits"), (int)S.get("cls_bits"), n, work, tmp, tb, (hipStream_t)0) != 0) die("uvc_sort_by_pos_cls failed");
    HIP(hipDeviceSynchronize());
    const uint32_t *perm = work + 3 * (size_t)n;
    save(dir, "perm", perm, n);
    for (int k = 0; k < (int)S.get("n_ranks"); k++) {
        const std::string tag = std::to_string(k);
        int32_t *ids = filled<int32_t>(n, sentinel), *rank = filled<int32_t>(n, sentinel);
        uvc_launch_rank_from_sorted(perm, n, S.get(("n_first_" + tag).c_str()), ids, rank, (hipStream_t)0);
        HIP(hipDeviceSynchronize());
        save(dir, "ids_" + tag, ids, n); save(dir, "rank_" + tag, rank, n);
    }
    for (int k = 0; k < (int)S.get("n_gathers"); k++) {
        const std::string g = "g" + std::to_string(k);
        const long long n_alns = S.get((g + "_n_alns").c_str());
        const int32_t *kind = load<int32_t>(dir, (g + "_kind").c_str(), n_alns);
        const int32_t *a[4]; int32_t *o[4];
        for (int c = 0; c < 4; c++) { a[c] = load<int32_t>(dir, (g + "_a" + std::to_string(c)).c_str(), n); o[c] = filled<int32_t>(n, sentinel); }
        int32_t *slot = filled<int32_t>(n_alns, sentinel);
        uvc_launch_gather4(perm, n, a[0], a[1], a[2], a[3], o[0], o[1], o[2], o[3], kind, n_alns, slot, (hipStream_t)0);
        HIP(hipDeviceSynchronize());
        for (int c = 0; c < 4; c++) save(dir, g + "_o" + std::to_string(c), o[c], n);
        save(dir, g + "_slot", slot, n_alns);
    }
    HIP(hipGetLastError());
}

int main(int argc, char **argv) {
    if (argc < 3) die("usage: prep_probe <prep|compact|sort> DIR [DIR ...]");
    const std::string mode = argv[1];
    if (mode != "prep" && mode != "compact" && mode != "sort") die("unknown mode %s", argv[1]);
    if (uvcgpu_init(0) != 0) die("uvcgpu_init: %s", uvcgpu_last_error());
    for (int k = 2; k < argc; k++) {
        if (mode == "prep") run_prep(argv[k]); else if (mode == "compact") run_compact(argv[k]); else run_sort(argv[k]);
        free_all();
    }
    return 0;
}
