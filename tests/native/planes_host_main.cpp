// Host check of uvc_amd/csrc/uvc_planes.h (tests/test_planes_cpu.py builds this with -fsanitize=undefined,address and runs it).
// For npos in {1, 63, 64, 65, 4095, 4096, 4097, 1 000 001, 2^29 - 1}:
//   1. every group offset, p5flag_off, occ_off, bucket_off and the total against the formulas of the commit before this header existed,
//      restated here (the bytes of a group spelled out per group, the hand-written order of the groups), and for two of the lengths against
//      literals that commit's code printed; 8-byte groups on 8-byte offsets;
//   2. bytes, first column and column count of every group against that commit's values (the columns as literals);
//   3. the rows of the zero-fill table: the same (off, elem, fam, sym) set as that commit's loops made, pairwise disjoint, covering every
//      byte in front of the bucket planes but the alignment padding behind p5flag and occ, and fam / sym by the rule.
#include <algorithm>
#include <cstdio>
#include <tuple>
#include <vector>
#include "../../uvc_amd/csrc/uvc_planes.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const long long NPOS[9] = { 1, 63, 64, 65, 4095, 4096, 4097, 1000001, ((long long)1 << 29) - 1 };

// ---- the commit before: group_bytes(), group_planes() / group_elem(), the order[] of configure_region ----
static size_t old_group_bytes(size_t n, int g) {
    switch (g) {
        case UVC_F_PREP32: return 4 * n * UVC_NPREP32;
        case UVC_F_PREP64: return 8 * n * UVC_NPREP64;
        case UVC_F_THRES: return 4 * n * UVC_NTHRES;
        case UVC_F_SEG32: return 4 * n * UVC_NSEG32 * 14;
        case UVC_F_SEG64: return 8 * n * UVC_NSEG64 * 14;
        case UVC_F_VQ: return 4 * n * UVC_NVQ * 14;
        case UVC_F_BQSUM: return 4 * n * 14;
        case UVC_F_FRAG: return 4 * n * 2 * UVC_NFRAG * 14;
        case UVC_F_FAM: return 4 * n * 2 * UVC_NFAM * 14;
        case UVC_F_FAMINFO32: return 4 * n * UVC_NFAMINFO32 * 14;
        case UVC_F_FAMINFO64: return 8 * n * UVC_NFAMINFO64 * 14;
        case UVC_F_DUPLEX: return 4 * n * UVC_NDUPLEX * 14;
        case UVC_F_RTR: return 4 * n * UVC_NRTR;
        case UVC_F_BAQ: return 8 * n * 2;
    }
    return 0;
}
struct OldLayout { size_t off[UVC_NUM_FIELD_GROUPS], p5flag_off, occ_off, bucket_off, total; };
static OldLayout old_layout(long long npos) {
    OldLayout L = {};
    const int order[] = { UVC_F_PREP64, UVC_F_SEG64, UVC_F_FAMINFO64, UVC_F_PREP32, UVC_F_THRES, UVC_F_SEG32, UVC_F_VQ, UVC_F_BQSUM, UVC_F_FRAG, UVC_F_FAM, UVC_F_FAMINFO32, UVC_F_DUPLEX };
    size_t o = 0;
    for (int g : order) { L.off[g] = o; o += old_group_bytes((size_t)npos, g); }
    L.p5flag_off = o; o += ((size_t)2 * npos + 255) & ~(size_t)255;
    L.occ_off = o; o += ((size_t)4 * npos + 255) & ~(size_t)255;
    L.bucket_off = o; o += (size_t)4 * npos * 2 * 14 * 16;
    L.total = o;
    return L;
}
// what that commit's code printed for two lengths: npos, off[14], p5flag_off, occ_off, bucket_off, total
struct Printed { long long npos; size_t off[UVC_NUM_FIELD_GROUPS], p5flag_off, occ_off, bucket_off, total; };
static const Printed PRINTED[2] = {
    { 4097LL, { 3146496u, 0u, 3572584u, 3867568u, 393312u, 10750528u, 13962576u, 14192008u, 15568600u, 19239512u, 2228768u, 22222128u, 0u, 0u }, 22680992u, 22689440u, 22706080u, 30047904u },
    { 1000001LL, { 768000768u, 0u, 872000872u, 944000944u, 96000096u, 2624002624u, 3408003408u, 3464003464u, 3800003800u, 4696004696u, 544000544u, 5424005424u, 0u, 0u }, 5536005536u, 5538005664u, 5542005920u, 7334007712u },
};
static const int OLD_N_COLUMNS = 1288;
static const int OLD_COLUMN_BASE[UVC_NUM_FIELD_GROUPS] = { 0, 26, 38, 56, 476, 532, 728, 742, 826, 1050, 1232, 1260, -1, -1 };

typedef std::tuple<unsigned long long, int, int, int> Row;   // off, elem, fam, sym
static std::vector<Row> old_zero_planes(const OldLayout &L, long long npos) {
    std::vector<Row> v;
    const size_t n = (size_t)npos;
    auto sym_planes = [&](int g, int nplanes, int elem, int fam) {
        for (int pl = 0; pl < nplanes; pl++) for (int sy = 0; sy < 14; sy++) {
            const bool always = (fam == 0 && (sy < UVC_BASE_NN || sy == UVC_LINK_M));
            v.push_back(Row{ (unsigned long long)(L.off[g] + ((size_t)pl * 14 + sy) * n * elem), elem, always ? -1 : fam, sy });
        }
    };
    for (int pl = 0; pl < UVC_NPREP32; pl++) v.push_back(Row{ (unsigned long long)(L.off[UVC_F_PREP32] + (size_t)pl * n * 4), 4, -1, 0 });
    for (int pl = 0; pl < UVC_NPREP64; pl++) v.push_back(Row{ (unsigned long long)(L.off[UVC_F_PREP64] + (size_t)pl * n * 8), 8, -1, 0 });
    for (int pl = 0; pl < UVC_NTHRES; pl++) v.push_back(Row{ (unsigned long long)(L.off[UVC_F_THRES] + (size_t)pl * n * 4), 4, -1, 0 });
    sym_planes(UVC_F_SEG32, UVC_NSEG32, 4, 0); sym_planes(UVC_F_SEG64, UVC_NSEG64, 8, 0); sym_planes(UVC_F_VQ, UVC_NVQ, 4, 0); sym_planes(UVC_F_BQSUM, 1, 4, 0);
    sym_planes(UVC_F_FRAG, 2 * UVC_NFRAG, 4, 0); sym_planes(UVC_F_FAM, 2 * UVC_NFAM, 4, 0);
    sym_planes(UVC_F_FAMINFO32, UVC_NFAMINFO32, 4, 1); sym_planes(UVC_F_FAMINFO64, UVC_NFAMINFO64, 8, 1); sym_planes(UVC_F_DUPLEX, UVC_NDUPLEX, 4, 2);
    v.push_back(Row{ (unsigned long long)L.p5flag_off, 1, -1, 0 }); v.push_back(Row{ (unsigned long long)(L.p5flag_off + n), 1, -1, 0 });
    v.push_back(Row{ (unsigned long long)L.occ_off, 4, -1, 0 });
    return v;
}

int main() {
    int n_layouts = 0, n_rows = 0, n_printed = 0;
    CHECK(UVC_N_COLUMNS == OLD_N_COLUMNS, "%d columns", UVC_N_COLUMNS);
    for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) CHECK(uvc_group_first_column(g) == OLD_COLUMN_BASE[g], "group %d: first column %d", g, uvc_group_first_column(g));
    for (long long npos : NPOS) {
        const SlabLayout L = slab_layout(npos);
        const OldLayout O = old_layout(npos);
        for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) {
            CHECK(L.off[g] == O.off[g], "npos %lld group %d: offset %zu, was %zu", npos, g, L.off[g], O.off[g]);
            CHECK(uvc_group_bytes(g, npos) == old_group_bytes((size_t)npos, g), "npos %lld group %d: %zu bytes", npos, g, uvc_group_bytes(g, npos));
            CHECK(uvc_group_elem(g) != 8 || L.off[g] % 8 == 0, "npos %lld group %d: an 8-byte group at %zu", npos, g, L.off[g]);
        }
        CHECK(L.p5flag_off == O.p5flag_off && L.occ_off == O.occ_off && L.bucket_off == O.bucket_off && L.total == O.total, "npos %lld: tail %zu %zu %zu %zu, was %zu %zu %zu %zu", npos,
              L.p5flag_off, L.occ_off, L.bucket_off, L.total, O.p5flag_off, O.occ_off, O.bucket_off, O.total);
        for (const Printed &P : PRINTED) if (P.npos == npos) {
            for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) CHECK(L.off[g] == P.off[g], "npos %lld group %d: offset %zu, printed %zu", npos, g, L.off[g], P.off[g]);
            CHECK(L.p5flag_off == P.p5flag_off && L.occ_off == P.occ_off && L.bucket_off == P.bucket_off && L.total == P.total, "npos %lld: the tail is not the printed one", npos);
            n_printed++;
        }
        n_layouts++;

        // the zero-fill table
        std::vector<ZeroPlane> z(UVC_N_ZERO_PLANES);
        zero_plane_rows(L, npos, z.data());
        std::vector<Row> now, old = old_zero_planes(O, npos);
        for (const ZeroPlane &p : z) now.push_back(Row{ p.off, p.elem, p.fam, p.sym });
        CHECK(now.size() == old.size(), "npos %lld: %zu rows, were %zu", npos, now.size(), old.size());
        std::sort(now.begin(), now.end()); std::sort(old.begin(), old.end());
        CHECK(now == old, "npos %lld: the rows are not the ones of the commit before", npos);
        // disjoint, and together every byte of [0, bucket_off) but the padding behind p5flag and occ (now is sorted by offset)
        unsigned long long at = 0;
        for (const Row &q : now) {
            const unsigned long long off = std::get<0>(q), len = (unsigned long long)std::get<1>(q) * (unsigned long long)npos;
            if (off == L.occ_off) { CHECK(at == L.p5flag_off + 2 * (unsigned long long)npos && off - at < 256, "npos %lld: occ at %llu behind %llu", npos, off, at); at = off; }
            CHECK(off == at, "npos %lld: a row at %llu, the one before ends at %llu", npos, off, at);
            at = off + len;
        }
        CHECK(at == L.occ_off + 4 * (unsigned long long)npos && L.bucket_off - at < 256, "npos %lld: the rows end at %llu, the buckets begin at %zu", npos, at, L.bucket_off);
        // fam / sym by the rule
        for (const ZeroPlane &p : z) {
            int g = -1;   // the group the row lies in, -1: p5flag / occ
            for (int q = 0; q < UVC_NUM_FIELD_GROUPS; q++) if (uvc_group_in_slab(q) && p.off >= L.off[q] && p.off < L.off[q] + uvc_group_bytes(q, npos)) g = q;
            const bool core = (g == UVC_F_SEG32 || g == UVC_F_SEG64 || g == UVC_F_VQ || g == UVC_F_BQSUM || g == UVC_F_FRAG || g == UVC_F_FAM);
            const bool dense = (p.sym == UVC_BASE_A || p.sym == UVC_BASE_C || p.sym == UVC_BASE_G || p.sym == UVC_BASE_T || p.sym == UVC_BASE_N || p.sym == UVC_LINK_M);
            int want = -1;
            if (core && !dense) want = 0;
            if (g == UVC_F_FAMINFO32 || g == UVC_F_FAMINFO64) want = 1;
            if (g == UVC_F_DUPLEX) want = 2;
            CHECK(p.fam == want, "npos %lld: the row at %llu (group %d, symbol %d) has family %d", npos, p.off, g, (int)p.sym, (int)p.fam);
            if (g < 0 || g == UVC_F_PREP32 || g == UVC_F_PREP64 || g == UVC_F_THRES) CHECK(p.sym == 0, "npos %lld: the row at %llu has symbol %d", npos, p.off, (int)p.sym);
            else CHECK((unsigned long long)p.sym == ((p.off - L.off[g]) / ((unsigned long long)p.elem * npos)) % 14, "npos %lld: the row at %llu has symbol %d", npos, p.off, (int)p.sym);
            CHECK(p.elem == (g < 0 ? (p.off < L.occ_off ? 1 : 4) : uvc_group_elem(g)), "npos %lld: the row at %llu has elements of %d bytes", npos, p.off, p.elem);
            n_rows++;
        }
    }
    printf("layouts %d, printed %d, zero-fill rows %d, %d failures\n", n_layouts, n_printed, n_rows, failures);
    return failures ? 1 : 0;
}
