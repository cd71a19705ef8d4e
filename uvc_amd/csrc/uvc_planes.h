// uvc_planes.h -- the plane groups of a region handle (include/uvc_field_groups.def), each fact once: planes, element size and bytes of a
// group, the columns of a fetched row, the layout of the plane slab, the rows of the zero-fill table and the RegionDev member a slab
// group is bound to.  No memory access and no HIP type in here, so the same text compiles for the host alone
// (tests/native/planes_host_main.cpp sweeps the layout there) and into the kernels' translation units (uvc_device.h includes it).
// To add a plane: the UVC_N<name> count and the row's `fields`.  To add a slab group: a row of the .def, the pointer in RegionDev and its
// entry in UVC_SLAB_MEMBERS (the count below does not compile without it); layout, fill, columns and the dirty check follow.
#ifndef UVC_PLANES_H
#define UVC_PLANES_H

#include <stddef.h>
#include <stdint.h>
#include "uvcgpu.h"
#include "uvc_rules.h"

#define NSYM UVC_NUM_SYMBOLS
#define NBUCKETS 16          // NUM_BUCKETS, main_conversion.hpp:920

// `fill` of a row: -1 as ZeroPlane::fam has it, 0..2 the plane family of RegionDev::dirty
enum { UVC_FILL_NONE = -2, UVC_FILL_ALWAYS = -1, UVC_FILL_CORE = 0, UVC_FILL_FAMINFO = 1, UVC_FILL_DUPLEX = 2, UVC_N_DIRTY_FAMILIES = 3 };
enum { UVC_NBQSUM = 1, UVC_NBAQ = 2 };   // the two groups whose plane count uvcgpu.h gives in words only
struct UvcGroup { const char *name; int elem, fields, strands, per_symbol, fill; };
constexpr UvcGroup UVC_GROUPS[] = {
#define UVC_GROUP(name, elem, fields, strands, per_symbol, fill) { #name, elem, fields, strands, per_symbol, UVC_FILL_##fill },
#include "uvc_field_groups.def"
#undef UVC_GROUP
};
static_assert(sizeof(UVC_GROUPS) / sizeof(UVC_GROUPS[0]) == UVC_NUM_FIELD_GROUPS, "one row per UVC_F_ id");
enum {
#define UVC_GROUP(name, elem, fields, strands, per_symbol, fill) UVC_GROUP_ROW_##name,
#include "uvc_field_groups.def"
#undef UVC_GROUP
};
#define UVC_GROUP(name, elem, fields, strands, per_symbol, fill) \
    static_assert(UVC_GROUP_ROW_##name == UVC_F_##name && (fields) == UVC_N##name && ((elem) == 4 || (elem) == 8) && ((strands) == 1 || (strands) == 2) && (UVC_FILL_##fill < 0 || (per_symbol)), \
                  "row " #name " of uvc_field_groups.def: the rows are in UVC_F_ order, `fields` is UVC_N" #name ", and only a per-symbol group has a dirty family");
#include "uvc_field_groups.def"
#undef UVC_GROUP

constexpr bool uvc_group_in_slab(int g) { return UVC_GROUPS[g].fill != UVC_FILL_NONE; }
constexpr int uvc_group_elem(int g) { return UVC_GROUPS[g].elem; }
constexpr int uvc_group_sym_planes(int g) { return UVC_GROUPS[g].strands * UVC_GROUPS[g].fields; }   // planes per symbol of a per-symbol group
constexpr int uvc_group_planes(int g) { return uvc_group_sym_planes(g) * (UVC_GROUPS[g].per_symbol ? NSYM : 1); }
constexpr size_t uvc_group_bytes(int g, int64_t npos) { return (size_t)uvc_group_elem(g) * (size_t)npos * (size_t)uvc_group_planes(g); }
// a row of uvcgpu_region_fetch_columns: the planes of the slab groups in id order (a group outside the slab has no columns: first column -1)
constexpr int uvc_group_columns(int g) { return uvc_group_in_slab(g) ? uvc_group_planes(g) : 0; }
constexpr int uvc_columns_before(int g) { int at = 0; for (int q = 0; q < g; q++) at += uvc_group_columns(q); return at; }
constexpr int uvc_group_first_column(int g) { return uvc_group_in_slab(g) ? uvc_columns_before(g) : -1; }
constexpr int UVC_N_COLUMNS = uvc_columns_before(UVC_NUM_FIELD_GROUPS);

// The plane slab of a handle: the 8-byte groups in id order, then the 4-byte groups in id order, then one byte per (strand, position) that
// says a P5 bucket was filled (k_p5b skips the others), RegionDev::occ, and the transient bucket planes.  off[] of a group outside the slab is 0.
struct SlabLayout { size_t off[UVC_NUM_FIELD_GROUPS]; size_t p5flag_off, occ_off, bucket_off, total; };
constexpr size_t uvc_align256(size_t n) { return (n + 255) & ~(size_t)255; }
constexpr SlabLayout slab_layout(int64_t npos) {
    SlabLayout L = {};
    size_t o = 0;
    for (int elem = 8; elem >= 4; elem -= 4)
        for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) if (uvc_group_in_slab(g) && uvc_group_elem(g) == elem) { L.off[g] = o; o += uvc_group_bytes(g, npos); }
    L.p5flag_off = o; o += uvc_align256((size_t)2 * npos);
    L.occ_off = o; o += uvc_align256((size_t)4 * npos);
    L.bucket_off = o; o += (size_t)4 * npos * 2 * NSYM * NBUCKETS;
    L.total = o;
    return L;
}

// one plane of the slab for k_zero_state; fam < 0: always filled, else the (plane family, sym) of RegionDev::dirty that says whether to
struct ZeroPlane { unsigned long long off; int32_t elem; int16_t fam, sym; };
static_assert(sizeof(ZeroPlane) == 16, "the host uploads the plane table as 16-byte rows");
constexpr int UVC_N_ZERO_PLANES = UVC_N_COLUMNS + 3;   // every plane in front of the buckets: the groups', the two of p5flag, occ
// The table of a layout into out[UVC_N_ZERO_PLANES].  (k_thres stores every threshold of every position, but a handle that is rebound to a
// region of another length relies on an all-zero slab: THRES is filled like the rest.)
inline void zero_plane_rows(const SlabLayout &L, int64_t npos, ZeroPlane *out) {
    const size_t n = (size_t)npos;
    int k = 0;
    for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) {
        if (!uvc_group_in_slab(g)) continue;
        const UvcGroup &G = UVC_GROUPS[g];
        for (int pl = 0; pl < uvc_group_planes(g); pl++) {
            const int sy = (G.per_symbol ? pl % NSYM : 0);
            const bool always = (G.fill == UVC_FILL_ALWAYS || (G.fill == UVC_FILL_CORE && sym_always_filled(sy)));
            out[k++] = ZeroPlane{ (unsigned long long)(L.off[g] + (size_t)pl * n * G.elem), G.elem, (int16_t)(always ? -1 : G.fill), (int16_t)sy };
        }
    }
    out[k++] = ZeroPlane{ (unsigned long long)L.p5flag_off, 1, -1, 0 };
    out[k++] = ZeroPlane{ (unsigned long long)(L.p5flag_off + n), 1, -1, 0 };
    out[k++] = ZeroPlane{ (unsigned long long)L.occ_off, 4, -1, 0 };
}

// the RegionDev member of every slab group: X(group, member)
#define UVC_SLAB_MEMBERS(X) \
    X(PREP32, prep32) X(PREP64, prep64) X(THRES, thres) X(SEG32, seg32) X(SEG64, seg64) X(VQ, vq) X(BQSUM, bqsum) X(FRAG, frag) X(FAM, fam) \
    X(FAMINFO32, faminfo32) X(FAMINFO64, faminfo64) X(DUPLEX, duplex)
constexpr int uvc_n_slab_groups() { int n = 0; for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++) n += uvc_group_in_slab(g); return n; }
#define X(g, m) + (uvc_group_in_slab(UVC_F_##g) ? 1 : -UVC_NUM_FIELD_GROUPS)
static_assert(0 UVC_SLAB_MEMBERS(X) == uvc_n_slab_groups(), "UVC_SLAB_MEMBERS names as many groups as the slab has, every one of them a slab group");
#undef X
#endif
