// The parameter surface of libuvcgpu: one name table generated from include/uvc_params.def and include/uvc_group_params.def
// (uvcgpu_param_count / _info / _get / _set), and the value refusals of a region handle (uvcgpu_params_check).  Host code only.
#include "uvcgpu.h"
#include "uvcgroup.h"
#include "uvc_host.h"

#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>

namespace {
struct Row { const char *name; int32_t kind, owner; size_t off; double dflt; };

const Row ROWS[] = {
#define UVC_PI(name, dflt) { #name, UVC_PARAM_INT, UVC_PARAM_OF_PARAMS, offsetof(UvcParams, name), (double)(dflt) },
#define UVC_PD(name, dflt) { #name, UVC_PARAM_DOUBLE, UVC_PARAM_OF_PARAMS, offsetof(UvcParams, name), (double)(dflt) },
#include "uvc_params.def"
#undef UVC_PI
#undef UVC_PD
#define UVC_GI(name, dflt) { #name, UVC_PARAM_INT, UVC_PARAM_OF_GROUP, offsetof(UvcGroupParams, name), (double)(dflt) },
#define UVC_GD(name, dflt) { #name, UVC_PARAM_DOUBLE, UVC_PARAM_OF_GROUP, offsetof(UvcGroupParams, name), (double)(dflt) },
#include "uvc_group_params.def"
#undef UVC_GI
#undef UVC_GD
};
const int32_t N_ROWS = (int32_t)(sizeof(ROWS) / sizeof(ROWS[0]));

// Derived rows: what the platform step infers (inferred_*) and the two predicates on the tumor VCF's name (tumor_vcf_*, uvc_params.def)
// are set by the caller from facts, never by a user.
bool settable(const Row &r) { return strncmp(r.name, "inferred_", 9) != 0 && strncmp(r.name, "tumor_vcf_", 10) != 0; }

// field form or option form (every '-' an '_'); case kept, as CLI11 compares option names
int32_t find(const char *name) {
    for (int32_t i = 0; i < N_ROWS; i++) {
        const char *a = ROWS[i].name, *b = name;
        while (*a && (*a == *b || (*a == '_' && *b == '-'))) { a++; b++; }
        if (!*a && !*b) return i;
    }
    return -1;
}

bool parse_int(const char *s, int32_t *v) {
    if (!strcmp(s, "true")) { *v = 1; return true; }
    if (!strcmp(s, "false")) { *v = 0; return true; }
    if (!((*s >= '0' && *s <= '9') || ((*s == '-' || *s == '+') && s[1] >= '0' && s[1] <= '9'))) return false;
    char *end = nullptr; errno = 0;
    const long long x = strtoll(s, &end, 10);
    if (errno || *end || x < INT32_MIN || x > INT32_MAX) return false;
    *v = (int32_t)x;
    return true;
}

bool parse_double(const char *s, double *v) {
    if (!*s || *s == ' ' || *s == '\t' || *s == '\n') return false;
    char *end = nullptr; errno = 0;
    const double x = strtod(s, &end);
    if (errno || *end || !std::isfinite(x)) return false;
    *v = x;
    return true;
}
}   // namespace

extern "C" int32_t uvcgpu_param_count(void) { return N_ROWS; }

extern "C" int uvcgpu_param_info(int32_t i, const char **name, int32_t *kind, int32_t *owner, double *dflt, int32_t *can_set) {
    if (i < 0 || i >= N_ROWS) return uvcgpu_set_error(UVCGPU_EINVAL, "parameter row out of range");
    const Row &r = ROWS[i];
    if (name) *name = r.name;
    if (kind) *kind = r.kind;
    if (owner) *owner = r.owner;
    if (dflt) *dflt = r.dflt;
    if (can_set) *can_set = settable(r) ? 1 : 0;
    return 0;
}

extern "C" int uvcgpu_param_get(const UvcParams *p, const UvcGroupParams *g, int32_t i, double *value) {
    if (i < 0 || i >= N_ROWS || !value) return uvcgpu_set_error(UVCGPU_EINVAL, "parameter row out of range");
    const Row &r = ROWS[i];
    const char *base = (r.owner == UVC_PARAM_OF_PARAMS ? (const char *)p : (const char *)g);
    if (!base) return uvcgpu_set_error(UVCGPU_EINVAL, (std::string(r.name) + ": its struct is NULL").c_str());
    if (r.kind == UVC_PARAM_INT) { int32_t v; memcpy(&v, base + r.off, sizeof(v)); *value = v; }
    else memcpy(value, base + r.off, sizeof(double));
    return 0;
}

extern "C" int uvcgpu_param_set(UvcParams *p, UvcGroupParams *g, const char *name, const char *value) {
    if (!name || !value) return uvcgpu_set_error(UVCGPU_EINVAL, "bad argument");
    const int32_t i = find(name);
    if (i < 0) return uvcgpu_set_error(UVCGPU_EINVAL, (std::string("unknown parameter ") + name).c_str());
    const Row &r = ROWS[i];
    if (!settable(r)) return uvcgpu_set_error(UVCGPU_EINVAL, (std::string(r.name) + " is derived by the library, not set").c_str());
    char *base = (r.owner == UVC_PARAM_OF_PARAMS ? (char *)p : (char *)g);
    if (!base) return uvcgpu_set_error(UVCGPU_EINVAL, (std::string(r.name) + ": its struct is NULL").c_str());
    if (r.kind == UVC_PARAM_INT) {
        int32_t v;
        if (!parse_int(value, &v)) return uvcgpu_set_error(UVCGPU_EINVAL, (std::string(r.name) + ": '" + value + "' is not an int32 (or true / false)").c_str());
        memcpy(base + r.off, &v, sizeof(v));
    } else {
        double v;
        if (!parse_double(value, &v)) return uvcgpu_set_error(UVCGPU_EINVAL, (std::string(r.name) + ": '" + value + "' is not a finite number").c_str());
        memcpy(base + r.off, &v, sizeof(v));
    }
    return 0;
}

extern "C" int uvcgpu_params_check(const UvcParams *params) {
    if (!params) return uvcgpu_set_error(UVCGPU_EINVAL, "bad argument");
    if (params->struct_size != (int32_t)sizeof(UvcParams)) return uvcgpu_set_error(UVCGPU_EINVAL, "UvcParams::struct_size mismatch");
    if (params->indel_str_repeatsize_max < 1 || params->indel_vntr_repeatsize_max < params->indel_str_repeatsize_max) return uvcgpu_set_error(UVCGPU_EINVAL, "bad repeat-size parameters");
    if (params->indel_vntr_repeatsize_max > 255 || params->indel_BQ_max < 1 || params->indel_BQ_max > 32767) return uvcgpu_set_error(UVCGPU_EUNSUPPORTED, "indel_vntr_repeatsize_max > 255 or indel_BQ_max outside 1..32767");
    // dist_to_interfering_indel is 10000 where a read has no low-quality InDel (main.hpp:1897) and a difference of GENOME coordinates next to
    // the sentinels of its InDel list otherwise: a threshold above 10000 compares with those.  The kernels carry the distance in 16 bits with
    // "10000 or more" as one value, which is exact for every threshold up to 10000 (the default is 5) and wrong beyond: refused, not approximated.
    if (params->bias_thres_interfering_indel > 10000) return uvcgpu_set_error(UVCGPU_EUNSUPPORTED, "bias_thres_interfering_indel above 10000");
    // A base's value is its quality plus bq_phred_added_misma (on IonTorrent, next to a short gap, plus the smaller of the two addends): below 0
    // with a negative addend.  The factor tables of k_p2_fast hold the values from -256 on: refused beyond, not approximated.
    if (params->bq_phred_added_misma < -256 || params->bq_phred_added_indel < -256) return uvcgpu_set_error(UVCGPU_EUNSUPPORTED, "bq_phred_added_misma or bq_phred_added_indel below -256");
    // Above, a value stays below 2^12 (255 + 3840): k_p2_fast squares it with a 24-bit multiply and k_frag packs "8 + average value" into 16 signed bits.
    if (params->bq_phred_added_misma > 3840 || params->bq_phred_added_indel > 3840) return uvcgpu_set_error(UVCGPU_EUNSUPPORTED, "bq_phred_added_misma or bq_phred_added_indel above 3840");
    // dealwith_segbias divides by the square of bias_thres_PFBQ1 / 2 for a value below the threshold (main.hpp:1473-1474): with a threshold of 0
    // (the IonTorrent default) and a value below 0 the reference ends in a division by zero, so there is nothing to equal.
    if ((params->bq_phred_added_misma < 0 || params->bq_phred_added_indel < 0) && (params->bias_thres_PFBQ1 == 0 || params->bias_thres_PFBQ2 == 0))
        return uvcgpu_set_error(UVCGPU_EUNSUPPORTED, "a negative bq_phred_added_misma or bq_phred_added_indel with bias_thres_PFBQ1 or bias_thres_PFBQ2 of 0");
    return 0;
}
