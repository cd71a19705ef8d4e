"""ctypes mirror of include/uvcgpu.h (struct layouts are generated from include/uvc_params.def).

`Lib` binds any shared library that exports the uvcgpu.h entry points under a prefix: the product library
(uvc_amd/csrc/libuvcgpu.so, prefix `uvcgpu_`) and, in tests / smoke / bench cpu_baseline only, the checker of the
same ABI (whose path lives with it, outside this package -- nothing here knows where it is).
"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_params_def():
    ints, dbls = [], []
    with open(os.path.join(ROOT, "include", "uvc_params.def")) as fh:
        for line in fh:
            m = re.match(r"UVC_P([ID])\((\w+),\s*(.*)\)\s*$", line)
            if not m:
                continue
            (ints if m.group(1) == "I" else dbls).append((m.group(2), eval(m.group(3))))
    return ints, dbls


PARAM_INTS, PARAM_DBLS = _read_params_def()


class UvcParams(C.Structure):
    _fields_ = ([("struct_size", C.c_int32), ("reserved_", C.c_int32)]
                + [(n, C.c_int32) for n, _ in PARAM_INTS] + [("pad_to_8_", C.c_int32)]
                + [(n, C.c_double) for n, _ in PARAM_DBLS])


class UvcReadSoA(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("reserved_", C.c_int32),
        ("n_reads", C.c_int64),
        ("pos", C.c_void_p), ("mpos", C.c_void_p), ("isize", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p),
        ("nm", C.c_void_p), ("l_qseq", C.c_void_p), ("seq_off", C.c_void_p), ("cigar_off", C.c_void_p), ("n_cigar", C.c_void_p),
        ("frag_id", C.c_void_p), ("fam_id", C.c_void_p), ("fam_strand", C.c_void_p),
        ("n_bases", C.c_int64), ("bases", C.c_void_p), ("quals", C.c_void_p),
        ("n_cigar_ops", C.c_int64), ("cigars", C.c_void_p),
        ("n_fams", C.c_int32), ("fam_dflag", C.c_void_p),
        ("bases4", C.c_void_p), ("n_bases4_bytes", C.c_int64),
    ]


class UvcIndelAllele(C.Structure):
    _fields_ = [("refpos", C.c_int32), ("symbol", C.c_int32), ("bDPa", C.c_int32), ("cDP0a", C.c_int32), ("indel_len", C.c_int32)]


class UvcTumorKey(C.Structure):
    _fields_ = [("refpos", C.c_int32), ("symbol", C.c_int32), ("cDP1x", C.c_int32), ("CDP1x", C.c_int32), ("bDP", C.c_int32), ("BDP", C.c_int32),
                ("tier2", C.c_int32), ("indel_len", C.c_int32)]
    _fields_ += [(n, C.c_int32) for n in ("cVQ1", "cPCQ1", "cDP2x", "CDP2x", "cVQ2", "cPCQ2", "bNMQ", "vHGQ", "tDP", "tAD0", "tAD1", "t2DP")]


class UvcGapRow(C.Structure):
    _fields_ = [("refpos", C.c_int32), ("symbol", C.c_int32), ("strand", C.c_int32), ("len", C.c_int32), ("seq_off", C.c_int64),
                ("bAD1", C.c_int32), ("cAD1", C.c_int32), ("c2AD", C.c_int32), ("c2dAD", C.c_int32)]


class UvcHapLink(C.Structure):
    _fields_ = [("which", C.c_int32), ("n_muts", C.c_int32), ("mut_off", C.c_int64), ("fr_cnt", C.c_int32 * 2), ("other_cnt", C.c_int32 * 2)]


class UvcScoreRequest(C.Structure):
    _fields_ = [("pos_beg", C.c_int32), ("pos_end", C.c_int32), ("all_out", C.c_int32), ("is_amplicon", C.c_int32),
                ("n_indel_alleles", C.c_int64), ("indel_alleles", C.c_void_p), ("n_tumor_keys", C.c_int64), ("tumor_keys", C.c_void_p),
                ("release_state", C.c_int32), ("base_at_pos_beg", C.c_int32), ("region_beg", C.c_int32), ("kept_only", C.c_int32),
                ("tumor_sample_columns", C.c_void_p), ("tumor_ref_alt", C.c_void_p), ("n_force_sites", C.c_int64), ("force_sites", C.c_void_p)]


class UvcScoreRange(C.Structure):
    _fields_ = [("pos_beg", C.c_int32), ("pos_end", C.c_int32), ("base_at_pos_beg", C.c_int32), ("region_beg", C.c_int32)]


class UvcCoverageRange(C.Structure):
    _fields_ = [("pos_beg", C.c_int32), ("pos_end", C.c_int32)]


class UvcErrorProfileRequest(C.Structure):
    _fields_ = [("min_depth", C.c_int32), ("max_alt_permille", C.c_int32)]


class UvcReadProfileRequest(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("min_depth", C.c_int32), ("max_alt_permille", C.c_int32)]


class UvcFamilyRange(C.Structure):
    _fields_ = [("pos_beg", C.c_int32), ("pos_end", C.c_int32), ("prev_end", C.c_int32), ("flags", C.c_int32)]


class UvcFragmentProfileRequest(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("short_lo", C.c_int32), ("short_hi", C.c_int32), ("long_lo", C.c_int32), ("long_hi", C.c_int32)]


class UvcCallableRequest(C.Structure):
    _fields_ = [("min_depth", C.c_int32 * 6), ("max_aDP", C.c_int32)]


class UvcSiteReadsRequest(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("alt_only", C.c_int32)]


class UvcSiteRead(C.Structure):
    _fields_ = [("site", C.c_int32), ("read", C.c_int32), ("q", C.c_int32), ("obs", C.c_int32), ("ins_q", C.c_int32), ("ins_len", C.c_int32), ("del_len", C.c_int32), ("reserved", C.c_int32)]


class UvcClipSitesRequest(C.Structure):
    _fields_ = [("min_mapq", C.c_int32), ("min_clip", C.c_int32), ("min_reads", C.c_int32), ("want_reads", C.c_int32)]


class UvcClipRead(C.Structure):
    _fields_ = [("site", C.c_int32), ("read", C.c_int32), ("soft_len", C.c_int32), ("hard_len", C.c_int32)]


class UvcClipJunctionsRequest(C.Structure):
    _fields_ = [("min_votes", C.c_int32), ("min_len", C.c_int32), ("max_mismatch", C.c_int32), ("max_dist", C.c_int32), ("mate_slop", C.c_int32)]


class UvcClipMatesRequest(C.Structure):
    _fields_ = [("tid", C.c_int32), ("min_mapq", C.c_int32), ("window", C.c_int32), ("overhang", C.c_int32), ("min_dist", C.c_int32), ("max_gap", C.c_int32), ("min_pairs", C.c_int32),
                ("want_reads", C.c_int32)]


class UvcClipMate(C.Structure):
    _fields_ = [("site", C.c_int32), ("read", C.c_int32), ("cluster", C.c_int32), ("klass", C.c_int32)]


class UvcCallableRun(C.Structure):
    _fields_ = [("range", C.c_int32), ("pos_beg", C.c_int32), ("pos_end", C.c_int32), ("mask", C.c_int32)]


class UvcMsiRequest(C.Structure):
    _fields_ = [("min_tracklen", C.c_int32), ("min_units", C.c_int32), ("max_unitlen", C.c_int32)]


class UvcScoreOut(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("n_records", C.c_int64), ("fields", C.c_void_p)]


def _parse_enums():
    """Pulls every `NAME = value` / implicit enumerator of include/uvcgpu.h into a dict."""
    txt = open(os.path.join(ROOT, "include", "uvcgpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for body in re.findall(r"enum\s*\w*\s*\{(.*?)\}", txt, flags=re.S):
        val = -1
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            if "=" in item:
                name, v = [t.strip() for t in item.split("=")]
                val = int(eval(v, {}, out))
            else:
                name = item
                val += 1
            out[name] = val
    return out


ENUMS = _parse_enums()
NSYM = ENUMS["UVC_NUM_SYMBOLS"]

# field group -> (id, dtype, planes per position as a shape prefix): the rows of include/uvc_field_groups.def in id order, each
# UVC_GROUP(name, element bytes, fields, strands, per_symbol, fill); an axis of length 1 in front of the symbols is not part of the shape
import numpy as _np


def _read_field_groups():
    groups = {}
    with open(os.path.join(ROOT, "include", "uvc_field_groups.def")) as fh:
        for m in filter(None, (re.match(r"UVC_GROUP\((\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*\w+\)\s*$", line) for line in fh)):
            elem, fields, strands, per_symbol = (int(t) for t in m.groups()[1:])
            shape = ((strands,) if strands > 1 else ()) + ((fields,) if fields > 1 or not per_symbol else ()) + ((NSYM,) if per_symbol else ())
            groups[m.group(1)] = (ENUMS["UVC_F_" + m.group(1)], {4: _np.int32, 8: _np.int64}[elem], shape)
    return groups


FIELD_GROUPS = _read_field_groups()
assert [gid for gid, _, _ in FIELD_GROUPS.values()] == list(range(ENUMS["UVC_NUM_FIELD_GROUPS"]))
SCORE_FIELDS = [k[len("UVC_O_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_O_")), key=lambda kv: kv[1])]
NUM_SCORE_FIELDS = ENUMS["UVC_NUM_SCORE_FIELDS"]
# the depth measures of uvcgpu_region_coverage in id order (UvcCoverageMeasure; the rows of include/uvc_coverage.def)
COVERAGE_MEASURES = [k[len("UVC_COV_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_COV_") and k[len("UVC_COV_"):] not in ("SUM", "MIN", "MAX", "GE", "MAX_THRESHOLDS", "ROW")), key=lambda kv: kv[1])]
assert len(COVERAGE_MEASURES) == ENUMS["UVC_NCOV"]
# the evidence levels of uvcgpu_region_error_profile in id order (UvcErrLevel; the rows of include/uvc_errprofile.def)
ERROR_LEVELS = [k[len("UVC_ERRLEVEL_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_ERRLEVEL_")), key=lambda kv: kv[1])]
assert len(ERROR_LEVELS) == ENUMS["UVC_NERRLEVEL"]


def _read_def(file, macro):
    """The rows `macro(name, first word, words)` of include/<file> as (name, first word, words): the sections of the row of numbers a
    report call fills.  A table of one column, `macro(name)`, gives its names."""
    with open(os.path.join(ROOT, "include", file)) as fh:
        rows = [re.match(macro + r"\((\w+)(?:,\s*(\d+),\s*(\d+))?\)\s*$", line) for line in fh]
    return [m.group(1) if m.group(2) is None else (m.group(1), int(m.group(2)), int(m.group(3))) for m in rows if m]


# the sections of a family-statistics row in id order (UvcFamStat): the table of include/uvc_famstats.def, checked against the header's enums
FAMSTAT_SECTIONS = _read_def("uvc_famstats.def", "UVC_FAMSTAT")
FAMILY_STATS = [n for n, _, _ in FAMSTAT_SECTIONS]
assert [ENUMS["UVC_FAMSTAT_" + n] for n in FAMILY_STATS] == list(range(ENUMS["UVC_NFAMSTAT"]))
assert sum(w for _, _, w in FAMSTAT_SECTIONS) == ENUMS["UVC_FAMSTAT_ROW"] and all(f == sum(w for _, _, w in FAMSTAT_SECTIONS[:k]) for k, (_, f, _) in enumerate(FAMSTAT_SECTIONS))

# the sections of the family-concordance row in id order (UvcFamConc): the table of include/uvc_famconcord.def, checked against the header's enums
FAMCONC_SECTIONS = _read_def("uvc_famconcord.def", "UVC_FAMCONC")
FAMILY_CONCORDANCE = [n for n, _, _ in FAMCONC_SECTIONS]
assert [ENUMS["UVC_FAMCONC_" + n] for n in FAMILY_CONCORDANCE] == list(range(ENUMS["UVC_NFAMCONC"]))
assert sum(w for _, _, w in FAMCONC_SECTIONS) == ENUMS["UVC_FAMCONC_ROW"] and all(f == sum(w for _, _, w in FAMCONC_SECTIONS[:k]) for k, (_, f, _) in enumerate(FAMCONC_SECTIONS))
assert [f for _, f, _ in FAMCONC_SECTIONS] == [ENUMS["UVC_FAMCONC_" + n.upper()] for n in FAMILY_CONCORDANCE] and FAMCONC_SECTIONS[-1][2] == ENUMS["UVC_NFAMCONCC"]
FAMCONC_COUNTERS = [k[len("UVC_FAMCONCC_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_FAMCONCC_")), key=lambda kv: kv[1])]

# the sections of a fragment-profile row in id order (UvcFragProfSection): the table of include/uvc_fragprofile.def, checked against the header's enums
FRAGPROF_SECTIONS = _read_def("uvc_fragprofile.def", "UVC_FRAGPROF")
FRAGMENT_PROFILE = [n for n, _, _ in FRAGPROF_SECTIONS]
assert [ENUMS["UVC_FRAGPROF_" + n] for n in FRAGMENT_PROFILE] == list(range(ENUMS["UVC_NFRAGPROF"]))
assert sum(w for _, _, w in FRAGPROF_SECTIONS) == ENUMS["UVC_FRAGPROF_ROW"] and all(f == sum(w for _, _, w in FRAGPROF_SECTIONS[:k]) for k, (_, f, _) in enumerate(FRAGPROF_SECTIONS))
assert [f for _, f, _ in FRAGPROF_SECTIONS[:ENUMS["UVC_FRAGPROF_TARGET_ROW"]]] == list(range(ENUMS["UVC_FRAGPROF_TARGET_ROW"])), "the first eight sections are the words of a TARGET row"
assert {n: (f, w) for n, f, w in FRAGPROF_SECTIONS}["LEN"] == (ENUMS["UVC_FRAGPROF_LEN_BINS"], ENUMS["UVC_FRAGPROF_NLEN"]) and {n: (f, w) for n, f, w in FRAGPROF_SECTIONS}["FAMLEN"] == (ENUMS["UVC_FRAGPROF_FAMLEN_BINS"], ENUMS["UVC_FRAGPROF_NLEN"])
assert {n: (f, w) for n, f, w in FRAGPROF_SECTIONS}["MOTIF"] == (ENUMS["UVC_FRAGPROF_MOTIF_BINS"], ENUMS["UVC_FRAGPROF_NMOTIF"]) and ENUMS["UVC_FRAGPROF_LEN_BINS"] == ENUMS["UVC_FRAGPROF_NCOUNTER"]

# the sections of a read-profile row in id order (UvcReadProfSection): the table of include/uvc_readprofile.def, checked against the header's enums
READPROF_SECTIONS = _read_def("uvc_readprofile.def", "UVC_READPROF")
assert [ENUMS["UVC_READPROF_" + n] for n, _, _ in READPROF_SECTIONS] == list(range(ENUMS["UVC_NREADPROF"]))
assert sum(w for _, _, w in READPROF_SECTIONS) == ENUMS["UVC_READPROF_ROW"] and all(f == sum(w for _, _, w in READPROF_SECTIONS[:k]) for k, (_, f, _) in enumerate(READPROF_SECTIONS))

# the bits of a callability mask in bit order (UvcCallableBit): the table of include/uvc_callable.def, checked against the header's enums and the measures
CALLABLE_BITS = _read_def("uvc_callable.def", "UVC_CALLBIT")
assert [ENUMS["UVC_CALL_" + n] for n in CALLABLE_BITS] == list(range(ENUMS["UVC_NCALLBIT"]))
assert CALLABLE_BITS[:len(COVERAGE_MEASURES)] == ["LOW_" + m for m in COVERAGE_MEASURES] and C.sizeof(UvcCallableRequest) == 4 * (ENUMS["UVC_NCOV"] + 1)

# the observation kinds of uvcgpu_region_site_reads in id order (uvcgpu_site_read_kind_name), checked against the header's enums
SITE_READ_KINDS = ["A", "C", "G", "T", "N", "DEL"]
assert [ENUMS["UVC_SITEREAD_" + n] for n in SITE_READ_KINDS] == list(range(ENUMS["UVC_SITEREAD_NKIND"])) and C.sizeof(UvcSiteRead) == 4 * ENUMS["UVC_SITEREAD_NCOL"]

# the sections of a clip-site row in id order (UvcClipSiteSection): the table of include/uvc_clipsites.def, checked against the header's enums
CLIPSITE_SECTIONS = _read_def("uvc_clipsites.def", "UVC_CLIPSITE")
assert [ENUMS["UVC_CLIPSITE_" + n] for n, _, _ in CLIPSITE_SECTIONS] == list(range(ENUMS["UVC_NCLIPSITE"]))
assert sum(w for _, _, w in CLIPSITE_SECTIONS) == ENUMS["UVC_CLIPSITE_ROW"] and all(f == sum(w for _, _, w in CLIPSITE_SECTIONS[:k]) for k, (_, f, _) in enumerate(CLIPSITE_SECTIONS))
assert CLIPSITE_SECTIONS[-1] == ("VOTE", ENUMS["UVC_CLIPSITE_VOTE_BINS"], ENUMS["UVC_CLIPSITE_NCONS"] * ENUMS["UVC_CLIPSITE_NCODE"]) and C.sizeof(UvcClipRead) == 16 and C.sizeof(UvcClipSitesRequest) == 16
CLIPSITE_TOTALS = [k[len("UVC_CLIPTOTAL_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_CLIPTOTAL_")), key=lambda kv: kv[1])]

# the sections of a clip-junction row in id order (UvcClipJuncSection): the table of include/uvc_clipjunc.def, checked against the header's enums
CLIPJUNC_SECTIONS = _read_def("uvc_clipjunc.def", "UVC_CLIPJUNC")
assert [ENUMS["UVC_CLIPJUNC_" + n] for n, _, _ in CLIPJUNC_SECTIONS] == list(range(ENUMS["UVC_NCLIPJUNC"]))
assert sum(w for _, _, w in CLIPJUNC_SECTIONS) == ENUMS["UVC_CLIPJUNC_ROW"] and all(f == sum(w for _, _, w in CLIPJUNC_SECTIONS[:k]) for k, (_, f, _) in enumerate(CLIPJUNC_SECTIONS))
assert dict((n, w) for n, _, w in CLIPJUNC_SECTIONS)["hist"] == ENUMS["UVC_CLIPJUNC_NHIST"] and C.sizeof(UvcClipJunctionsRequest) == 20
CLIPJUNC_TOTALS = [k[len("UVC_CLIPJTOTAL_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_CLIPJTOTAL_")), key=lambda kv: kv[1])]
CLIP_CLASSES = [k[len("UVC_CLIPCLASS_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_CLIPCLASS_")), key=lambda kv: kv[1])]
assert len(CLIP_CLASSES) == ENUMS["UVC_NCLIPCLASS"]

# the words of the two rows of uvcgpu_region_clip_mates in id order (UvcClipMateSiteWord, UvcClipMateClusterWord): the two tables of
# include/uvc_clipmates.def, checked against the header's enums
CLIPMATE_SITE_WORDS = _read_def("uvc_clipmates.def", "UVC_CLIPMATE_SITE")
CLIPMATE_CLUSTER_WORDS = _read_def("uvc_clipmates.def", "UVC_CLIPMATE_CLUSTER")
assert [ENUMS["UVC_CLIPMSITE_" + n] for n, _, _ in CLIPMATE_SITE_WORDS] == list(range(ENUMS["UVC_NCLIPMSITE"])) and [ENUMS["UVC_CLIPMCLUS_" + n] for n, _, _ in CLIPMATE_CLUSTER_WORDS] == list(range(ENUMS["UVC_NCLIPMCLUS"]))
assert [(f, w) for _, f, w in CLIPMATE_SITE_WORDS] == [(k, 1) for k in range(ENUMS["UVC_CLIPMATE_SITE_ROW"])] and [(f, w) for _, f, w in CLIPMATE_CLUSTER_WORDS] == [(k, 1) for k in range(ENUMS["UVC_CLIPMATE_ROW"])]
assert C.sizeof(UvcClipMatesRequest) == 32 and C.sizeof(UvcClipMate) == 16
CLIPMATE_TOTALS = [k[len("UVC_CLIPMTOTAL_"):] for k, v in sorted(((k, v) for k, v in ENUMS.items() if k.startswith("UVC_CLIPMTOTAL_")), key=lambda kv: kv[1])]
CLIPMATE_CLASSES = ["CONCORDANT", "OTHER_CONTIG", "SAME_STRAND", "FAR"]
assert [ENUMS["UVC_CLIPMATE_" + n] for n in CLIPMATE_CLASSES] == list(range(ENUMS["UVC_NCLIPMATECLASS"]))

# the sections of a microsatellite row in id order (UvcMsiSection): the table of include/uvc_msi.def, checked against the header's enums
MSI_SECTIONS = _read_def("uvc_msi.def", "UVC_MSI")
assert [ENUMS["UVC_MSI_" + n] for n, _, _ in MSI_SECTIONS] == list(range(ENUMS["UVC_NMSI"]))
assert sum(w for _, _, w in MSI_SECTIONS) == ENUMS["UVC_MSI_ROW"] and all(f == sum(w for _, _, w in MSI_SECTIONS[:k]) for k, (_, f, _) in enumerate(MSI_SECTIONS))
assert dict((n, (f, w)) for n, f, w in MSI_SECTIONS)["depth"] == (ENUMS["UVC_MSI_DEPTH"], ENUMS["UVC_MSI_NLEVEL"]) and dict((n, (f, w)) for n, f, w in MSI_SECTIONS)["hist"] == (ENUMS["UVC_MSI_HIST"], ENUMS["UVC_MSI_NLEVEL"] * ENUMS["UVC_MSI_NBIN"])


class Lib:
    """Binds one shared library exporting the uvcgpu.h entry points under `prefix`."""

    def __init__(self, path, prefix):
        self.path, self.prefix = path, prefix
        self.dll = C.CDLL(path)
        f = self._f
        f("params_default", None, [C.POINTER(UvcParams)])
        f("last_error", C.c_char_p, [])
        create = "region_create" if prefix == "uvcgpu_" else "create"
        self.n = dict(create=create,
                      set_reads="region_set_reads" if prefix == "uvcgpu_" else "set_reads",
                      accumulate="region_accumulate" if prefix == "uvcgpu_" else "accumulate",
                      field_bytes="region_field_bytes" if prefix == "uvcgpu_" else "field_bytes",
                      fetch="region_fetch" if prefix == "uvcgpu_" else "fetch",
                      score="region_score" if prefix == "uvcgpu_" else "score",
                      destroy="region_destroy" if prefix == "uvcgpu_" else "destroy")
        f(self.n["create"], C.c_int, [C.POINTER(C.c_void_p), C.POINTER(UvcParams), C.c_int32, C.c_int32, C.c_int32, C.c_char_p])
        f(self.n["set_reads"], C.c_int, [C.c_void_p, C.POINTER(UvcReadSoA)])
        f(self.n["accumulate"], C.c_int, [C.c_void_p])
        f(self.n["field_bytes"], C.c_int64, [C.c_void_p, C.c_int32])
        f(self.n["fetch"], C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64])
        f(self.n["score"], C.c_int, [C.c_void_p, C.POINTER(UvcScoreRequest), C.POINTER(UvcScoreOut)])
        f(self.n["destroy"], None, [C.c_void_p])

    def _f(self, name, restype, argtypes):
        fn = getattr(self.dll, self.prefix + name)
        fn.restype, fn.argtypes = restype, argtypes
        return fn

    def call(self, key, *args):
        return getattr(self.dll, self.prefix + self.n.get(key, key))(*args)

    def last_error(self):
        e = getattr(self.dll, self.prefix + "last_error")()
        return e.decode() if e else ""


def gpu_library_path():
    # UVCGPU_LIBRARY: another build of the same ABI (A/B measurements of a kernel variant on one GPU box: scripts/gpu_ab_*.sh)
    return os.environ.get("UVCGPU_LIBRARY") or os.path.join(ROOT, "uvc_amd", "csrc", "libuvcgpu.so")
