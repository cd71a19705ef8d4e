"""The kernel forms of the accumulate and the matrix of tests/test_gpu_kernel_forms.py that reaches them.

uvc_launch_accumulate (uvc_amd/csrc/uvc_kernels_acc.hip) picks one specialisation per pass from the tile's shape, the parameters and the
families' flags, and with UVCGPU_TIMING set names them on one stderr line:

    [uvcgpu accumulate] forms prep=split p2=split,generic frag=h16,split,generic family=digest duplex=digest frag_generic=all

expected_forms() restates the dispatch rules; the GPU module asserts that every cell prints what it computes, and
tests/test_kernel_forms_cpu.py that the union over the matrix covers FORMS."""
import re

from test_gpu_parity import CASES, VARIANTS

# Every form the dispatcher can name, with the kernels of uvc_amd/csrc/uvc_kernels_acc.hip it launches.  frag_generic=sweep is left out: whether the
# sweep list is used depends on the fragments, not on the switches (test_gpu_fuzz.py::test_fragment_longer_than_the_sweep_window covers it).
FORMS = [
    "prep=wave",               # k_prep_fast<false>
    "prep=split",              # k_prep_fast<true>
    "p2=wave,plain",           # k_p2_fast<., ., true>
    "p2=wave,generic",         # k_p2_fast<., ., false>
    "p2=split,plain",          # k_p2_fast_split<., ., true>
    "p2=split,generic",        # k_p2_fast_split<., ., false>
    "frag=h16,split,plain",    # k_frag16_split<true>
    "frag=h16,split,generic",  # k_frag16_split<false>
    "frag=h16,wave,plain",     # k_frag16<true>
    "frag=h16,wave,generic",   # k_frag16<false>
    "frag=b32,wave,plain",     # k_frag<true>
    "frag=b32,wave,generic",   # k_frag<false>
    "family=generic",          # k_fam_p4 / k_fam_p5
    "family=digest",           # k_fam_p4d + k_fam_p4d_rest / k_fam_p5d
    "duplex=generic",          # k_duplex
    "duplex=digest",           # k_duplex_d
    "frag_generic=all",        # k_frag_generic over every fragment (IonTorrent)
    "fastq_only",              # no k_prep_* / k_thres / k_p2_* (prep=none p2=none), k_frag without the P3 arms
]

IONTORRENT = 2   # UVC_PLATFORM_IONTORRENT (include/uvcgpu.h)


def _edited(name):
    kw = dict(CASES[name])
    kw["indel_every"] = 400
    kw["clip_frac"] = 0.05   # as in test_gpu_parity.py::test_parameter_variants
    return kw


# The tiles, and the facts about them that the dispatch reads (checked on the GPU through the forms line):
#   family: the family form set_reads chooses when it is not forced to the generic one ("none": no unit has two fragments or a duplex
#           partner, so no family pass runs -- a single-fragment unit is folded in by k_frag while the singleton thresholds allow it);
#   duplex: the tile has duplex families (fam_dflag 0x2 with both strands);
#   h16:    fewer than 65 536 fragments cover every position;
#   split:  the form UVCGPU_SPLIT unset gives (acc_forms of uvc_kernels_acc.hip), for the cells that do not force it.
TILES = {
    "nodedup_3kb_60x": dict(gen=_edited("nodedup_3kb_60x"), amplicon=False, family="none", duplex=False, h16=True),
    "umi_duplex_2kb_400x": dict(gen=_edited("umi_duplex_2kb_400x"), amplicon=False, family="digest", duplex=True, h16=True),
    # every other family of the first tile flagged amplicon (fam_dflag 0x4): R->any_amplicon, the P2 rules of amplicon reads
    "amplicon_nodedup_3kb_60x": dict(gen=_edited("nodedup_3kb_60x"), amplicon=True, family="none", duplex=False, h16=True),
}
# a 70 000-read pile-up (test_gpu_parity.py::test_more_than_65535_fragments_on_one_position): 32-bit buckets without forcing; 400 positions
# in 7 windows, 70 000 x (60 + 64) / 400 read-window slots per position: the split form
STACK = dict(family="none", duplex=False, h16=False, split=True)

ARMS = {"default": {}}
ARMS.update(VARIANTS)
ARMS["iontorrent_sscs_primer"] = dict(platform=IONTORRENT, set=dict(fam_flag=1, primerlen=12))
# The SSCS table caps P3's consensus quality (main.hpp:2758) only where it is below 8 + the average base quality: with the default table (40 .. 58)
# it changes no plane of these tiles, with this one every tile's VQ planes
ARMS["sscs_table_low_phreds"] = dict(set=dict(fam_flag=1, fam_phred_sscs_transition_CG_TA=20, fam_phred_sscs_transition_AT_GC=22, fam_phred_sscs_transversion_CG_AT=24,
                                              fam_phred_sscs_transversion_other=26, fam_phred_sscs_indel_open=30))


def switches(tile):
    """The forced switches of one (tile, arm): (UVCGPU_FRAG32, UVCGPU_FAM_PATH, [UVCGPU_SPLIT of the two accumulates on one handle])."""
    fam_paths = (None, "generic") if TILES[tile]["family"] != "none" else (None,)
    return [(frag32, fam_path, ("0", "1")) for frag32 in (False, True) for fam_path in fam_paths]


def arm_params(p, arm):
    for k, val in ARMS[arm].get("set", {}).items():
        assert hasattr(p, k), k
        setattr(p, k, val)
    return p


def expected_forms(p, facts, split, frag32=False, fam_generic=False):
    """The forms line uvc_launch_accumulate prints for parameters `p` (a UvcParams) on a tile with `facts`, under the forced switches.
    split: UVCGPU_SPLIT ("0" / "1"), or None for the tile's own choice."""
    vcf = bool(p.inferred_is_vcf_generated)
    proton = (p.inferred_sequencing_platform == IONTORRENT)
    sp = (split != "0") if split is not None else facts.get("split")
    # AccForms::p2_plain: P2 without the IonTorrent / amplicon / primer / short-read arms
    p2_plain = (not proton and not facts.get("amplicon", False) and not (p.primerlen > 0 and not (p.primer_flag & 0x2))
                and p.central_readlen >= p.microadjust_median_readlen_thres)
    # AccForms::frag_plain: P3 without the IonTorrent / SSCS-table / padded-deletion arms (and not on a FASTQ-only run)
    frag_plain = vcf and not proton and not (p.fam_flag & 0x1) and not (p.microadjust_padded_deletion_flag & 0x1)
    h16 = facts["h16"] and not frag32                                                   # AccForms::h16
    fam = facts["family"] if (facts["family"] == "none" or not fam_generic) else "generic"   # the family form set_reads chooses (uvc_host.cpp)
    sh = "split" if sp else "wave"
    return dict(prep=sh if vcf else "none",
                p2=("%s,%s" % (sh, "plain" if p2_plain else "generic")) if vcf else "none",
                frag="%s,%s,%s" % ("h16" if h16 else "b32", "split" if (sp and h16) else "wave", "plain" if frag_plain else "generic"),
                family=fam,
                duplex=fam if (vcf and facts["duplex"]) else "none",
                frag_generic="all" if proton else None)   # None: "sweep" or "none", decided by the fragments


def form_names(forms):
    """The FORMS entries one forms line reaches."""
    out = {"%s=%s" % (k, v) for k, v in forms.items() if v not in (None, "none")}
    if forms["prep"] == "none" and forms["p2"] == "none":
        out.add("fastq_only")
    return out


FORMS_RE = re.compile(r"^\[uvcgpu accumulate\] forms (.*)$", re.M)


def parse_forms(err):
    """Every forms line in captured stderr, as dicts."""
    return [dict(kv.split("=", 1) for kv in m.group(1).split()) for m in FORMS_RE.finditer(err)]


def forms_match(got, want):
    return all((got.get(k) in ("sweep", "none")) if v is None else got.get(k) == v for k, v in want.items()) and set(got) == set(want)
