"""The parameter ledger: one or more non-default values for every hot-path parameter, with the input each runs on and the outputs it changes.

Every UvcParams row of include/uvc_params.def and every UvcGroupParams field (include/uvc_group_params.def plus the fields uvcgroup.h
declares by hand) is either in MOVES or in EXEMPT.  tests/test_param_moves_cpu.py checks that the ledger is complete and that every move
changes the oracle's outputs it names; tests/test_gpu_param_moves.py runs every move on the oracle and on the HIP path and compares them.

A move is Move(value, input, outputs, companions): `value` replaces the parameter's default (UvcGroupParams fields are keyed "group.<name>"),
`input` names an entry of INPUTS, `companions` are further settings the move needs to reach its branch, and `outputs` is a subset of OUTPUTS:
    planes    every integer plane group of tests/util.py (INT_GROUPS)
    gate      the records of the input's own score request (default gate)
    records   the records of the same request with all_out
    alleles   the InDel allele rows (Region.indel_alleles)
    hap       the haplotype links (Region.hap_links)
    vcf       the record lines of the default-gate request
    families  the family assignment (uvc_amd.group.group_families)"""
import ctypes as C
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from uvc_amd import _ffi, group, region, synth
from util import INT_GROUPS

OUTPUTS = ("planes", "gate", "records", "alleles", "hap", "vcf", "families")

Move = namedtuple("Move", "value input outputs companions")


def M(value, input, outputs, **companions):
    return Move(value, input, tuple(outputs.split()), companions)


# ---- inputs ----
_PLAIN = dict(region_len=3000, depth=60, seed=3, dedup_by_position=False, indel_every=400, clip_frac=0.05, snv_every=90, somatic_every=400)

# gen: synth.generate_region keywords; platform: 1 Illumina, 2 IonTorrent; amplicon: every other family flagged amplicon (fam_dflag 0x4) and the
# score request's is_amplicon set; tumor: the normal sample of a T/N pair (tumor_vcf_is_provided, keys from the default records);
# correct_bq: Region.correct_bq before the accumulate; alignments: tests/test_group.py::make_alignments keywords (family assignment only)
INPUTS = {
    "plain": dict(gen=_PLAIN),                                                           # non-UMI, InDels, clips, dense SNVs (hap links)
    "duplex": dict(gen=dict(region_len=2000, depth=400, seed=11, umi=True, indel_every=400, clip_frac=0.05)),
    "iontorrent": dict(gen=_PLAIN, platform=2),
    "amplicon": dict(gen=dict(_PLAIN, depth=120), amplicon=True),
    "normal": dict(gen=_PLAIN, tumor=True),
    "bqfix": dict(gen=dict(_PLAIN, clip_frac=0.3), correct_bq=True),
    "lowmq": dict(gen=_PLAIN, mapq=25),                                                 # every read at MAPQ 25
    "weird": dict(fuzz=dict(seed=0)),                                                  # tests/test_gpu_fuzz.py: multi-allelic InDels, long clips, every MQ
    "fam_umi": dict(alignments=dict(seed=41, umi=True, n_pairs=300)),
    "fam_amplicon": dict(alignments=dict(seed=42, amplicon=True, n_pairs=1400)),
    "fam_amplicon_umi": dict(alignments=dict(seed=43, amplicon=True, umi=True, n_pairs=1400)),
}

_reads_cache = {}


def reads_of(name):
    """The reads (or, for a family-assignment input, (columns, fetch_tbeg, fetch_tend)) of one input, made once."""
    if name not in _reads_cache:
        inp = INPUTS[name]
        if "alignments" in inp:
            from test_group import make_alignments
            cols, _qnames, tb, te = make_alignments(**inp["alignments"])
            _reads_cache[name] = (cols, tb, te)
        elif "fuzz" in inp:
            from test_gpu_fuzz import weird_region
            _reads_cache[name] = weird_region(**inp["fuzz"])
        else:
            reads = synth.generate_region(**inp["gen"])
            if "mapq" in inp:
                reads = dict(reads, mapq=np.full(reads["n_reads"], inp["mapq"], np.uint8))
            if inp.get("amplicon"):
                reads = dict(reads, fam_dflag=(reads["fam_dflag"] | np.where(np.arange(reads["n_fams"]) % 2 == 0, 4, 0)).astype(np.uint8))
            _reads_cache[name] = reads
    return _reads_cache[name]


_keys_cache = {}


def tumor_keys(oracle_lib, name):
    """The tumor keys of a T/N input: made from the oracle's tumor-only records of the same reads at defaults (as test_gpu_parity.py does)."""
    if name not in _keys_cache:
        from test_gpu_parity import tumor_keys_from
        R = region.Region(oracle_lib, region.default_params(oracle_lib, platform=INPUTS[name].get("platform", 1)), *_region_args(reads_of(name)))
        R.set_reads(reads_of(name))
        R.accumulate()
        _keys_cache[name] = tumor_keys_from(R.score(all_out=False))
        R.close()
    return _keys_cache[name]


def _region_args(reads):
    return reads["tid"], reads["beg"], reads["end"], reads["refseq"]


def is_group(param):
    return param.startswith("group.")


def settings(param, move):
    """{field: value} of one move: the companions, then the value."""
    s = dict(move.companions)
    s[param[len("group."):] if is_group(param) else param] = move.value
    return s


def score_kw(oracle_lib, name):
    inp = INPUTS[name]
    kw = {}
    if inp.get("amplicon"):
        kw["is_amplicon"] = True
    if inp.get("tumor"):
        kw["tumor_keys"] = tumor_keys(oracle_lib, name)
    return kw


def make_params(lib, name, setting):
    inp = INPUTS[name]
    if "alignments" in inp:
        _cols, tb, te = reads_of(name)
        p = group.default_params(lib, tb, te)
    else:
        p = region.default_params(lib, platform=inp.get("platform", 1))
        if inp.get("tumor"):
            p.tumor_vcf_is_provided = 1
    for k, v in setting.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _zip(arrays):
    return {k: (zlib.compress(a.tobytes(), 1), a.dtype, a.shape) for k, a in arrays.items()}


def _unzip(packed):
    return {k: np.frombuffer(zlib.decompress(z), dtype=dt).reshape(shape) for k, (z, dt, shape) in packed.items()}


class Outputs:
    """What one run of an input produced, detached from the handle (which is closed).  fetch(group) makes it usable with util.diff_groups.
    pack() / unpack() hold the planes and records compressed (a few hundred runs wait for the GPU side at once)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def fetch(self, g):
        return self.planes[g]

    def pack(self):
        if hasattr(self, "planes"):
            self.planes, self.gate, self.records = _zip(self.planes), _zip(self.gate), _zip(self.records)
        return self

    def unpack(self):
        if hasattr(self, "planes"):
            self.planes, self.gate, self.records = _unzip(self.planes), _unzip(self.gate), _unzip(self.records)
        return self


def oracle_vcf_text(R, **kw):
    """The record lines the oracle writes (uvc_oracle_region_vcf), unformatted: one string per line, the sample column as the oracle's
    spec.  Enough to see whether a move changes the lines; tests/test_vcf_text.py::_oracle_lines turns it into the reference's text."""
    fn = R.lib.dll.uvc_oracle_region_vcf
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(_ffi.UvcScoreRequest), C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    req, _keep = region.Region.make_request(**kw)
    ln = C.c_int64(0)
    fn(R.h, C.byref(req), b"chrP", None, 0, C.byref(ln))
    buf = C.create_string_buffer(max(1, ln.value))
    assert fn(R.h, C.byref(req), b"chrP", buf, ln.value, C.byref(ln)) == 0, R.lib.last_error()
    text = buf.raw[:ln.value].decode()
    return text.split("\x1d") if text else []


def run(lib, oracle_lib, name, setting, vcf=None):
    """One run of input `name` with the parameters `setting` on `lib` -> Outputs.  `vcf(R, gate_records, score_kw)` makes the record lines
    (default: the oracle's unformatted lines, for the oracle only).  Family-assignment inputs give Outputs(families=...)."""
    inp = INPUTS[name]
    p = make_params(lib, name, setting)
    if "alignments" in inp:
        return Outputs(families=group.group_families(lib, p, reads_of(name)[0]))
    reads = reads_of(name)
    kw = score_kw(oracle_lib, name)
    R = region.Region(lib, p, *_region_args(reads))
    try:
        R.set_reads(reads)
        if inp.get("correct_bq"):
            R.correct_bq()
        R.accumulate()
        planes = {g: R.fetch(g) for g in INT_GROUPS}
        gate = R.score(**kw)
        lines = vcf(R, gate, kw) if vcf is not None else oracle_vcf_text(R, **kw)
        records = R.score(all_out=True, **kw)
        return Outputs(planes=planes, gate=gate, records=records, alleles=R.indel_alleles(), hap=R.hap_links(), vcf=lines)
    finally:
        R.close()


def _same_records(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def changed(a, b):
    """The outputs (of OUTPUTS) in which two runs of the same input differ."""
    if hasattr(a, "families"):
        fa, fb = a.families, b.families
        from test_group import canon
        same = all(np.array_equal(fa[k], fb[k]) for k in ("filter_reason", "isize_norm")) and canon(fa) == canon(fb) and \
            all(fa[k] == fb[k] for k in ("n_kept", "n_fams", "n_frags", "ext_beg", "ext_end", "n_amplicon", "n_visited_qnames"))
        return set() if same else {"families"}
    out = set()
    if any(not np.array_equal(a.planes[g], b.planes[g]) for g in INT_GROUPS):
        out.add("planes")
    if not _same_records(a.gate, b.gate):
        out.add("gate")
    if not _same_records(a.records, b.records):
        out.add("records")
    for k in ("alleles", "hap", "vcf"):
        if getattr(a, k) != getattr(b, k):
            out.add(k)
    return out


# ---- the parameter names ----
ROOT = _ffi.ROOT


def def_names():
    """(UvcParams names with their types and defaults, UvcGroupParams names with theirs) read from the .def files and from the hand-declared
    fields of UvcGroupParams in uvcgroup.h; the defaults are the libraries' own (uvcgpu_params_default / uvcgpu_group_params_default)."""
    params = {}
    with open(os.path.join(ROOT, "include", "uvc_params.def")) as fh:
        for line in fh:
            m = re.match(r"\s*UVC_P([ID])\(\s*(\w+)\s*,", line)
            if m:
                assert m.group(2) not in params, m.group(2)
                params[m.group(2)] = int if m.group(1) == "I" else float
    groups = {}
    with open(os.path.join(ROOT, "include", "uvc_group_params.def")) as fh:
        for line in fh:
            m = re.match(r"\s*UVC_G([ID])\(\s*(\w+)\s*,", line)
            if m:
                groups["group." + m.group(2)] = int if m.group(1) == "I" else float
    with open(os.path.join(ROOT, "include", "uvcgroup.h")) as fh:
        body = fh.read()
    body = body[body.index("typedef struct UvcGroupParams {"):]
    body = body[:body.index("} UvcGroupParams;")]
    for decl in re.findall(r"^\s*int32_t ([^;]*);", body, flags=re.M):
        for n in decl.split(","):
            n = n.strip()
            if n not in ("struct_size", "pad_"):
                groups["group." + n] = int
    return params, groups


def default_of(lib, param):
    if is_group(param):
        return getattr(group.default_params(lib, 100_000, 103_000), param[len("group."):])
    p = _ffi.UvcParams()
    lib.call("params_default", C.byref(p))
    return getattr(p, param)


# ---- the ledger ----
# Moves that change what an input is (a T/N normal pass without tumor keys scores nothing, a FASTQ-only run no InDel): kept out of the
# combined vectors, which move many parameters of one input at once
MODE_SWITCHES = {"tumor_vcf_is_provided", "inferred_is_vcf_generated"}


def combined_vectors(inputs, n_vectors, per_vector, seed0, only=None):
    """Seeded vectors of ledger moves applied together: [(input, {field: value})], vector i on inputs[i % len(inputs)], about `per_vector`
    UvcParams moves of that input each (their companions first, so that a companion never overrides a move).  only: a set of names."""
    out = []
    for i in range(n_vectors):
        inp = inputs[i % len(inputs)]
        cand = sorted((name, k) for name, moves in MOVES.items() if name not in MODE_SWITCHES and (only is None or name in only)
                      for k, m in enumerate(moves) if m.input == inp)
        rng = np.random.default_rng(seed0 + i)
        pick = [cand[j] for j in sorted(rng.choice(len(cand), size=min(per_vector, len(cand)), replace=False))]
        setting = {}
        for name, k in pick:
            for c, v in MOVES[name][k].companions.items():
                setting.setdefault(c, v)
        for name, k in pick:
            setting[name] = MOVES[name][k].value
        out.append((inp, setting))
    return out


# Parameters no move here reaches, each with the code that stands in the way.  Fewer than ten.
EXEMPT = {
    "group.molecule_tag": "read by uvcgpu_qname_digest* as an argument, never by uvcgpu_group_families (the UMI kinds come in with the input); "
                          "test_group.py::test_hashes_and_digest moves it",
    "group.disable_duplex": "as group.molecule_tag: an argument of uvcgpu_qname_digest*, not read by uvcgpu_group_families",
    "indel_vntr_repeatsize_max": "changes only anyTR_* of repeats with a unit above indel_str_repeatsize_max (refstring2repeatvec, "
                                 "oracle_accumulate.cpp:135-150); the synthetic and fuzzed references have no such tandem repeat",
    "indel_multiallele_diffpos_penal": "penal2 = value * log(nearInDelDP / max(aDP, nearInDelDP)) is <= 0 for a value >= 0 and enters only "
                                       "max(penal1, penal2) with penal1 >= 0 (oracle_score.cpp:614-619); negative values changed nothing either",
    "microadjust_germline_mix_with_del_snv_penalty": "needs an SNV inside a track of >= 8 units with three times its depth in deletions "
                                                     "(oracle_score.cpp:664-668), which no input here has",
}

# One or more moves per parameter (see the module text).  The values are the first of a fixed list of candidates (2v + 3 / 1.7v + 0.3, then
# 0, v / 2, v +- 1, 4v + 1, ...) that changed the oracle's outputs on the input, with the companions that open the parameter's branch.
MOVES = {
    "should_output_all": [M(3, "plain", "gate vcf"), M(3, "duplex", "gate vcf")],
    "fam_thres_highBQ_snv": [M(53, "plain", "gate hap planes records vcf"), M(53, "duplex", "gate planes records vcf")],
    "fam_thres_highBQ_indel": [M(29, "plain", "gate records vcf"), M(29, "duplex", "gate records vcf")],
    "fam_thres_dup1add": [M(7, "duplex", "alleles gate planes records vcf")],
    "fam_thres_dup1perc": [M(163, "duplex", "alleles gate planes records vcf")],
    "fam_thres_dup2add": [M(9, "duplex", "gate planes records vcf")],
    "fam_thres_dup2perc": [M(143, "duplex", "gate planes records vcf")],
    "fam_thres_qseqlen": [M(153, "duplex", "gate planes records vcf")],
    "min_altdp_thres": [M(7, "plain", "gate vcf"), M(7, "duplex", "gate")],
    "inferred_sequencing_platform": [M(5, "iontorrent", "gate planes records vcf")],
    "inferred_maxMQ": [M(61, "lowmq", "gate records vcf")],
    "primerlen": [M(3, "plain", "gate hap planes records vcf"), M(3, "duplex", "gate planes records vcf")],
    "primerlen2": [M(49, "amplicon", "gate planes records vcf")],
    "primer_flag": [M(2, "plain", "alleles gate hap planes records vcf", primerlen=12, tn_is_paired=1), M(2, "duplex", "alleles gate planes records vcf", primerlen=12, tn_is_paired=1)],
    "central_readlen": [M(75, "plain", "gate planes records vcf", microadjust_BAQ_per_base_x1024=4096), M(75, "duplex", "gate planes records vcf", microadjust_BAQ_per_base_x1024=4096)],
    "bq_phred_added_misma": [M(3, "plain", "gate hap planes records vcf"), M(3, "duplex", "gate planes records vcf")],
    "bq_phred_added_indel": [M(3, "plain", "gate planes records vcf"), M(3, "duplex", "gate planes records vcf")],
    "powlaw_exponent": [M(5.4, "plain", "gate records vcf"), M(5.4, "duplex", "gate records vcf")],
    "powlaw_anyvar_base": [M(153.3, "plain", "gate records vcf"), M(153.3, "duplex", "gate records vcf")],
    "powlaw_amplicon_allele_fraction_coef": [M(0.0, "duplex", "gate records vcf", primerlen=12)],
    "penal4lowdep": [M(77, "plain", "gate records vcf"), M(77, "normal", "gate records")],
    "assay_sequencing_BQ_max": [M(0, "bqfix", "gate hap planes records vcf")],
    "assay_sequencing_BQ_inc": [M(3, "bqfix", "gate hap planes records vcf")],
    "bias_thres_highBQ": [M(43, "plain", "gate hap planes records vcf"), M(43, "duplex", "gate planes records vcf")],
    "bias_thres_highBAQ": [M(43, "plain", "gate planes records vcf"), M(43, "duplex", "gate planes records vcf")],
    "bias_thres_aLPxT_add": [M(13, "plain", "gate planes records vcf"), M(13, "duplex", "gate planes records vcf")],
    "bias_thres_aLRP1t_minus": [M(23, "plain", "gate planes records vcf"), M(23, "duplex", "gate planes records vcf")],
    "bias_thres_aLRP2t_minus": [M(13, "plain", "gate planes records vcf"), M(13, "duplex", "gate planes records vcf")],
    "bias_thres_aLRB1t_minus": [M(103, "plain", "planes vcf"), M(103, "duplex", "planes vcf")],
    "bias_thres_aLRB2t_minus": [M(53, "plain", "planes vcf"), M(53, "duplex", "planes vcf")],
    "bias_thres_aLRP1t_avgmul_perc": [M(203, "plain", "gate planes records vcf"), M(203, "duplex", "gate planes records vcf")],
    "bias_thres_aLRP2t_avgmul_perc": [M(203, "plain", "gate planes records vcf"), M(203, "duplex", "gate planes records vcf")],
    "bias_thres_aLRB1t_avgmul_perc": [M(203, "plain", "planes vcf"), M(203, "duplex", "planes vcf")],
    "bias_thres_aLRB2t_avgmul_perc": [M(203, "plain", "planes vcf"), M(203, "duplex", "planes vcf")],
    "bias_thres_aLRP1Nt_avgmul_perc": [M(163, "normal", "gate planes records vcf")],
    "bias_thres_aLRB1Nt_avgmul_perc": [M(163, "normal", "planes vcf")],
    "bias_thres_aLRI1T_perc": [M(403, "plain", "planes vcf"), M(403, "duplex", "planes vcf")],
    "bias_thres_aLRI2T_perc": [M(303, "plain", "planes vcf"), M(303, "duplex", "planes vcf")],
    "bias_thres_aLRI1t_perc": [M(103, "plain", "gate planes records vcf"), M(103, "duplex", "gate planes records vcf")],
    "bias_thres_aLRI2t_perc": [M(137, "plain", "gate planes records vcf"), M(137, "duplex", "gate planes records vcf")],
    "bias_thres_aLRI1NT_perc": [M(503, "normal", "planes vcf")],
    "bias_thres_aLRI1Nt_perc": [M(83, "normal", "gate planes records vcf")],
    "bias_thres_aLRI1T_add": [M(363, "plain", "planes vcf"), M(363, "duplex", "planes vcf")],
    "bias_thres_aLRI2T_add": [M(303, "plain", "planes vcf"), M(303, "duplex", "planes vcf")],
    "bias_thres_PFBQ1": [M(53, "plain", "gate planes records vcf"), M(53, "duplex", "gate planes records vcf")],
    "bias_thres_PFBQ2": [M(63, "plain", "gate planes records vcf"), M(63, "duplex", "gate planes records vcf")],
    "bias_thres_interfering_indel": [M(13, "plain", "planes records vcf"), M(13, "duplex", "gate planes records vcf")],
    "bias_thres_interfering_indel_BQ": [M(45, "plain", "gate planes records vcf"), M(45, "duplex", "gate planes records")],
    "bias_thres_BAQ1": [M(49, "plain", "gate planes records vcf"), M(49, "duplex", "gate planes records vcf")],
    "bias_thres_BAQ2": [M(69, "plain", "gate planes records vcf"), M(69, "duplex", "gate planes records vcf")],
    "bias_thres_strict_c2LRP0": [M(13, "duplex", "gate planes records vcf")],
    "bias_thres_FTS_FA": [M(1.32, "plain", "gate records vcf"), M(1.32, "duplex", "gate records vcf")],
    "bias_is_orientation_artifact_mixed_with_sequencing_error": [M(3, "plain", "gate records vcf"), M(3, "duplex", "gate records vcf")],
    "bias_orientation_min_effective_allelefrac": [M(0.3068, "plain", "records"), M(0.3068, "duplex", "gate records")],
    "bias_prior_DPadd_perc": [M(103, "plain", "gate records vcf"), M(103, "duplex", "gate records vcf")],
    "bias_priorfreq_pos": [M(68.3, "plain", "gate records vcf"), M(68.3, "duplex", "gate records vcf")],
    "bias_priorfreq_indel_in_read_div": [M(34.3, "plain", "gate records vcf"), M(34.3, "duplex", "gate records vcf")],
    "bias_priorfreq_indel_in_var_div2": [M(25.8, "plain", "gate records vcf"), M(25.8, "duplex", "gate records")],
    "bias_priorfreq_indel_in_str_div2": [M(17.3, "plain", "gate records vcf"), M(17.3, "duplex", "gate records")],
    "bias_priorfreq_var_in_str_div2": [M(8.8, "plain", "gate records vcf"), M(8.8, "duplex", "gate records")],
    "bias_prior_var_DP_mul": [M(2.425, "plain", "gate records vcf"), M(2.425, "duplex", "gate records vcf")],
    "bias_priorfreq_ipos_snv": [M(0, "duplex", "gate records"), M(0, "amplicon", "gate records vcf")],
    "bias_priorfreq_ipos_indel": [M(460, "duplex", "gate records")],
    "bias_priorfreq_strand_snv_base": [M(23, "duplex", "gate records vcf")],
    "bias_priorfreq_strand_indel": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "bias_FA_pseudocount_indel_in_read": [M(0.385, "plain", "gate records vcf"), M(0.385, "duplex", "gate records vcf")],
    "bias_priorfreq_orientation_snv_base": [M(76.8, "plain", "records"), M(76.8, "duplex", "gate records")],
    "bias_priorfreq_orientation_indel_base": [M(76.8, "plain", "records"), M(76.8, "duplex", "records")],
    "bias_FA_powerlaw_noUMI_phred_inc_snv": [M(13, "plain", "gate records vcf"), M(13, "duplex", "gate records vcf")],
    "bias_FA_powerlaw_noUMI_phred_inc_indel": [M(17, "plain", "gate records vcf"), M(17, "duplex", "gate records vcf")],
    "bias_FA_powerlaw_withUMI_phred_inc_snv": [M(19, "duplex", "gate records vcf")],
    "bias_FA_powerlaw_withUMI_phred_inc_indel": [M(17, "plain", "gate records vcf"), M(17, "duplex", "gate records vcf")],
    "bias_reduction_by_high_sequencingDP_min_n_totDepth": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "bias_reduction_by_high_sequencingDP_min_n_altDepth": [M(0, "plain", "records", bias_reduction_by_high_sequencingDP_min_n_totDepth=0), M(0, "duplex", "gate records", bias_reduction_by_high_sequencingDP_min_n_totDepth=0)],
    "nobias_flag": [M(7, "plain", "gate records vcf"), M(7, "duplex", "gate records vcf")],
    "nobias_pos_indel_lenfrac_thres": [M(3.7, "plain", "records"), M(3.7, "duplex", "records")],
    "nobias_pos_indel_str_track_len": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "fam_thres_emperr_all_flat_snv": [M(11, "duplex", "gate planes records vcf")],
    "fam_thres_emperr_con_perc_snv": [M(137, "duplex", "gate planes records vcf")],
    "fam_thres_emperr_all_flat_indel": [M(11, "duplex", "gate planes records vcf")],
    "fam_thres_emperr_con_perc_indel": [M(137, "duplex", "gate planes records vcf")],
    "fam_min_n_copies": [M(0, "duplex", "gate records vcf")],
    "fam_min_n_copies_DPxAD": [M(0, "duplex", "gate records vcf")],
    "fam_min_overseq_perc": [M(0, "amplicon", "gate records")],
    "fam_bias_overseq_perc": [M(0, "duplex", "gate records vcf")],
    "fam_tier3DP_bias_overseq_perc": [M(703, "duplex", "gate records vcf")],
    "fam_indel_nonUMI_phred_dec_per_fold_overseq": [M(21, "duplex", "gate records vcf")],
    "fam_phred_indel_inc_before_barcode_labeling": [M(31, "duplex", "planes records")],
    "fam_phred_sscs_transition_CG_TA": [M(83, "plain", "gate records vcf"), M(83, "duplex", "gate records vcf")],
    "fam_phred_sscs_transition_AT_GC": [M(91, "plain", "gate records vcf"), M(91, "duplex", "gate records vcf")],
    "fam_phred_sscs_transversion_CG_AT": [M(99, "plain", "gate records vcf"), M(99, "duplex", "gate planes records vcf")],
    "fam_phred_sscs_transversion_other": [M(99, "plain", "gate records vcf"), M(99, "duplex", "gate planes records vcf")],
    "fam_phred_sscs_indel_open": [M(119, "plain", "gate records vcf"), M(119, "duplex", "gate records vcf")],
    "fam_phred_sscs_indel_ext": [M(3, "plain", "gate records vcf"), M(3, "duplex", "gate records vcf")],
    "fam_phred_dscs_all": [M(119, "duplex", "gate records vcf")],
    "fam_phred_dscs_max": [M(139, "duplex", "records")],
    "fam_phred_dscs_inc_max": [M(43, "duplex", "gate records vcf")],
    "fam_phred_pow_sscs_transversion_AT_TA_origin": [M(29, "plain", "gate records vcf"), M(29, "duplex", "gate records")],
    "fam_phred_pow_sscs_snv_origin": [M(15.6, "plain", "gate records vcf"), M(15.6, "duplex", "gate records vcf")],
    "fam_phred_pow_sscs_indel_origin": [M(53.0, "plain", "gate records vcf"), M(53.0, "duplex", "gate records vcf")],
    "fam_phred_pow_dscs_all_origin": [M(10000.0, "plain", "gate records vcf"), M(100.0, "duplex", "gate records vcf")],
    "fam_flag": [M(3, "iontorrent", "planes records")],
    "syserr_BQ_prior": [M(63, "plain", "gate records vcf"), M(63, "duplex", "gate records vcf")],
    "syserr_BQ_sbratio_q_add": [M(13, "plain", "gate records vcf"), M(13, "duplex", "gate records vcf")],
    "syserr_BQ_sbratio_q_max": [M(83, "plain", "records"), M(83, "duplex", "gate records")],
    "syserr_BQ_xmratio_q_add": [M(13, "plain", "records"), M(13, "amplicon", "records")],
    "syserr_BQ_xmratio_q_max": [M(83, "plain", "gate records vcf"), M(83, "duplex", "gate records vcf")],
    "syserr_BQ_bmratio_q_add": [M(13, "amplicon", "records")],
    "syserr_BQ_bmratio_q_max": [M(83, "plain", "gate records vcf"), M(83, "duplex", "gate records vcf")],
    "syserr_BQ_strand_favor_mul": [M(9, "plain", "records"), M(9, "duplex", "records")],
    "syserr_minABQ_pcr_snv": [M(403, "amplicon", "gate records vcf")],
    "syserr_minABQ_pcr_indel": [M(203, "amplicon", "gate records vcf")],
    "syserr_minABQ_cap_snv": [M(403, "plain", "gate records vcf"), M(403, "duplex", "gate records vcf")],
    "syserr_minABQ_cap_indel": [M(203, "plain", "gate records vcf"), M(203, "duplex", "gate records vcf")],
    "syserr_mut_region_n_bases": [M(25, "plain", "gate planes records vcf"), M(25, "duplex", "gate planes records vcf")],
    "syserr_MQ_min": [M(3, "plain", "records"), M(3, "duplex", "records")],
    "syserr_MQ_max": [M(123, "plain", "gate records vcf"), M(123, "duplex", "gate records vcf")],
    "syserr_MQ_NMR_expfrac": [M(0.351, "plain", "gate records vcf"), M(0.351, "duplex", "gate records vcf")],
    "syserr_MQ_NMR_altfrac_coef": [M(3.7, "plain", "gate records vcf"), M(3.7, "duplex", "gate records vcf")],
    "syserr_MQ_NMR_nonaltfrac_coef": [M(3.7, "plain", "gate records vcf"), M(3.7, "duplex", "gate records vcf")],
    "syserr_MQ_NMR_pl_exponent": [M(5.4, "plain", "gate records vcf"), M(5.4, "duplex", "gate records vcf")],
    "syserr_MQ_nonref_base": [M(68.3, "plain", "gate records vcf"), M(68.3, "duplex", "gate records vcf")],
    "germ_phred_hetero_snp": [M(65, "plain", "gate records vcf"), M(65, "duplex", "gate records vcf")],
    "germ_phred_hetero_indel": [M(83, "plain", "gate records vcf"), M(83, "duplex", "gate records vcf")],
    "germ_phred_homalt_snp": [M(69, "plain", "gate records vcf"), M(69, "duplex", "gate records vcf")],
    "germ_phred_homalt_indel": [M(87, "plain", "gate records"), M(87, "duplex", "gate records")],
    "germ_phred_het3al_snp": [M(121, "plain", "gate records vcf"), M(121, "duplex", "gate records vcf")],
    "germ_phred_het3al_indel": [M(101, "plain", "gate records vcf"), M(101, "duplex", "gate records vcf")],
    "tn_q_inc_max": [M(21, "plain", "gate records vcf"), M(21, "duplex", "gate records vcf")],
    "tn_q_inc_max_sscs_CG_AT": [M(3, "plain", "gate records vcf"), M(3, "duplex", "gate records vcf")],
    "tn_q_inc_max_sscs_other": [M(13, "plain", "gate records vcf"), M(13, "duplex", "gate records vcf")],
    "tn_is_paired": [M(1, "plain", "alleles gate hap planes records vcf", primerlen=12, primer_flag=1), M(1, "duplex", "alleles gate planes records vcf", primerlen=12, primer_flag=1)],
    "indel_BQ_max": [M(87, "plain", "gate planes records vcf"), M(87, "duplex", "gate planes records vcf")],
    "indel_str_repeatsize_max": [M(15, "duplex", "records"), M(15, "amplicon", "records")],
    "indel_polymerase_size": [M(13.9, "plain", "gate planes records vcf"), M(13.9, "duplex", "gate planes records vcf")],
    "indel_polymerase_slip_rate": [M(13.9, "plain", "planes records"), M(13.9, "duplex", "planes records")],
    "indel_del_to_ins_err_ratio": [M(8.8, "plain", "gate planes records vcf"), M(8.8, "duplex", "gate planes records vcf")],
    "indel_adj_tracklen_dist": [M(15, "plain", "gate planes records vcf"), M(15, "duplex", "gate planes records vcf")],
    "indel_adj_indellen_perc": [M(323, "plain", "gate planes records vcf"), M(323, "duplex", "gate planes records vcf")],
    "indel_multiallele_samepos_penal": [M(19.0, "iontorrent", "records")],
    "indel_multiallele_soma_penal_thres": [M(0.0, "weird", "gate records")],
    "indel_tetraallele_germline_penal_value": [M(10000.0, "amplicon", "gate records vcf")],
    "indel_tetraallele_germline_penal_thres": [M(0.0, "amplicon", "gate records vcf")],
    "indel_ins_penal_pseudocount": [M(0, "weird", "gate records")],
    "indel_nonSTR_phred_per_base": [M(13, "plain", "gate planes records vcf"), M(13, "duplex", "gate planes records vcf")],
    "indel_str_phred_per_region": [M(23, "plain", "gate planes records vcf"), M(23, "duplex", "gate planes records vcf")],
    "indel_filter_edge_dist": [M(13, "plain", "alleles gate hap planes records vcf"), M(13, "duplex", "alleles gate planes records vcf")],
    "contam_any_mul_frac": [M(0.334, "plain", "gate records vcf"), M(0.334, "duplex", "gate records vcf")],
    "contam_t2n_mul_frac": [M(0.385, "normal", "gate records vcf")],
    "microadjust_xm": [M(17, "plain", "gate planes records vcf"), M(17, "duplex", "gate planes records vcf")],
    "microadjust_cliplen": [M(13, "plain", "gate planes records vcf"), M(13, "normal", "gate planes records")],
    "microadjust_delFAQmax": [M(200, "plain", "gate planes records vcf", indel_BQ_max=1000), M(200, "duplex", "gate planes records vcf", indel_BQ_max=1000)],
    "microadjust_bias_pos_indel_fold": [M(3.7, "plain", "gate records vcf"), M(3.7, "duplex", "gate records")],
    "microadjust_bias_pos_indel_misma_to_indel_ratio": [M(0.0, "plain", "gate records vcf"), M(17.0, "duplex", "gate records")],
    "microadjust_nobias_pos_indel_misma_to_indel_ratio": [M(0.0, "plain", "gate records vcf", nobias_pos_indel_str_track_len=0), M(0.0, "duplex", "gate records vcf", nobias_pos_indel_str_track_len=0)],
    "microadjust_nobias_pos_indel_maxlen": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "microadjust_nobias_pos_indel_bMQ": [M(0, "plain", "records"), M(0, "duplex", "records")],
    "microadjust_nobias_pos_indel_perc": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "microadjust_nobias_strand_all_fold": [M(8.8, "plain", "records"), M(8.8, "duplex", "gate records")],
    "microadjust_refbias_indel_max": [M(0.0, "normal", "gate records vcf")],
    "microadjust_counterbias_pos_odds_ratio": [M(6.25, "amplicon", "gate records")],
    "microadjust_counterbias_pos_fold_ratio": [M(8.8, "amplicon", "gate records")],
    "microadjust_fam_binom_qual_halving_thres": [M(143, "duplex", "gate records vcf")],
    "microadjust_near_clip_dist": [M(7, "amplicon", "planes vcf")],
    "microadjust_longfrag_sidelength_min": [M(603, "duplex", "gate records")],
    "microadjust_longfrag_sidelength_max": [M(0, "duplex", "gate records")],
    "microadjust_longfrag_sidelength_zeroMQpenalty": [M(510.3, "duplex", "gate records")],
    "microadjust_alignment_clip_min_len": [M(27, "plain", "planes"), M(27, "duplex", "planes vcf")],
    "microadjust_padded_deletion_flag": [M(7, "plain", "gate planes records vcf"), M(7, "duplex", "gate planes records")],
    "microadjust_strand_orientation_absence_DP_fold": [M(13, "plain", "records"), M(13, "duplex", "gate records")],
    "microadjust_orientation_absence_snv_penalty": [M(0, "plain", "gate records vcf", microadjust_strand_orientation_absence_DP_fold=0), M(0, "duplex", "gate records vcf", microadjust_strand_orientation_absence_DP_fold=0)],
    "microadjust_strand_absence_snv_penalty": [M(11, "plain", "records"), M(11, "duplex", "gate records")],
    "microadjust_dedup_absence_indel_penalty": [M(5, "amplicon", "gate records vcf")],
    "microadjust_median_readlen_thres": [M(200, "plain", "gate planes records vcf", microadjust_BAQ_per_base_x1024=4096), M(200, "duplex", "gate planes records vcf", microadjust_BAQ_per_base_x1024=4096)],
    "microadjust_BAQ_per_base_x1024": [M(4096, "plain", "gate planes records vcf", central_readlen=75), M(4096, "duplex", "gate planes records vcf", central_readlen=75)],
    "lib_wgs_min_avg_fraglen": [M(603, "plain", "records"), M(603, "duplex", "gate records")],
    "lib_nonwgs_ad_pseudocount": [M(0.47, "plain", "gate records vcf"), M(0.47, "duplex", "gate records vcf")],
    "lib_nonwgs_clip_penal_min_indelsize": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "lib_nonwgs_normal_full_self_rescue_fa": [M(0.47, "normal", "gate records")],
    "lib_nonwgs_normal_min_self_rescue_fa_ratio": [M(0.64, "normal", "gate records vcf")],
    "lib_nonwgs_normal_max_rescued_MQ": [M(63, "plain", "gate records vcf"), M(63, "duplex", "gate records vcf")],
    "lib_wgs_normal_max_rescued_MQ": [M(3, "plain", "records"), M(3, "duplex", "gate records")],
    "outvar_flag": [M(127, "plain", "gate records vcf"), M(127, "duplex", "gate records vcf")],
    "should_output_all_germline": [M(1, "plain", "gate records vcf", outvar_flag=63), M(1, "duplex", "gate records vcf", outvar_flag=63)],
    "vqual": [M(25.8, "plain", "gate records vcf"), M(25.8, "normal", "records")],
    "vdp1": [M(0, "plain", "records"), M(0, "duplex", "records")],
    "vad1": [M(1, "plain", "records", vdp1=50), M(1, "duplex", "gate records vcf", vdp1=50)],
    "vfa1": [M(0.1, "plain", "gate records vcf", vdp1=50, vqual=1000.0), M(0.3, "duplex", "gate records vcf", vdp1=50, vqual=1000.0)],
    "vdp2": [M(0, "plain", "records"), M(0, "duplex", "records")],
    "vad2": [M(1, "plain", "records", vdp2=50), M(1, "duplex", "gate records vcf", vdp2=50)],
    "vfa2": [M(0.3, "plain", "gate records vcf", vdp2=50, vqual=1000.0), M(0.3, "duplex", "gate records vcf", vdp2=50, vqual=1000.0)],
    "min_r_ad": [M(200, "plain", "records"), M(200, "duplex", "records")],
    "min_a_ad": [M(3, "plain", "gate records vcf"), M(3, "iontorrent", "gate records vcf")],
    "germ_hetero_FA": [M(1.099, "plain", "gate records vcf"), M(1.099, "duplex", "gate records vcf")],
    "tn_syserr_norm_devqual": [M(-1.0, "plain", "gate records vcf"), M(-1.0, "duplex", "gate records vcf")],
    "microadjust_syserr_MQ_NMR_tn_syserr_no_penal_qual_min": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate records vcf")],
    "microadjust_syserr_MQ_NMR_tn_syserr_no_penal_qual_max": [M(0, "plain", "gate records vcf", microadjust_syserr_MQ_NMR_tn_syserr_no_penal_qual_min=0), M(0, "duplex", "gate records vcf", microadjust_syserr_MQ_NMR_tn_syserr_no_penal_qual_min=0)],
    "lib_nonwgs_normal_add_mul_ad": [M(2.0, "normal", "gate records vcf")],
    "inferred_is_vcf_generated": [M(0, "plain", "alleles gate hap planes records vcf"), M(0, "duplex", "alleles gate planes records vcf")],
    "tumor_vcf_is_provided": [M(3, "plain", "gate planes records vcf"), M(3, "duplex", "gate planes records vcf")],
    "tumor_vcf_fname_nonempty": [M(0, "plain", "gate records vcf"), M(0, "duplex", "gate planes records vcf")],
    "phasing_haplotype_max_count": [M(0, "plain", "hap vcf"), M(0, "normal", "hap vcf")],
    "phasing_haplotype_min_ad": [M(5, "plain", "hap vcf"), M(5, "normal", "hap vcf")],
    "phasing_haplotype_max_detail_cnt": [M(9, "plain", "hap vcf"), M(9, "normal", "hap vcf")],
    "microadjust_alignment_clip_min_count": [M(7, "bqfix", "vcf")],
    "microadjust_alignment_tracklen_min": [M(0, "plain", "vcf"), M(0, "duplex", "vcf")],
    "microadjust_alignment_clip_min_frac": [M(0.385, "bqfix", "vcf")],
    "group.kept_aln_min_aln_len": [M(3, "fam_umi", "families"), M(3, "fam_amplicon", "families")],
    "group.kept_aln_min_mapqual": [M(200, "fam_umi", "families"), M(200, "fam_amplicon", "families")],
    "group.kept_aln_min_isize": [M(200, "fam_umi", "families"), M(200, "fam_amplicon", "families")],
    "group.kept_aln_max_isize": [M(4294967297, "fam_umi", "families"), M(4294967297, "fam_amplicon", "families")],
    "group.kept_aln_is_zero_isize_discarded": [M(3, "fam_umi", "families"), M(3, "fam_amplicon", "families")],
    "group.pair_end_merge": [M(3, "fam_umi", "families"), M(3, "fam_amplicon", "families")],
    "group.dedup_flag": [M(3, "fam_umi", "families"), M(3, "fam_amplicon", "families")],
    "group.dedup_center_mult": [M(0.0, "fam_umi", "families"), M(0.0, "fam_amplicon", "families")],
    "group.dedup_amplicon_end2end_ratio": [M(0.0, "fam_amplicon_umi", "families", dedup_amplicon_border_strong_minDP=50.0)],
    "group.dedup_amplicon_border_to_insert_cov_weak_avgDP_ratio": [M(10000.0, "fam_amplicon", "families")],
    "group.dedup_amplicon_border_to_insert_cov_strong_avgDP_ratio": [M(100.0, "fam_amplicon", "families", dedup_amplicon_border_strong_minDP=50.0), M(100.0, "fam_amplicon_umi", "families", dedup_amplicon_border_strong_minDP=50.0)],
    "group.dedup_amplicon_border_to_insert_cov_weak_totDP_ratio": [M(1.2, "fam_amplicon", "families")],
    "group.dedup_amplicon_border_to_insert_cov_strong_totDP_ratio": [M(0.5, "fam_amplicon", "families", dedup_amplicon_border_strong_minDP=50.0), M(0.5, "fam_amplicon_umi", "families", dedup_amplicon_border_strong_minDP=50.0)],
    "group.dedup_amplicon_border_weak_minDP": [M(0.0, "fam_amplicon", "families")],
    "group.dedup_amplicon_border_strong_minDP": [M(0.0, "fam_amplicon", "families")],
    "group.fetch_tbeg": [M(100500, "fam_umi", "families"), M(100500, "fam_amplicon", "families")],
    "group.fetch_tend": [M(102500, "fam_umi", "families"), M(102500, "fam_amplicon", "families")],
    "group.end2end": [M(3, "fam_umi", "families"), M(3, "fam_amplicon", "families")],
    "group.inferred_sequencing_platform": [M(2, "fam_umi", "families")],

}
