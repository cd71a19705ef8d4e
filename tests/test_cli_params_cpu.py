"""The parameter surface of uvc1-mi355x and of the C ABI, without a device: every option of the reference's command line is classified,
every ledger move (tests/param_moves.py) reaches its row of the resolved parameters (--print-params), the platform step comes after the
user's values, bad values are refused before any file or device is opened, and uvcgpu_param_set / region.set_param cover every row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bamwriter
from param_moves import MOVES
from uvc_amd import _ffi, group, region

ROOT = _ffi.ROOT
EXE = os.path.join(ROOT, "uvc_amd", "csrc", "uvc1-mi355x")


def run(args, timeout=60):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def option(field):
    return "--" + field.replace("_", "-")


def write_bam(d, name, paired, quals, n=300, readlen=100):
    """A small BAM + FASTA: `n` reads of one length on one contig, paired (Illumina-like) or single-end with the given base qualities."""
    rng = np.random.default_rng(7)
    L = 20000
    ref = rng.integers(0, 4, L)
    recs = []
    for i in range(n):
        pos = 1000 + 30 * i
        fl = (1 | 2 | (0x40 if i % 2 == 0 else 0x80) | (0x10 if i % 2 else 0x20)) if paired else (0x10 if i % 2 else 0)
        recs.append(dict(tid=0, pos=pos, qname="q%d" % (i // 2 if paired else i), flag=fl, mapq=50 + i % 11, cigar=[(0, readlen)],
                         bases=ref[pos:pos + readlen].astype(np.uint8), quals=np.full(readlen, quals, np.uint8),
                         mtid=(0 if paired else -1), mpos=(pos if paired else -1), tlen=0, nm=0))
    bam = str(d / (name + ".bam"))
    bamwriter.write_bam(bam, [("chrP", L)], recs)
    bamwriter.write_fasta(str(d / (name + ".fa")), [("chrP", "".join("ACGT"[i] for i in ref))])
    return bam


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("clip")
    return dict(illumina=write_bam(d, "ill", True, 35), iontorrent=write_bam(d, "ion", False, 24))


def print_params(bam, *args):
    r = run([bam, "--print-params"] + list(args))
    assert r.returncode == 0, r.stderr
    rows = [l.split("=", 1) for l in r.stdout.splitlines()]
    return dict(rows), [k for k, _ in rows]


def help_classes():
    r = run(["--help"])
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("  -"):
            names, cls = line.split()[:2]
            for n in names.split(","):
                assert n not in out, n
                out[n] = cls.strip("[]")
    return out


def test_every_reference_option_is_classified():
    classes = help_classes()
    golden = [l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "ref_cli_option_names.txt")) if l.strip()]
    assert len(golden) > 250
    missing = [n for n in golden if n not in classes]
    assert not missing, missing
    assert set(classes.values()) == {"PARAM", "GROUP", "CLI", "MODE", "INERT", "UNSUPPORTED"}
    # every settable row of both .def files is an option (its own PARAM / GROUP line, or a CLI / MODE switch that sets it)
    for row in region.param_table():
        if row["settable"]:
            assert option(row["name"]) in classes, row["name"]
        else:
            assert option(row["name"]) not in classes, row["name"]


def test_resolved_rows_are_the_def_rows(bams):
    vals, order = print_params(bams["illumina"])
    assert order == [r["name"] for r in region.param_table()]


def _cli_moves():
    """(field, value, group?) of every ledger move of a settable row; values outside int32 are expected to be refused"""
    settable = {r["name"]: r for r in region.param_table() if r["settable"]}
    out = []
    for key, moves in MOVES.items():
        field = key[len("group."):] if key.startswith("group.") else key
        if field in settable:
            for m in moves:
                out.append((field, m.value, settable[field]["kind"]))
    return out


# the MODE switches that set a row take the reference's enum values only (common.hpp:124-146)
ENUM_ROWS = {"molecule_tag": 3, "disable_duplex": 1, "pair_end_merge": 1}


def test_every_ledger_move_reaches_its_row_only(bams):
    moves = _cli_moves()
    assert len(moves) > 120
    base, _ = print_params(bams["illumina"], "--sequencing-platform", "3")
    for field, value, kind in moves:
        if (kind == "int" and not (-2 ** 31 <= value < 2 ** 31)) or (field in ENUM_ROWS and not 0 <= value <= ENUM_ROWS[field]):
            r = run([bams["illumina"], "--print-params", option(field), value])
            assert r.returncode == 2 and option(field) in r.stderr, (field, value, r.stderr)
            continue
        got, _ = print_params(bams["illumina"], option(field), repr(value) if isinstance(value, float) else value, "--sequencing-platform", "3")
        diff = {k for k in base if base[k] != got[k]}
        assert diff <= {field}, (field, diff)
        assert (int(got[field]) == value) if kind == "int" else (float(got[field]) == float(value)), (field, value, got[field])
        if float(value) != float(base[field]):
            assert diff == {field}, field


def test_option_and_equals_forms_agree(bams):
    a, _ = print_params(bams["illumina"], "--fam-thres-highBQ-snv", "7", "--kept-aln-min-mapqual=9", "--vqual=3.5", "-q", "4.5")
    assert a["fam_thres_highBQ_snv"] == "7" and a["kept_aln_min_mapqual"] == "9" and a["vqual"] == "4.5"   # the last value wins


def test_platform_step_after_the_user_values(bams):
    ill, ion = bams["illumina"], bams["iontorrent"]
    # AUTO infers Illumina / IonTorrent from the first alignments and adds the deltas on top of the user's values
    a, _ = print_params(ill, "--syserr-minABQ-pcr-snv", "50")
    assert a["inferred_sequencing_platform"] == "1" and a["syserr_minABQ_pcr_snv"] == "250" and a["syserr_minABQ_cap_indel"] == "100"
    assert a["central_readlen"] == "100" and a["inferred_maxMQ"] == "60"
    b, _ = print_params(ion, "--fam-thres-highBQ-snv", "50", "--bias-thres-highBQ", "10")
    assert b["inferred_sequencing_platform"] == "2" and b["fam_thres_highBQ_snv"] == "20" and b["bias_thres_highBQ"] == "0"   # dec(v, 30), dec(v, 13)
    assert b["bq_phred_added_misma"] == "8" and b["syserr_minABQ_pcr_snv"] == "0"
    # OTHER records the inferred platform and keeps the deltas off
    c, _ = print_params(ion, "--fam-thres-highBQ-snv", "50", "--sequencing-platform", "3")
    assert c["inferred_sequencing_platform"] == "2" and c["fam_thres_highBQ_snv"] == "50" and c["bq_phred_added_misma"] == "0"
    c, _ = print_params(ill, "--sequencing-platform", "3")
    assert c["inferred_sequencing_platform"] == "1" and c["syserr_minABQ_pcr_snv"] == "0"
    # a given platform is taken as it is, without a look at the file: the IonTorrent-like file called as Illumina
    d, _ = print_params(ion, "--sequencing-platform", "1", "--syserr-minABQ-pcr-snv", "50")
    assert d["inferred_sequencing_platform"] == "1" and d["syserr_minABQ_pcr_snv"] == "250" and d["central_readlen"] == "0"
    r = run(["/no/such.bam", "--print-params", "--sequencing-platform", "2"])
    assert r.returncode == 0 and "inferred_sequencing_platform=2\n" in r.stdout, r.stderr
    # central_readlen: 0 = inferred, any other value stays
    e, _ = print_params(ill, "--central-readlen", "75")
    assert e["central_readlen"] == "75"
    r = run([ill, "--print-params", "--sequencing-platform", "4"])
    assert r.returncode == 2 and "--sequencing-platform" in r.stderr


@pytest.mark.parametrize("args,named", [
    (["--fam-thres-highBQ-snv", "abc"], "--fam-thres-highBQ-snv"),
    (["--fam-thres-highBQ-snv", "1e99"], "--fam-thres-highBQ-snv"),
    (["--min-altdp-thres", "99999999999"], "--min-altdp-thres"),
    (["--vfa1", "nan"], "--vfa1"),
    (["--vfa1=1e999"], "--vfa1"),
    (["--kept-aln-min-isize", "3.5"], "--kept-aln-min-isize"),
    (["--bias-thres-interfering-indel", "10001"], "bias_thres_interfering_indel above 10000"),
    (["--indel-str-repeatsize-max", "0"], "bad repeat-size parameters"),
    (["--fam-consensus-out-fastq", "out"], "--fam-consensus-out-fastq"),
    (["--fam-consensus-out-fastq-thres-dup1add", "3"], "--fam-consensus-out-fastq-thres-dup1add"),
    (["--should-add-note", "1"], "--should-add-note"),
    (["--debug-tid", "0"], "--debug-tid"),
    (["--debug-pos", "5"], "--debug-pos"),
    (["--bed-in-avg-sequencing-DP", "300"], "--bed-in-avg-sequencing-DP"),
    (["--bed-in-avg-sequencing-DP-n-from-t", "1"], "--bed-in-avg-sequencing-DP-n-from-t"),
    (["--assay-type", "3"], "--assay-type"),
    (["--assay-type", "1e99"], "--assay-type"),
    (["--sequencing-platform=-1"], "--sequencing-platform"),
    (["--pair-end-merge", "2"], "--pair-end-merge"),
    (["--molecule-tag", "4"], "--molecule-tag"),
    (["--disable-duplex", "2"], "--disable-duplex"),
    (["--debug-note-flag", "1"], "--debug-note-flag"),
    (["--inferred-maxMQ", "61"], "unknown option"),
    (["--always-log", "x"], "--always-log"),
])
def test_refusals_come_before_any_file_or_device(args, named):
    """A BAM that does not exist: the refusal is the first thing the program says, with exit status 2."""
    for mode in ([], ["--print-params"]):
        r = run(["/no/such.bam", "-f", "/no/such.fa", "-o", "/no/such/out.vcf.gz"] + mode + args)
        assert r.returncode == 2 and named in r.stderr, (args, r.stderr)
        assert "such" not in r.stderr and "HIP" not in r.stderr, r.stderr


def test_unsupported_options_at_their_defaults_are_accepted(bams):
    base, _ = print_params(bams["illumina"])
    got, _ = print_params(bams["illumina"], "--fam-consensus-out-fastq", "", "--fam-consensus-out-fastq-thres-dup1add", "1", "--should-add-note", "false",
                          "--debug-tid", "-1", "--debug-pos=-1", "--debug-note-flag", "0", "--bed-in-avg-sequencing-DP", "-1", "--bed-in-avg-sequencing-DP-n-from-t", "0")
    assert got == base


def test_inert_options_change_nothing(bams):
    classes = help_classes()
    inert = sorted(n for n, c in classes.items() if c == "INERT")
    assert {"--always-log", "--bias-thres-aXM1T-add", "--microadjust-fam-lowfreq-invFA", "--bias-thres-PFXM1T-add"} <= set(inert)
    base, _ = print_params(bams["illumina"])
    args = []
    for n in inert:
        args += [n, "1"]
    got, _ = print_params(bams["illumina"], *args)
    assert got == base


def test_header_mode(tmp_path):
    def header(*args):
        r = run(["/only-print-vcf-header/"] + list(args))
        assert r.returncode == 0, r.stderr
        return [l for l in r.stdout.splitlines() if not l.startswith(("##fileDate=", "##variantCallerCommand="))]
    a = header()
    assert a[0] == "##fileformat=VCFv4.2" and a[-1].startswith("#CHROM\tPOS")
    b = header("--germ-phred-hetero-indel", "50")
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and len(diff) == 1 and "plus 9." in diff[0][0] and "plus 19." in diff[0][1]
    c = header("--sequencing-platform", "2")
    diff = [(x, y) for x, y in zip(a, c) if x != y]
    assert len(diff) == 1 and diff[0][1].startswith("##variantCallerInferredParameters=(inferred_sequencing_platform=IonTorrent")


def test_help_and_version():
    r = run(["--help"])
    assert r.returncode == 0 and "--fam-thres-highBQ-snv [PARAM] default=25" in r.stdout and "--dedup-center-mult [GROUP] default=5" in r.stdout
    r = run(["-v"])
    assert r.returncode == 0 and "uvcgpu" in r.stdout


def test_set_param_round_trips_every_row():
    rows = region.param_table()
    assert len(rows) == len(_ffi.PARAM_INTS) + len(_ffi.PARAM_DBLS) + len(group.GROUP_INTS) + len(group.GROUP_DBLS)
    p = _ffi.UvcParams()
    region.gpu_lib().call("params_default", C.byref(p))
    g = group.default_params(region.gpu_lib(), 0, 1)
    for r in rows:
        target = p if r["owner"] == "params" else g
        assert getattr(target, r["name"]) == r["default"], r["name"]
        if not r["settable"]:
            with pytest.raises(region.UvcError):
                region.set_param(p, g, r["name"], 1)
            continue
        v = (r["default"] + 3 if r["default"] < 2 ** 31 - 3 else 5) if r["kind"] == "int" else r["default"] * 1.5 + 0.1
        region.set_param(p, g, r["name"].replace("_", "-") if len(r["name"]) % 2 else r["name"], v)
        assert getattr(target, r["name"]) == v, r["name"]
    region.set_param(p, None, "fam_thres_highBQ_snv", True)
    assert p.fam_thres_highBQ_snv == 1
    region.set_param(p, None, "fam_thres_highBQ_snv", "false")
    assert p.fam_thres_highBQ_snv == 0


def test_c_abi_param_set_refuses_and_names_the_row():
    lib = region.gpu_lib()
    f = lib.dll.uvcgpu_param_set
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
    p = _ffi.UvcParams()
    lib.call("params_default", C.byref(p))
    einval = _ffi.ENUMS["UVCGPU_EINVAL"]
    for name, value in ((b"fam_thres_highBQ_snv", b" 7"), (b"fam_thres_highBQ_snv", b"7x"), (b"fam_thres_highBQ_snv", b""), (b"vfa1", b"inf"),
                        (b"fam-thres-highbq-snv", b"7"), (b"struct_size", b"7"), (b"tumor_vcf_is_provided", b"1")):
        assert f(C.addressof(p), None, name, value) == einval, (name, value)
    assert f(C.addressof(p), None, b"vfa1", b"x") == einval and "vfa1" in lib.last_error()
    assert f(None, None, b"vfa1", b"0.5") == einval                         # its struct is missing
    assert p.fam_thres_highBQ_snv == 25 and p.vfa1 == 0.002                 # nothing changed
    assert f(C.addressof(p), None, b"--fam-thres-highBQ-snv"[2:], b"-7") == 0 and p.fam_thres_highBQ_snv == -7
    chk = lib.dll.uvcgpu_params_check
    chk.restype, chk.argtypes = C.c_int, [C.POINTER(_ffi.UvcParams)]
    lib.call("params_default", C.byref(p))
    assert chk(C.byref(p)) == 0
    p.bias_thres_interfering_indel = 10001
    assert chk(C.byref(p)) == _ffi.ENUMS["UVCGPU_EUNSUPPORTED"] and lib.last_error() == "bias_thres_interfering_indel above 10000"
    p.bias_thres_interfering_indel, p.indel_str_repeatsize_max = 5, 0
    assert chk(C.byref(p)) == einval and lib.last_error() == "bad repeat-size parameters"
    p.indel_str_repeatsize_max, p.struct_size = 6, 8
    assert chk(C.byref(p)) == einval and lib.last_error() == "UvcParams::struct_size mismatch"


def test_params_check_bounds_the_quality_addends():
    """bq_phred_added_misma / _indel within -256 .. 3840 (the kernels' value tables and 16-bit fields), and no negative addend beside a
    bias_thres_PFBQ1 / 2 of 0 -- the IonTorrent default -- where the reference divides by zero for a value below 0."""
    lib = region.gpu_lib()
    chk = lib.dll.uvcgpu_params_check
    chk.restype, chk.argtypes = C.c_int, [C.POINTER(_ffi.UvcParams)]
    unsupported = _ffi.ENUMS["UVCGPU_EUNSUPPORTED"]
    for plat, ok_negative in ((1, True), (2, False)):
        for name in ("bq_phred_added_misma", "bq_phred_added_indel"):
            p = region.default_params(lib, platform=plat)
            assert chk(C.byref(p)) == 0 and (p.bias_thres_PFBQ1 == 0) == (plat == 2)
            setattr(p, name, 3840); assert chk(C.byref(p)) == 0
            setattr(p, name, 3841); assert chk(C.byref(p)) == unsupported and lib.last_error().endswith("above 3840")
            setattr(p, name, -1); assert (chk(C.byref(p)) == 0) == ok_negative
            if not ok_negative:
                assert lib.last_error().endswith("bias_thres_PFBQ1 or bias_thres_PFBQ2 of 0")
                p.bias_thres_PFBQ1 = 25; assert chk(C.byref(p)) == unsupported          # bias_thres_PFBQ2 is still 0
                p.bias_thres_PFBQ2 = 30
            setattr(p, name, -256); assert chk(C.byref(p)) == 0
            setattr(p, name, -257); assert chk(C.byref(p)) == unsupported and lib.last_error().endswith("below -256")


def test_apply_platform_ex_matches_apply_platform():
    """AUTO is uvcgpu_params_apply_platform; the Python restatement region.apply_platform agrees with both"""
    lib = region.gpu_lib()
    for plat in (1, 2):
        a, b = _ffi.UvcParams(), _ffi.UvcParams()
        lib.call("params_default", C.byref(a)); lib.call("params_default", C.byref(b))
        region.apply_platform_ex(a, 0, plat, 101, 57)
        region.apply_platform(b, plat, 101, 57)
        assert bytes(a) == bytes(b)
    with pytest.raises(region.UvcError):
        region.apply_platform_ex(a, 4, 1, 100, 60)
