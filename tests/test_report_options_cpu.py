"""The six report options (--coverage-out, --error-profile-out, --family-stats-out, --callable-out, --msi-out, --read-profile-out) refuse
the same runs in the same sentence: only the option's name and its own words for why differ.  Their whole-number sub-options, and the two
other whole-number options of the command line, take and refuse the same spellings in one sentence.  The messages are read from the built
uvc1-mi355x; no file is opened and no device is needed, every refusal comes first."""
import math
import os
import re
import subprocess

import pytest

from uvc_amd import _ffi

EXE = os.path.join(_ffi.ROOT, "uvc_amd", "csrc", "uvc1-mi355x")
BASE = ["in.bam", "-f", "ref.fa", "-o", "o.vcf.gz"]
PAIR = ["t.bam", "--normal-bam", "n.bam", "-f", "ref.fa", "-o", "n.vcf.gz", "--tumor-output", "t.vcf.gz"]
# option -> (its window option or None, why no --shard, why no --repeat, what pair mode does not write)
REPORTS = {
    "--coverage-out": ("--coverage-window", "a target can straddle shards", "every tile would be counted that many times", "coverage report"),
    "--error-profile-out": (None, "every shard would write a part of the table", "every tile would be counted that many times", "error profile"),
    "--family-stats-out": ("--family-stats-window", "a target can straddle shards", "every tile would be counted that many times", "family report"),
    "--callable-out": (None, "a target can straddle shards", "every tile would report its runs that many times", "callable regions"),
    "--msi-out": (None, "a target can straddle shards", "every tile would report its loci that many times", "microsatellite tally"),
    "--read-profile-out": (None, "every shard would write a part of the profile", "every tile would be counted that many times", "read profile"),
}
WINDOWED = [opt for opt, row in REPORTS.items() if row[0]]


def refusal(args, cwd):
    assert os.path.exists(EXE), "build it: make -C uvc_amd/csrc"
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=str(cwd))
    assert r.returncode == 2 and os.listdir(cwd) == [], (args, r.returncode, r.stderr)
    lines = r.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith("uvc1-mi355x: "), r.stderr
    return lines[0][len("uvc1-mi355x: "):]


def with_windows(opt):
    """The option with what it needs to get past its window rules: a window length where it has one."""
    w = REPORTS[opt][0]
    return [opt, "r.out"] + ([w, "1000"] if w else [])


@pytest.mark.parametrize("opt", list(REPORTS))
def test_the_runs_no_report_comes_from(tmp_path, opt):
    _, no_shard, no_repeat, _ = REPORTS[opt]
    assert refusal(["/only-print-vcf-header/"] + with_windows(opt), tmp_path) == opt + " cannot go with /only-print-vcf-header/: no tile is called"
    assert refusal(BASE + with_windows(opt) + ["--shard", "1/3"], tmp_path) == "%s cannot go with --shard 1/3: %s, and --concat joins VCFs only" % (opt, no_shard)
    assert refusal(BASE + with_windows(opt) + ["--repeat", "4"], tmp_path) == "%s cannot go with --repeat 4: %s" % (opt, no_repeat)
    # several faults at once: the header-only run is named first, then the shard, then the repeat
    assert "/only-print-vcf-header/" in refusal(["/only-print-vcf-header/"] + with_windows(opt) + ["--shard", "1/3", "--repeat", "4"], tmp_path)
    assert "--shard 1/3" in refusal(BASE + with_windows(opt) + ["--shard", "1/3", "--repeat", "4"], tmp_path)


@pytest.mark.parametrize("opt", WINDOWED)
def test_the_targets_of_a_windowed_report(tmp_path, opt):
    w = REPORTS[opt][0]
    assert refusal(BASE + [opt, "r.out", w, "1000", "-R", "p.bed"], tmp_path) == "%s cannot go with -R / --bed-in-fname: with a BED file the targets of %s are its lines" % (w, opt)
    assert refusal(BASE + [opt, "r.out", w, "1000", "--bed-in-fname", "p.bed"], tmp_path) == "%s cannot go with -R / --bed-in-fname: with a BED file the targets of %s are its lines" % (w, opt)
    assert refusal(BASE + [opt, "r.out"], tmp_path) == "%s needs %s N without -R / --bed-in-fname: there are no BED lines to report on" % (opt, w)
    assert refusal(BASE + [w, "1000"], tmp_path) == "%s needs %s: it only shapes that report" % (w, opt)
    for bad in ("0", "-5", "2.5", "true", "x", "", "3e10"):
        assert refusal(BASE + [opt, "r.out", w + "=" + bad], tmp_path) == "%s takes a window length in bp, not '%s'" % (w, bad)
    # the run comes before the targets
    assert "--repeat 2" in refusal(BASE + [opt, "r.out", "--repeat", "2"], tmp_path)


def test_the_sentences_are_the_same_for_every_report(tmp_path):
    """What is left of each refusal once the option's name and its own words are taken out is one text for all six."""
    frames = {}
    for opt, (w, no_shard, no_repeat, writes) in REPORTS.items():
        got = [refusal(["/only-print-vcf-header/"] + with_windows(opt), tmp_path),
               refusal(BASE + with_windows(opt) + ["--shard", "0/2"], tmp_path).replace(no_shard, "<why>"),
               refusal(BASE + with_windows(opt) + ["--repeat", "2"], tmp_path).replace(no_repeat, "<why>"),
               refusal(PAIR + [opt, "r.out"], tmp_path).replace(writes, "<what>")]
        if w:
            got += [refusal(BASE + [opt, "r.out", w, "50", "-R", "p.bed"], tmp_path), refusal(BASE + [opt, "r.out"], tmp_path)]
            got = [g.replace(w, "<window>") for g in got]
        frames[opt] = [g.replace(opt, "<opt>") for g in got]
        assert all("<opt>" in g for g in frames[opt]) and "<why>" in frames[opt][1] and "<why>" in frames[opt][2] and "<what>" in frames[opt][3], frames[opt]
    first = frames["--coverage-out"]
    assert len(first) == 6 and frames["--family-stats-out"] == first
    assert frames["--error-profile-out"] == first[:4] and frames["--callable-out"] == first[:4]
    assert frames["--msi-out"] == first[:4] and frames["--read-profile-out"] == first[:4]


@pytest.mark.parametrize("opt", list(REPORTS))
def test_pair_mode_writes_no_report(tmp_path, opt):
    w, _, _, writes = REPORTS[opt]
    assert refusal(PAIR + [opt, "r.out"], tmp_path) == "%s cannot go with --normal-bam: pair mode has its own tile loop and writes no %s" % (opt, writes)
    if w:
        assert refusal(PAIR + [w + "=100"], tmp_path) == "%s cannot go with --normal-bam: pair mode has its own tile loop and writes no %s" % (w, writes)


# ---- every report option and sub-option; the whole-number options ----
# report -> its sub-options, each with a value it takes (written out here, not read from the program: an option the program's table
# forgets is then accepted in pair mode, and the test fails)
SUBS = {
    "--coverage-out": {"--coverage-thresholds": "1,20", "--coverage-window": "1000"},
    "--error-profile-out": {"--error-profile-min-depth": "5", "--error-profile-max-alt-permille": "10"},
    "--family-stats-out": {"--family-stats-window": "1000"},
    "--callable-out": {"--callable-min-depth": "cDP12=5", "--callable-max-aDP": "7"},
    "--msi-out": {"--msi-min-tract": "8", "--msi-min-units": "3", "--msi-max-unit": "4", "--msi-min-depth": "9", "--msi-unstable-permille": "100"},
    "--read-profile-out": {"--read-profile-min-mapq": "1", "--read-profile-min-depth": "5", "--read-profile-max-alt-permille": "10"},
}
# report -> the one sentence for its sub-options without it; None: one per sub-option, "<sub> needs <report>: it only shapes that report"
NEEDS = {
    "--coverage-out": None,
    "--error-profile-out": "--error-profile-min-depth and --error-profile-max-alt-permille need --error-profile-out: they only gate that report",
    "--family-stats-out": None,
    "--callable-out": "--callable-min-depth and --callable-max-aDP need --callable-out: they only set the criteria of that file",
    "--msi-out": "--msi-min-tract, --msi-min-units, --msi-max-unit, --msi-min-depth and --msi-unstable-permille need --msi-out: they only shape that file",
    "--read-profile-out": "--read-profile-min-mapq, --read-profile-min-depth and --read-profile-max-alt-permille need --read-profile-out: they only gate that report",
}
# whole-number option -> (lo, hi, spelling, what it "takes"); the spellings:
#   strtod       what C's strtod reads to the end of the value with no blank in front, finite; not true / false
#   digits       [0-9]+ only
#   strtod+bool  strtod, and true is 1, false is 0
A_WINDOW, A_DEPTH, PERMILLE, AT_LEAST_1 = "a window length in bp", "a depth of at least 1", "thousandths from 0 to 1000", "a whole number of at least 1"
NUMBERS = {
    "--coverage-window": (1, 2e9, "strtod", A_WINDOW), "--family-stats-window": (1, 2e9, "strtod", A_WINDOW),
    "--error-profile-min-depth": (1, 2e9, "strtod", A_DEPTH), "--read-profile-min-depth": (1, 2e9, "strtod", A_DEPTH),
    "--error-profile-max-alt-permille": (0, 1000, "strtod", PERMILLE), "--read-profile-max-alt-permille": (0, 1000, "strtod", PERMILLE),
    "--read-profile-min-mapq": (0, 255, "strtod", "a mapping quality from 0 to 255"),
    "--msi-min-tract": (1, 2e9, "strtod", AT_LEAST_1), "--msi-min-units": (1, 2e9, "strtod", AT_LEAST_1),
    "--msi-max-unit": (1, 2e9, "strtod", AT_LEAST_1), "--msi-min-depth": (1, 2e9, "strtod", AT_LEAST_1),
    "--msi-unstable-permille": (0, 2e9, "strtod", "thousandths of the depth (a whole number >= 0)"),
    "--score-mem-mb": (0, 1e9, "strtod", "a size in MiB (0 = off)"),
    "--callable-max-aDP": (0, 2e9, "digits", "a depth (0 = off)"),
    "--merge-regions": (0, 2e9, "strtod+bool", "a distance in bp (0 = off)"),
}
VALUES = ["0", "1", "-1", "2.5", "true", "false", "x", "", "1e3", "0x10", "+5", " 5", "5 ", "3e10", "1000", "1001", "255", "256", "2000000000", "2000000001"]
PRINT = ["--sequencing-platform", "1", "--print-params"]   # a given platform: exit 0 behind all option checks, no file, no device


def c_strtod(v):
    """The value of v where C's strtod reads all of it and it does not begin with a blank, else None."""
    if v == "" or v != v.strip() or "_" in v:
        return None
    try:
        x = float.fromhex(v) if v.lstrip("+-")[:2].lower() == "0x" else float(v)
    except ValueError:
        return None
    return x if math.isfinite(x) else None


def taken(opt, v):
    """Whether the table says that `opt` takes the value `v`."""
    lo, hi, spelling, _ = NUMBERS[opt]
    if v in ("true", "false"):
        x = float(v == "true") if spelling == "strtod+bool" else None
    elif spelling == "digits":
        x = float(v) if re.fullmatch("[0-9]+", v) else None
    else:
        x = c_strtod(v)
    return x is not None and lo <= x <= hi and x == int(x)


def test_the_table_of_spellings():
    """The expectations below come from the table: what it says of the spellings the issue names."""
    assert [v for v in VALUES if taken("--msi-min-depth", v)] == ["1", "1e3", "0x10", "+5", "1000", "1001", "255", "256", "2000000000"]
    assert [v for v in VALUES if taken("--callable-max-aDP", v)] == ["0", "1", "1000", "1001", "255", "256", "2000000000"]
    assert [v for v in VALUES if taken("--merge-regions", v)] == ["0", "1", "true", "false", "1e3", "0x10", "+5", "1000", "1001", "255", "256", "2000000000"]
    assert len(NUMBERS) * len(VALUES) == 300


@pytest.mark.parametrize("group", list(REPORTS) + ["--score-mem-mb", "--merge-regions"])
def test_every_report_option_and_whole_number(tmp_path, group):
    """A report with all of its sub-options, or one of the two other whole-number options: each whole-number option over VALUES as the
    table has it, then per report a sub-option without the report, an empty path, and every option of it in pair mode."""
    report = group if group in REPORTS else None
    window = REPORTS[report][0] if report else None
    front = BASE + PRINT + ([report, "r.out"] if report else ["-R", "p.bed"] if group == "--merge-regions" else [])
    for opt in ([o for o in SUBS[report] if o in NUMBERS] if report else [group]):
        for v in VALUES:
            args = front + ([window, "1000"] if window and opt != window else []) + [opt + "=" + v]
            if taken(opt, v):
                r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
                assert (r.returncode, r.stderr) == (0, "") and "vqual=" in r.stdout and os.listdir(tmp_path) == [], (args, r.returncode, r.stderr)
            else:
                assert refusal(args, tmp_path) == "%s takes %s, not '%s'" % (opt, NUMBERS[opt][3], v), args
    if not report:
        return
    writes = REPORTS[report][3]
    assert refusal(BASE + [report, ""], tmp_path) == report + " needs a path"
    assert refusal(BASE + [report + "="], tmp_path) == report + " needs a path"
    for opt, value in [(report, "r.out")] + list(SUBS[report].items()):
        for args in ([opt, value], [opt + "=" + value]):
            assert refusal(PAIR + args, tmp_path) == "%s cannot go with --normal-bam: pair mode has its own tile loop and writes no %s" % (opt, writes)
    for sub, value in SUBS[report].items():
        assert refusal(BASE + [sub, value], tmp_path) == (NEEDS[report] or "%s needs %s: it only shapes that report" % (sub, report))
        assert refusal(BASE + PRINT + [sub + "=" + value], tmp_path) == (NEEDS[report] or "%s needs %s: it only shapes that report" % (sub, report))
