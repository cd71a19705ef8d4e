"""The four report options (--coverage-out, --error-profile-out, --family-stats-out, --callable-out) refuse the same runs in the same
sentence: only the option's name and its own words for why differ.  The messages are read from the built uvc1-mi355x; no file is opened and
no device is needed, every refusal comes first."""
import os
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
    """What is left of each refusal once the option's name and its own words are taken out is one text for all four."""
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


@pytest.mark.parametrize("opt", list(REPORTS))
def test_pair_mode_writes_no_report(tmp_path, opt):
    w, _, _, writes = REPORTS[opt]
    assert refusal(PAIR + [opt, "r.out"], tmp_path) == "%s cannot go with --normal-bam: pair mode has its own tile loop and writes no %s" % (opt, writes)
    if w:
        assert refusal(PAIR + [w + "=100"], tmp_path) == "%s cannot go with --normal-bam: pair mode has its own tile loop and writes no %s" % (w, writes)
