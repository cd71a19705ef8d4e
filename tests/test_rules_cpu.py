"""uvc_amd/csrc/uvc_rules.h holds the reference rules that several kernels (and host code) share, as pure integer functions that compile for
the host too.  tests/native/rules_host_main.cpp checks them there: the pair consensus of a plain fragment against the generic
fill_consensus path it stands in for (7 350 cases), the zero-value quality threshold, and is_fam_good at its boundaries.  Built with the
undefined-behaviour sanitizer as a stand-alone program; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_rules_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "rules_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "rules_host_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout
    assert "pair_consensus 7350 cases, zero_value_qual 12, is_fam_good 13, 0 failures" in r.stdout, r.stdout
