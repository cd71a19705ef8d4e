"""uvc_amd/csrc/uvc_score_rows.h declares the staged rows of the scoring path once and derives from that one table the scratch layout of a
one-call score, the row set of a streamed chunk and the bytes per record that --score-mem-mb divides by; it compiles for the host alone.
tests/native/score_layout_host_main.cpp sweeps the layouts there (alignment, order, room, the rows per group min(groups, capacity) long,
the zeroed head) and holds the sizes to the values of the commit that still spelled them out by hand.  Built with the undefined-behaviour
sanitizer as a stand-alone program; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_row_layouts_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "score_layout_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "score_layout_host_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout
    assert "row blocks and sets 405 cases, scratch 63, set_bytes literals 4, 0 failures" in r.stdout, r.stdout
