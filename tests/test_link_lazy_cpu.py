"""uvc_amd/csrc/uvc_link.h holds the host-side rules of the lazy completion of LINK_M: where the need / done marks live, which
entry asks for which scope of windows, and what a handle remembers.  tests/native/link_host_main.cpp runs them against a stub of the device
side (two byte arrays and a pass that walks them as the kernel does).  Built with the undefined-behaviour and address sanitizers as a
stand-alone program; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_link_scopes_marks_layout_and_state_machine_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "link_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "link_host_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout
    assert "link rules: 0 failures" in r.stdout, r.stdout
