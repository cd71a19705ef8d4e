"""The host-side rules of the sparse completion pass of LINK_M in uvc_amd/csrc/uvc_link.h: how a class list of a window is cut
into slices for the waves of a block, where the window list and its count live, which score request asks for which scope now that the host
passes the keyed and forced positions, and the state machine of an accumulate with an early and a final phase.
tests/native/link_sparse_main.cpp runs them against a stub of the device side.  Built with the address and undefined-behaviour sanitizers as
a stand-alone program; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slices_list_layout_scopes_and_two_phase_state_machine_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "link_sparse")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "link_sparse_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout
    assert "sparse link rules: 0 failures" in r.stdout, r.stdout
