"""include/uvc_field_groups.def states the plane groups of a region handle once; uvc_amd/csrc/uvc_planes.h derives from it the bytes and
columns of a group, the layout of the plane slab and the rows of the zero-fill table, and uvc_amd/_ffi.py the dtype and shape of a fetched
group.  tests/native/planes_host_main.cpp sweeps the derived values on the host and holds them to the values of the commit that still spelled
them out by hand in ten places.  Built with the undefined-behaviour and address sanitizers as a stand-alone program; nothing is loaded into
Python."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_layout_and_zero_fill_rows_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "planes_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "native", "planes_host_main.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout
    assert "layouts 9, printed 2, zero-fill rows 11619, 0 failures" in r.stdout, r.stdout   # 9 lengths x (1 288 planes + p5flag x 2 + occ)


# _ffi.FIELD_GROUPS as the commit before this table wrote it out: name -> (id, dtype, planes per position as a shape prefix)
FIELD_GROUPS_BEFORE = {
    "PREP32": (0, np.int32, (26,)),
    "PREP64": (1, np.int64, (12,)),
    "THRES": (2, np.int32, (18,)),
    "SEG32": (3, np.int32, (30, 14)),
    "SEG64": (4, np.int64, (4, 14)),
    "VQ": (5, np.int32, (14, 14)),
    "BQSUM": (6, np.int32, (14,)),
    "FRAG": (7, np.int32, (2, 3, 14)),
    "FAM": (8, np.int32, (2, 8, 14)),
    "FAMINFO32": (9, np.int32, (13, 14)),
    "FAMINFO64": (10, np.int64, (2, 14)),
    "DUPLEX": (11, np.int32, (2, 14)),
    "RTR": (12, np.int32, (7,)),
    "BAQ": (13, np.int64, (2,)),
}


def test_the_python_mirror_of_the_groups_is_unchanged():
    from uvc_amd import _ffi
    assert _ffi.FIELD_GROUPS == FIELD_GROUPS_BEFORE
    assert list(_ffi.FIELD_GROUPS) == list(FIELD_GROUPS_BEFORE)   # id order
