"""The internal C interface of libuvcgpu.so is declared once, in headers (uvc_amd/csrc/uvc_launch.h, uvc_host.h, uvc_prep.h, uvc_rtr.h, uvc_rules.h, uvc_score_rows.h): a source
file that defines a function includes the header that declares it, so the compiler checks the two against each other.  A prototype or a
boundary struct written out again in a .cpp / .hip file is checked by nobody."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "uvc_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hip")))
BOUNDARY_STRUCTS = ("RawReads", "UvcProf", "ZeroPlane", "UvcScoreRangeDev", "UvcRangeRow", "UvcUnitSpan", "UvcRangeCursor", "UvcChunkDev",
                    "ScoreRowDesc", "ScoreRows", "ScratchLayout", "SetLayout")


def _lines():
    assert len(SOURCES) >= 15, SOURCES
    for path in SOURCES:
        with open(path) as f:
            for no, line in enumerate(f, 1):
                yield "%s:%d" % (os.path.basename(path), no), line.rstrip("\n")


def test_no_extern_c_prototype_in_a_source_file():
    bad = [at for at, line in _lines() if line.startswith('extern "C"') and line.split("//")[0].rstrip().endswith(";")]   # (a trailing comment aside)
    assert not bad, bad


def test_boundary_structs_are_defined_in_headers_only():
    pat = re.compile(r"^struct\s+(%s)\b" % "|".join(BOUNDARY_STRUCTS))
    bad = [at for at, line in _lines() if pat.match(line)]
    assert not bad, bad
