"""The internal C interface of libuvcgpu.so is declared once, in headers (uvc_amd/csrc/uvc_launch.h, uvc_host.h, uvc_prep.h, uvc_rtr.h, uvc_rules.h, uvc_planes.h, uvc_score_rows.h, uvc_collectives.h): a source
file that defines a function includes the header that declares it, so the compiler checks the two against each other.  A prototype or a
boundary struct written out again in a .cpp / .hip file is checked by nobody."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "uvc_amd", "csrc")
SOURCES = sorted(glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hip")))
BOUNDARY_STRUCTS = ("RawReads", "UvcProf", "ZeroPlane", "UvcScoreRangeDev", "UvcRangeRow", "UvcUnitSpan", "UvcRangeCursor", "UvcChunkDev",
                    "ScoreRowDesc", "ScoreRows", "ScratchLayout", "SetLayout", "UvcGroup", "SlabLayout")


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


# Loops over shuffle distances (a `for` whose step is `<<= 1` or `>>= 1` around a __shfl_ call) live in uvc_collectives.h, and the segmented
# fold of the reports -- not a scan or reduction of that header's kind -- once in uvc_report_dev.h.  The two that stay in a source file, one
# each, with the shuffle they use: the suffix minimum of uvc_rtr.hip, not of the header's kind either; the butterfly of uvc_coverage.hip costs
# k_coverage registers when it goes through the header (the comment on wave_merge has the numbers).
SHUFFLE_LOOPS_OUTSIDE_THE_HEADER = [("uvc_coverage.hip", "__shfl_xor"), ("uvc_rtr.hip", "__shfl_down")]


def _closing(text, i, open_ch, close_ch):
    """index just behind the bracket that closes the one at text[i]"""
    depth = 0
    for j in range(i, len(text)):
        depth += (text[j] == open_ch) - (text[j] == close_ch)
        if depth == 0:
            return j + 1
    raise AssertionError("unbalanced %s at %d" % (open_ch, i))


def _shuffle_loops(text):
    """the set of __shfl_ calls in the body of every `for` with a shift step"""
    text = re.sub(r"//[^\n]*", "", text)
    found = []
    for m in re.finditer(r"\bfor\s*\(", text):
        head_end = _closing(text, m.end() - 1, "(", ")")
        if not re.search(r"(<<|>>)=\s*1\s*\)$", text[m.end():head_end]):
            continue
        body = text[head_end:]
        while body.lstrip().startswith("#"):   # (#pragma unroll in front of a nested loop)
            body = body.lstrip().split("\n", 1)[1]
        start = len(body) - len(body.lstrip())
        body = body[:_closing(body, start, "{", "}")] if body[start] == "{" else body[:body.index(";") + 1]
        calls = sorted(set(re.findall(r"__shfl_\w*", body)))
        if calls:
            found.append(calls)
    return found


def test_shuffle_loop_finder_sees_both_forms():
    assert _shuffle_loops("for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);  // x") == [["__shfl_xor"]]
    assert _shuffle_loops("for (int o = 1; o < 64; o <<= 1) {\n#pragma unroll\n for (int c = 0; c < 2; c++) { t = __shfl_up(v[c], o); } }") == [["__shfl_up"]]
    assert _shuffle_loops("for (int o = 1; o < 64; o <<= 1) n++;\nx = __shfl_up(m, 1);\nfor (int i = 0; i < 4; i++) y = __shfl(y, i);") == []


def test_loops_over_shuffle_distances_live_in_the_collectives_header():
    found = []
    for path in SOURCES:
        with open(path) as f:
            found += [(os.path.basename(path), call) for calls in _shuffle_loops(f.read()) for call in calls]
    assert sorted(found) == SHUFFLE_LOOPS_OUTSIDE_THE_HEADER, found
    with open(os.path.join(CSRC, "uvc_collectives.h")) as f:
        assert len(_shuffle_loops(f.read())) == 4   # wave_sum, wave_min, wave_max, wave_incl
    with open(os.path.join(CSRC, "uvc_report_dev.h")) as f:
        assert _shuffle_loops(f.read()) == [["__shfl_down"]]   # seg_fold_minmax


# The memory of a region handle has two owners in uvc_host.cpp, Buf (a buffer that grows on demand) and Pool (allocations freed together):
# both wait for the handle's streams before a block goes back.  Outside their definitions the file names no allocation call, and it has no
# switch over the plane groups (include/uvc_field_groups.def is their table).
def _code_of_uvc_host():
    with open(os.path.join(CSRC, "uvc_host.cpp")) as f:
        text = f.read()
    text = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', text)   # string literals (messages name the calls)
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)


def test_allocation_calls_only_inside_the_two_owning_types():
    text = _code_of_uvc_host()
    for owner in ("Buf", "Pool"):
        m = re.search(r"\bstruct %s\s*\{" % owner, text)
        assert m, owner
        text = text[:m.start()] + text[_closing(text, m.end() - 1, "{", "}"):]
    found = re.findall(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|uvc_dev_malloc|uvc_dev_free)\b", text)
    assert not found, found
    assert not re.search(r"#\s*define\s+hip\w+", text)   # (no call under another name)


def test_no_switch_over_the_plane_groups_in_uvc_host():
    text = _code_of_uvc_host()
    bad = []
    for m in re.finditer(r"\bswitch\s*\(", text):
        body_at = text.index("{", _closing(text, m.end() - 1, "(", ")"))
        if "UVC_F_" in text[body_at:_closing(text, body_at, "{", "}")]:
            bad.append(text[m.start():body_at])
    assert not bad, bad
    assert not re.search(r"\bcase\s+UVC_F_", text)
