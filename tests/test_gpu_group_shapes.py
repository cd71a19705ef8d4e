"""uvcgpu_group_families against the oracle on the cases of tests/group_cases.py: block edges, scan rounds, the window clamp, every filter
reason, mates on other references, two-strand families, hash collisions and extremes, and the thresholds of k_g_center (the device pow
against the host's).  Everything is exact.  tests/test_group_shapes_cpu.py shows, without a GPU, that each case reaches what it is named
for and that a lost scan carry or a power one ulp off changes the expected result.

center_thresholds-3.0 is the case that found the device pow low against the host's (56 families where the oracle has 60: equalities
(hicnt + 1) == (locnt + 1) * 3^d read as "greater" and snapped); k_g_center has taken its powers from the host since."""
import numpy as np
import pytest

import group_cases as gc
from test_group import structure
from uvc_amd import group

pytestmark = pytest.mark.gpu
SCALARS = ("n_kept", "n_fams", "n_frags", "ext_beg", "ext_end", "n_amplicon", "n_visited_qnames")


def check(ro, rg):
    for k in ("filter_reason", "isize_norm"):
        assert np.array_equal(ro[k], rg[k]), k
    for k in SCALARS:
        assert ro[k] == rg[k], (k, ro[k], rg[k])
    # every family as the exact sequence of (strand, input index) with its two flags, every fragment as its index sequence; structure()
    # asserts the order inside the families (strands, contiguous fragments, file order)
    fams_o, frags_o = structure(ro)
    fams_g, frags_g = structure(rg)
    assert fams_g == fams_o
    assert frags_g == frags_o


@pytest.mark.parametrize("name,sub", gc.ALL, ids=gc.IDS)
def test_gpu_against_oracle(oracle_lib, gpu_lib, name, sub):
    P, cols = gc.params(gpu_lib, name, sub)
    check(gc.reference(oracle_lib, name, sub), group.group_families(gpu_lib, P, cols))


def test_call_again(oracle_lib, gpu_lib):
    """The pool hands back the blocks of the call before, and b2c, e2c, fam_dflag and fam_idflag are not zero-filled: a large input, the
    smallest, the large one again.  Each result equals the oracle's and the two large ones are the same arrays."""
    runs = []
    for name, sub in (("duplex_families", "mixed"), ("sizes", 1), ("duplex_families", "mixed")):
        runs.append(group.group_families(gpu_lib, *gc.params(gpu_lib, name, sub)))
        check(gc.reference(oracle_lib, name, sub), runs[-1])
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[2][k]), k
