"""The haplotype links of the HIP path (k_hap_cand / k_hap_frags / k_hap_units, then uvc_hap.cpp) against the oracle on the planted cases of
tests/hap_cases.py and the moved parameters on `nested`; tests/test_hap_cpu.py holds the oracle against the independent restatement on the
same inputs and asserts that every case is what it claims to be.  Every cell: the three link vectors equal, the bHap / cHap / c2Hap values of
every written VCF record equal, and the handle's error state clean afterwards (no UVCGPU_EDEVICE from an event slot that was too small)."""
import pytest

import hap_cases as hc
from hap_cases import oracle_tags, params_of, product_tags
from util import run_region

pytestmark = pytest.mark.gpu

CELLS = [(name, None) for name in hc.CASES] + [("nested", move) for move in hc.NESTED_MOVES]


@pytest.mark.parametrize("case,move", CELLS, ids=[c if m is None else "%s-%s=%d" % (c, m[0], m[1]) for c, m in CELLS])
def test_links_and_tags_match_the_oracle(case, move, oracle_lib, gpu_lib):
    c = hc.CASES[case]()
    reads, platform = c["reads"], c["platform"]
    setting = {move[0]: move[1]} if move else {}
    Ro = run_region(oracle_lib, reads, params=params_of(oracle_lib, platform, setting))
    Rg = run_region(gpu_lib, reads, params=params_of(gpu_lib, platform, setting))
    try:
        lo, lg = Ro.hap_links(), Rg.hap_links()                  # raises on a device-side error
        if setting.get("phasing_haplotype_max_count") != 0:
            assert sum(len(l) for l in lo) >= 2, [len(l) for l in lo]
        for w, name in enumerate(("bq", "fq", "f2q")):
            assert lo[w] == lg[w], (name, next((a, b) for a, b in zip(lo[w] + [None], lg[w] + [None]) if a != b))
        want, mine = oracle_tags(Ro), product_tags(Rg)
        assert sorted(want) == sorted(mine)
        for key in want:
            assert mine[key] == want[key], (key, mine[key], want[key])
        if setting.get("phasing_haplotype_max_count") != 0:
            assert sum(1 for v in want.values() if any(v)) >= 2
        Rg.fetch("PREP32")                                       # surfaces the device-side error flag once more after the link kernels
    finally:
        Ro.close(); Rg.close()
