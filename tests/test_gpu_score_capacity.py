"""The one-call score (uvcgpu_region_score) at both sides of the rule that sizes its rows per group: min(groups of the request, record
capacity).  One small non-UMI region; the all-out records at a generous capacity are the expectation (held against the oracle here too);
fresh handles -- the device capacity of a handle only grows -- then score at the exact capacity n, at n + 1 and at 4 n (capacity far above
the 2 x positions groups: the rows per group follow the groups), at the default gate with a capacity between its record count and the
groups (the rows per group follow the capacity), and with kept_only.  Every field of every record is equal.  A capacity of n - 1 is
refused with UVCGPU_ENOMEM and n_records = n, and the handle scores as before afterwards."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import compare_records
from util import run_region
from uvc_amd import _ffi, synth

pytestmark = pytest.mark.gpu

REGION = dict(region_len=600, depth=30, seed=21, snv_every=40, somatic_every=130, indel_every=90, variant_inset=100)   # some 11 000 all-out records in 1 596 groups, 18 at the default gate


def score_at(R, capacity, all_out=False, kept_only=False):
    """uvcgpu_region_score into exactly `capacity` columns, without Region.score's retry: (return code, n_records, records or None)."""
    req, _keep = R.make_request(all_out, -1, -1, False, None, None, False, False, 0, kept_only=kept_only)
    buf = np.full((_ffi.NUM_SCORE_FIELDS, capacity), -77, dtype=np.int32)
    out = _ffi.UvcScoreOut(capacity, 0, buf.ctypes.data)
    rc = R.lib.call("score", R.h, C.byref(req), C.byref(out))
    n = int(out.n_records)
    return rc, n, ({name: buf[i, :n].copy() for i, name in enumerate(_ffi.SCORE_FIELDS)} if rc == 0 else None)


def same(got, want, what):
    assert got is not None and len(got["refpos"]) == len(want["refpos"]), (what, None if got is None else len(got["refpos"]), len(want["refpos"]))
    bad = [f for f in want if not np.array_equal(got[f], want[f])]
    assert not bad, (what, bad[:6])


def test_records_do_not_depend_on_the_capacity(oracle_lib, gpu_lib):
    reads = synth.generate_region(**REGION)
    groups = 2 * (reads["end"] - 1 - (reads["beg"] + 1))                   # the default request: [beg + 1, end - 1), two groups per position
    R = run_region(gpu_lib, reads)
    want = {(a, k): R.score(all_out=a, kept_only=k) for a in (False, True) for k in (False, True)}   # generous capacities (Region.score's own)
    R.close()
    Ro = run_region(oracle_lib, reads)
    compare_records(Ro.score(all_out=True), want[True, False])
    Ro.close()
    n, n_gate = len(want[True, False]["refpos"]), len(want[False, False]["refpos"])
    between = (n_gate + groups) // 2
    print("positions", groups // 2, "groups", groups, "records: all-out", n, "kept of them", len(want[True, True]["refpos"]), "default gate", n_gate, "kept of them", len(want[False, True]["refpos"]),
          "capacity between", between)
    assert n > 2 * groups and 0 < n_gate < between < groups                 # the capacities below are on the side of the rule they are meant for
    cases = [("all-out, exact capacity", n, True, False), ("all-out, capacity + 1", n + 1, True, False), ("all-out, 4 x capacity", 4 * n, True, False),
             ("default gate, capacity between its records and the groups", between, False, False),
             ("default gate, kept_only", between, False, True), ("all-out, kept_only, exact capacity", len(want[True, True]["refpos"]), True, True)]
    for what, capacity, all_out, kept_only in cases:
        Rf = run_region(gpu_lib, reads)                                    # a fresh handle: its device capacity is this call's
        rc, n_rec, got = score_at(Rf, capacity, all_out, kept_only)
        assert rc == 0, (what, rc, n_rec)
        same(got, want[all_out, kept_only], what)
        Rf.close()
    # one record too few: refused with the count, nothing else changes
    Rf = run_region(gpu_lib, reads)
    rc, n_rec, got = score_at(Rf, n - 1, True)
    assert rc == _ffi.ENUMS["UVCGPU_ENOMEM"] and n_rec == n and got is None, (rc, n_rec, n)
    rc, n_rec, got = score_at(Rf, n, True)
    assert rc == 0, (rc, n_rec)
    same(got, want[True, False], "after a refused call")
    same(score_at(Rf, between, False)[2], want[False, False], "default gate on the same handle")
    Rf.close()
