"""The inputs of tests/test_gpu_misq.py reach the edges they are named after, and the restatement of the mismatch queue (misq_cases.items)
counts what the oracle counts: no GPU here.

The oracle has no queue; what it has per (symbol, position) is the depth aDPff + aDPfr + aDPrf + aDPrr of SEG32, one per M-op base of every
read.  misq_cases.pileup makes the same table from the read columns, and on the cells of a symbol that differs from the reference it is
the number of mismatching bases there -- the items of the work-list entries plus the mismatching bases of the reads that are not on the
list (kind 1), which the restatement keeps apart by edge_reads.classify."""
import numpy as np
import pytest

import misq_cases as mc
from uvc_amd import _ffi, region
from util import run_region

E = _ffi.ENUMS


def oracle_depths(oracle_lib, reads, platform=1):
    R = run_region(oracle_lib, reads, platform=platform)
    seg, bqsum = R.fetch("SEG32"), R.fetch("BQSUM")
    R.close()
    return (seg[E["UVC_S_aDPff"]] + seg[E["UVC_S_aDPfr"]] + seg[E["UVC_S_aDPrf"]] + seg[E["UVC_S_aDPrr"]])[:5].astype(np.int64), bqsum[:5].astype(np.int64)


def check_against_oracle(oracle_lib, reads):
    """Every mismatching M-op base is one unit of the oracle's depth of its symbol, and no other cell of a non-reference symbol is set; the
    items plus the mismatching bases of the kind-1 reads are all of them; where no read is of kind 1, the values of the items add up to
    the oracle's BQSUM of those cells."""
    ad, bqsum = oracle_depths(oracle_lib, reads)
    ref = mc.ref_codes(reads)
    off_ref = np.arange(5)[:, None] != ref[None, :]
    assert np.array_equal(ad * off_ref, mc.pileup(reads) * off_ref)
    rows, _ = mc.items(reads, added_misma=region.default_params(oracle_lib).bq_phred_added_misma)
    kd = mc.kinds(reads)
    n_kind1 = sum(len(mc.mismatches(reads, k, ref)[0]) for k in np.nonzero(kd == 1)[0])
    assert len(rows) + n_kind1 == int((ad * off_ref).sum())
    if not (kd == 1).any():
        want = np.zeros_like(bqsum)
        for _, epos, symval in rows:
            want[symval & 0xFF, epos - reads["beg"]] += symval >> 8
        assert np.array_equal(bqsum * off_ref, want)
    return rows


@pytest.mark.parametrize("npos", mc.REGION_LENGTHS)
def test_boundary_inputs_have_items_on_the_named_indices(npos, oracle_lib):
    case = mc.boundary(npos)
    reads = case["reads"]
    assert reads["end"] - reads["beg"] + 1 == npos
    last = npos - 3   # the last plane index a read may cover (misq_cases)
    rows = check_against_oracle(oracle_lib, reads)
    at = {(k, epos - reads["beg"]) for k, epos, _ in rows}
    xs = {x for _, x in at}
    want = [x for x in (0, 63, 64, 1023, 1024) if x <= last] + [last]
    assert case["planted"] == sorted(set(want)) and all(x in xs for x in want), (want, case["planted"])
    # a read that begins on the region's first position and one that ends on the last position a read may cover, each with an item there
    assert reads["pos"][case["first_read"]] == reads["beg"] and (case["first_read"], 0) in at
    k = case["last_read"]
    assert mc.m_bases(reads, k)[1][-1] == last and (k, last) in at
    # a partial last tile, or a region that ends on a tile's edge
    assert (npos % mc.PSCAN_TILE != 0) == (npos != 1024)
    # a read across a tile boundary with items on both sides (only a region of more than one tile and a half has room for it)
    assert (len(case["spanning"]) > 0) == (npos == 2049)
    for k in case["spanning"]:
        mine = sorted(x for kk, x in at if kk == k)
        assert 1023 in mine and 1024 in mine and mine[0] < 1023 and mine[-1] > 1024
    # InDel reads on the work list (kind 2) and off it (kind 1), the former with items next to the InDel and far from it
    kd = mc.kinds(reads)
    on_list = [k for k in case["indel_reads"] if kd[k] == 2]
    assert len(on_list) >= 3 and any(kd[k] == 1 for k in case["indel_reads"]) and all(kd[k] == 0 for k in range(reads["n_reads"]) if k not in case["indel_reads"])
    for k in on_list:
        xi, run = mc.m_bases(reads, k)[1], mc.m_bases(reads, k)[2]
        assert (k, int(xi[run == 0][-1])) in at and (k, int(xi[-1]) - 3) in at
    assert not any(kk in set(np.nonzero(kd == 1)[0]) for kk, _ in at)
    assert mc.demoted_mismatches(reads) >= 2   # (each of them has its two planted mismatches)


def test_overflow_input_fills_the_lds_queue_in_one_round(oracle_lib):
    reads = mc.overflow()
    assert reads["end"] - reads["beg"] + 1 == mc.PSCAN_TILE
    check_against_oracle(oracle_lib, reads)
    per_entry = mc.scan_rounds(reads)
    # every entry lies in the one tile and has at least two mismatches: any PSCAN_ROUND entries hold more than PSCAN_QCAP
    assert len(per_entry) == reads["n_reads"] > mc.PSCAN_ROUND and per_entry.min() >= 2
    assert mc.PSCAN_ROUND * int(per_entry.min()) > mc.PSCAN_QCAP
    assert np.sort(per_entry)[:mc.PSCAN_ROUND].sum() > mc.PSCAN_QCAP
    assert mc.demoted_mismatches(reads) == 0   # every read is a simple alignment: the device's count is the count set_reads made


def test_empty_input_has_no_item(oracle_lib):
    reads = mc.empty()
    rows = check_against_oracle(oracle_lib, reads)
    assert rows == [] and (mc.kinds(reads) == 2).any()


def test_n_input(oracle_lib):
    case = mc.with_n()
    reads = case["reads"]
    rows = check_against_oracle(oracle_lib, reads)
    at = {(k, epos - reads["beg"]): symval & 0xFF for k, epos, symval in rows}
    assert len(case["read_n"]) >= 6 and all(at.get(kx) == 4 for kx in case["read_n"])          # N over a base of the reference: an item of symbol N
    assert len(case["ref_n_read_n"]) >= 4 and not any(kx in at for kx in case["ref_n_read_n"])   # N under N: no item
    assert len(case["ref_n_read_base"]) >= 6 and all(at.get(kx, 9) < 4 for kx in case["ref_n_read_base"])   # a base over N: an item of that base


def test_quality_byte_input(oracle_lib):
    case = mc.quality_bytes()
    reads = case["reads"]
    rows = check_against_oracle(oracle_lib, reads)
    val = {(k, epos - reads["beg"]): symval >> 8 for k, epos, symval in rows}
    kd = mc.kinds(reads)
    seen = set()
    for k, x, qv in case["planted"]:
        assert kd[k] != 1 and val[(k, x)] == qv
        seen.add((qv, bool(kd[k] == 2)))
    assert {q for q, _ in seen} == set(mc.QUALITY_BYTES) and {q for q, m in seen if m} >= {93, 128, 255}
