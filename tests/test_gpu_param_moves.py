"""Every move of the parameter ledger (tests/param_moves.py) on the oracle and on the HIP path with identical parameters: planes bit-exact,
default-gate and all-out records within the classes of test_gpu_parity.compare_records, the InDel allele rows and haplotype links equal,
record lines through test_vcf_text.compare_lines where the move names vcf, and the family assignment of test_group.py for UvcGroupParams
moves.  Eight seeded vectors move about twenty ledger entries of one input at once (parameters that meet in one expression).
The oracle sides run first, on a fixed pool of threads; the GPU side runs serially here, one handle at a time."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import param_moves as pm
from test_gpu_parity import compare_records
from test_vcf_text import REF_SO, _load_ref_vcf, _oracle_lines, compare_lines
from util import diff_groups

pytestmark = pytest.mark.gpu

THREADS = 16
VECTORS = pm.combined_vectors(("plain", "duplex", "normal", "amplicon"), 8, 20, 500)


def _jobs():
    jobs = [("move", name, k) for name, moves in pm.MOVES.items() for k in range(len(moves))]
    return jobs + [("vector", i, None) for i in range(len(VECTORS))]


def _input_and_setting(job):
    kind, a, k = job
    if kind == "vector":
        return VECTORS[a]
    m = pm.MOVES[a][k]
    return m.input, pm.settings(a, m)


def _wants_vcf(job):
    kind, a, k = job
    return kind == "vector" or "vcf" in pm.MOVES[a][k].outputs


@pytest.fixture(scope="module")
def ref_vcf_or_none():
    return _load_ref_vcf() if os.path.exists(REF_SO) else None


@pytest.fixture(scope="module")
def oracle_sides(oracle_lib, ref_vcf_or_none):
    """{job: the oracle's Outputs (packed)} for every move and vector."""
    for inp in pm.INPUTS:
        pm.reads_of(inp)
        if pm.INPUTS[inp].get("tumor"):
            pm.tumor_keys(oracle_lib, inp)

    def one(job):
        inp, setting = _input_and_setting(job)
        vcf = None
        if ref_vcf_or_none is not None and _wants_vcf(job):
            vcf = lambda R, gate, kw: _oracle_lines(oracle_lib, ref_vcf_or_none, R, "chrP", **kw)   # noqa: E731
        return job, pm.run(oracle_lib, oracle_lib, inp, setting, vcf=vcf if vcf else (lambda R, gate, kw: None)).pack()
    with ThreadPoolExecutor(THREADS) as ex:
        return dict(ex.map(one, _jobs()))


def _gpu_vcf(R, gate, kw):
    return R.vcf_records("chrP", gate, tumor_keys=kw.get("tumor_keys")).splitlines()


def _compare(job, oracle_lib, gpu_lib, oracle_sides, ref_vcf):
    inp, setting = _input_and_setting(job)
    o = oracle_sides.pop(job).unpack()
    g = pm.run(gpu_lib, oracle_lib, inp, setting, vcf=_gpu_vcf if (ref_vcf is not None and _wants_vcf(job)) else (lambda R, gate, kw: None))
    if hasattr(o, "families"):
        from test_group import canon
        fo, fg = o.families, g.families
        for k in ("filter_reason", "isize_norm"):
            assert np.array_equal(fo[k], fg[k]), k
        for k in ("n_kept", "n_fams", "n_frags", "ext_beg", "ext_end", "n_amplicon", "n_visited_qnames"):
            assert fo[k] == fg[k], (k, fo[k], fg[k])
        assert canon(fo) == canon(fg)
        assert (np.diff(fg["fam_id"]) >= 0).all() and (np.diff(fg["frag_id"]) >= 0).all()
        return
    bad = diff_groups(o, g)
    assert not bad, "\n".join("%s: %d cells differ, e.g. %s" % (grp, v[0], v[1]) for grp, v in bad.items())
    compare_records(o.gate, g.gate)
    compare_records(o.records, g.records)
    assert o.alleles == g.alleles
    for w in range(3):
        assert o.hap[w] == g.hap[w], (w, next((a, b) for a, b in zip(o.hap[w] + [None], g.hap[w] + [None]) if a != b))
    if ref_vcf is not None and _wants_vcf(job):
        compare_lines(g.vcf, o.vcf)


@pytest.mark.parametrize("name", sorted(pm.MOVES))
def test_move_matches_oracle(name, oracle_lib, gpu_lib, oracle_sides, ref_vcf_or_none):
    for k in range(len(pm.MOVES[name])):
        _compare(("move", name, k), oracle_lib, gpu_lib, oracle_sides, ref_vcf_or_none)


@pytest.mark.parametrize("vector", range(len(VECTORS)))
def test_combined_moves_match_oracle(vector, oracle_lib, gpu_lib, oracle_sides, ref_vcf_or_none):
    assert len(VECTORS[vector][1]) >= 12   # every move of the normal and amplicon inputs, twenty of plain and duplex
    _compare(("vector", vector, None), oracle_lib, gpu_lib, oracle_sides, ref_vcf_or_none)


def test_record_lines_were_compared():
    """The record lines are compared only where oracle/_ref/libref_vcf.so is built (as in test_vcf_text.py): skips without it."""
    _load_ref_vcf()
    assert sum(1 for name, moves in pm.MOVES.items() for m in moves if "vcf" in m.outputs) > 100
