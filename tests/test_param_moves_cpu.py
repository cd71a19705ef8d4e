"""The parameter ledger (tests/param_moves.py) on the oracle alone: it names every parameter, every move changes what it says it changes,
and the oracle's scoring agrees with the independent restatement (tests/score_restatement.py) at moved values."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import param_moves as pm
from uvc_amd import region

THREADS = 16   # ctypes releases the GIL inside the oracle; a fixed pool, whatever the host's core count


def test_ledger_names_every_parameter_once():
    params, groups = pm.def_names()
    names = set(params) | set(groups)
    # the parser sees what the ctypes mirrors of the two structs hold (less their padding / size fields)
    from uvc_amd import _ffi, group
    assert set(params) == {f for f, _ in _ffi.UvcParams._fields_} - {"struct_size", "reserved_", "pad_to_8_"}
    assert set(groups) == {"group." + f for f, _ in group.UvcGroupParams._fields_} - {"group.struct_size", "group.pad_"}
    assert not set(pm.MOVES) & set(pm.EXEMPT), set(pm.MOVES) & set(pm.EXEMPT)
    assert set(pm.MOVES) | set(pm.EXEMPT) == names, (sorted(names - set(pm.MOVES) - set(pm.EXEMPT)), sorted((set(pm.MOVES) | set(pm.EXEMPT)) - names))
    assert len(pm.EXEMPT) < 10 and all(isinstance(r, str) and len(r) > 20 for r in pm.EXEMPT.values())


def test_def_names_follow_the_files(tmp_path, monkeypatch):
    """A row added to a .def file (or a hand-declared UvcGroupParams field) is a name the ledger must then carry."""
    root = pm.ROOT
    for rel, row in (("uvc_params.def", "UVC_PI(new_threshold, 3)\n"), ("uvc_group_params.def", "UVC_GD(new_ratio, 0.5)\n")):
        inc = tmp_path / rel.replace(".def", "") / "include"
        inc.mkdir(parents=True)
        for f in ("uvc_params.def", "uvc_group_params.def", "uvcgroup.h"):
            text = open(os.path.join(root, "include", f)).read()
            (inc / f).write_text(text + row if f == rel else text)
        monkeypatch.setattr(pm, "ROOT", str(inc.parent))
        params, groups = pm.def_names()
        new = (set(params) | set(groups)) - set(pm.MOVES) - set(pm.EXEMPT)
        assert new == {"new_threshold" if rel == "uvc_params.def" else "group.new_ratio"}, new


def test_moves_are_well_formed(oracle_lib):
    params, groups = pm.def_names()
    types = dict(params, **groups)
    for name, moves in pm.MOVES.items():
        assert moves, name
        for m in moves:
            assert m.input in pm.INPUTS and set(m.outputs) <= set(pm.OUTPUTS) and m.outputs, (name, m)
            assert ("alignments" in pm.INPUTS[m.input]) == pm.is_group(name), (name, m.input)
            assert type(m.value) is types[name], (name, m.value)                      # an int field gets an int, a double field a float
            at_default = pm.make_params(oracle_lib, m.input, m.companions)
            field = name[len("group."):] if pm.is_group(name) else name
            assert m.value != getattr(at_default, field), (name, m.value)
            ok = pm.make_params(oracle_lib, m.input, pm.settings(name, m))
            if not pm.is_group(name):    # what uvcgpu_region_create accepts (uvc_host.cpp:291-296)
                assert 1 <= ok.indel_str_repeatsize_max <= ok.indel_vntr_repeatsize_max <= 255 and 1 <= ok.indel_BQ_max <= 32767, (name, m)
                assert ok.bias_thres_interfering_indel <= 10000, (name, m)


def _changes(oracle_lib):
    """{(param, k): the outputs move k of param changed}, every run on a fixed pool; each move against the run of its input with its companions."""
    jobs = [(name, k, m) for name, moves in pm.MOVES.items() for k, m in enumerate(moves)]
    for inp in pm.INPUTS:
        pm.reads_of(inp)
        if pm.INPUTS[inp].get("tumor"):
            pm.tumor_keys(oracle_lib, inp)
    bases = {(m.input, tuple(sorted(m.companions.items()))) for _, _, m in jobs}
    with ThreadPoolExecutor(THREADS) as ex:
        base = dict(zip(bases, ex.map(lambda b: pm.run(oracle_lib, oracle_lib, b[0], dict(b[1])), bases)))

        def one(job):
            name, k, m = job
            moved = pm.run(oracle_lib, oracle_lib, m.input, pm.settings(name, m))
            return (name, k), pm.changed(base[(m.input, tuple(sorted(m.companions.items())))], moved)
        return dict(ex.map(one, jobs))


@pytest.fixture(scope="module")
def changes(oracle_lib):
    return _changes(oracle_lib)


@pytest.mark.parametrize("name", sorted(pm.MOVES))
def test_every_move_changes_what_it_names(name, changes):
    for k, m in enumerate(pm.MOVES[name]):
        got = changes[(name, k)]
        assert set(m.outputs) <= got, (name, m, "changed only", sorted(got))


# ---- the oracle against the independent restatement at moved values ----
def _restated_params():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "score_restatement.py")).read()
    return set(re.findall(r"\bP\.(\w+)", src))


@pytest.mark.parametrize("vector", range(4))
def test_oracle_scoring_against_the_restatement_at_moved_values(vector, oracle_lib):
    from test_score_cpu import check
    inp, setting = pm.combined_vectors(("plain", "duplex"), 4, 20, 100, only=_restated_params())[vector]
    assert len(setting) >= 20
    P = pm.make_params(oracle_lib, inp, setting)
    R = region.Region(oracle_lib, P, *pm._region_args(pm.reads_of(inp)))
    R.set_reads(pm.reads_of(inp))
    R.accumulate()
    assert check(oracle_lib, R, P, all_out=True) > 10000
    R.close()
