"""P1 and P2 walk ONE work list (RegionDev::frec2, four class sub-lists sorted by begin): k_prep_sums / k_prep_fast skip the entries that are not
a whole simple alignment.  Every case: all 14 plane groups bit-exact against the oracle, no presence violation, and the default-gate records
within the classes of test_gpu_parity.compare_records.  The shapes are the smallest that still have several windows, empty windows, empty
sub-lists, lists with nothing for P1, and a handle that is used again."""
import numpy as np
import pytest

from uvc_amd import region, synth
import prep_unit_cases
from test_bq_correction import corrected
from test_gpu_parity import compare_records
from util import INT_GROUPS, diff_groups, presence_violations, run_region

pytestmark = pytest.mark.gpu

CASE1 = dict(seed=31, region_len=3000, depth=40, indel_every=500)   # 800 reads, classes of 176 / 176 / 224 / 224 alignments, 57 InDel reads, 46 windows (one empty)
CASE2 = dict(seed=32, region_len=3000, depth=40, indel_every=0)     # 200 per class, 8 multi-op CIGARs
CASE5 = dict(seed=33, region_len=1000, depth=4, indel_every=300)    # 26 reads, 3 empty windows of 15
M, I, D, S = 0, 1, 2, 4
ENOREADS = -1   # UVCGPU_ENOREADS

_oracle_runs = {}


def oracle_run(oracle_lib, key, make):
    """The oracle's handle of a case, computed once and shared (never changed) by the tests that need it."""
    if key not in _oracle_runs:
        reads = make()
        Ro = run_region(oracle_lib, reads)
        _oracle_runs[key] = (reads, Ro, Ro.score())
    return _oracle_runs[key]


def check(Ro, ro, Rg, what=""):
    assert len(INT_GROUPS) == 14
    bad = diff_groups(Ro, Rg)
    assert not bad, what + "\n".join("%s: %d cells differ, e.g. %s" % (g, v[0], v[1]) for g, v in bad.items())
    assert presence_violations(Rg) == 0, what
    return compare_records(ro, Rg.score())


def unpaired(specs, n_ref=400, beg=7_000_000, seed=8):
    """Unpaired reads, one per fragment and family: specs = [(start, flag, [(op, len) ...])]; the bases follow the reference (0.4 % errors,
    inserted bases at random)."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, n_ref)
    n = len(specs)
    pos, flag, lq, so, co, nc, bases, cig = [], [], [], [], [], [], [], []
    for start, fl, cg in specs:
        r, b = start, []
        for op, ln in cg:
            if op == M:
                b += list(ref[r:r + ln]); r += ln
            elif op == D:
                r += ln
            else:
                b += list(rng.integers(0, 4, ln))
        assert r <= n_ref
        pos.append(beg + start); flag.append(fl); lq.append(len(b)); so.append(len(bases)); co.append(len(cig)); nc.append(len(cg))
        bases += b; cig += [(ln << 4) | op for op, ln in cg]
    bases = np.array(bases, np.int64)
    bases = np.where(rng.random(len(bases)) < 0.004, rng.integers(0, 4, len(bases)), bases).astype(np.uint8)
    flag = np.array(flag, np.uint16)
    return dict(n_reads=n, pos=np.array(pos, np.int32), mpos=np.full(n, -1, np.int32), isize=np.zeros(n, np.int32), flag=flag, mapq=np.full(n, 60, np.uint8),
                nm=np.full(n, -1, np.int32), l_qseq=np.array(lq, np.int32), seq_off=np.array(so, np.int64), cigar_off=np.array(co, np.int64), n_cigar=np.array(nc, np.int32),
                frag_id=np.arange(n, dtype=np.int32), fam_id=np.arange(n, dtype=np.int32), fam_strand=((flag & 16) != 0).astype(np.uint8), n_fams=n, fam_dflag=np.zeros(n, np.uint8),
                bases=bases, quals=rng.choice([12, 30, 37], len(bases)).astype(np.uint8), cigars=np.array(cig, np.uint32), tid=1, beg=beg, end=beg + n_ref,
                refseq="".join("ACGT"[b] for b in ref))


def forward_stack(alternate):
    rng = np.random.default_rng(5)
    starts = np.sort(rng.integers(20, 320, 300))
    return unpaired([(int(s), (16 if (alternate and k % 2) else 0), [(M, 60)]) for k, s in enumerate(starts)])


def indel_only(leading_insertion=False):
    rng = np.random.default_rng(6)
    shapes = [[(M, 30), (D, 2), (M, 30)], [(M, 30), (I, 2), (M, 28)], [(S, 5), (M, 20), (D, 1), (M, 35)], [(M, 10), (I, 1), (M, 20), (D, 3), (M, 29)]]
    if leading_insertion:   # one M run that spans the whole alignment, yet no simple alignment: P1 must leave it to the per-read kernel
        shapes += [[(I, 2), (M, 58)], [(M, 58), (I, 2)], [(S, 3), (I, 2), (M, 55)]]
    starts = np.sort(rng.integers(20, 310, 240))
    return unpaired([(int(s), 16 * (k % 2), shapes[k % len(shapes)]) for k, s in enumerate(starts)], seed=9)


@pytest.mark.parametrize("split", [None, "1"])
@pytest.mark.parametrize("case", ["case1", "case2"])
def test_paired_reads_with_and_without_indel_reads(case, split, oracle_lib, gpu_lib, monkeypatch):
    """Four class sub-lists with InDel reads interleaved (case 1) and without (case 2), by the wave form and by the split form of k_prep_fast."""
    if split:
        monkeypatch.setenv("UVCGPU_SPLIT", split)
    else:
        monkeypatch.delenv("UVCGPU_SPLIT", raising=False)
    reads, Ro, ro = oracle_run(oracle_lib, case, lambda: synth.generate_region(**(CASE1 if case == "case1" else CASE2)))
    if case == "case1":
        assert reads["n_reads"] == 800 and (reads["n_cigar"] > 1).sum() >= 57
    Rg = run_region(gpu_lib, reads)
    check(Ro, ro, Rg)
    Rg.close()


@pytest.mark.parametrize("alternate", [False, True])
def test_unpaired_reads_leave_sub_lists_empty(alternate, oracle_lib, gpu_lib):
    """Flag 0 throughout: only class 0 has entries; flags 0 / 16 in turn: classes 0 and 3."""
    reads = forward_stack(alternate)
    Ro = run_region(oracle_lib, reads)
    Rg = run_region(gpu_lib, reads)
    check(Ro, Ro.score(), Rg)
    assert Rg.fetch("PREP32").any()


@pytest.mark.parametrize("leading_insertion", [False, True])
def test_every_read_has_an_indel(leading_insertion, oracle_lib, gpu_lib):
    """No simple alignment at all: the lists P1 walks hold only entries it must skip."""
    reads = indel_only(leading_insertion)
    assert (reads["n_cigar"] > 1).all()
    Ro = run_region(oracle_lib, reads)
    Rg = run_region(gpu_lib, reads)
    check(Ro, Ro.score(), Rg)


def test_sparse_region_and_no_reads(oracle_lib, gpu_lib):
    """26 reads over 15 windows, three of them empty; then no reads at all on the same handle (refused by accumulate, as by the reference),
    and the sparse reads again."""
    reads, Ro, ro = oracle_run(oracle_lib, "case5", lambda: synth.generate_region(**CASE5))
    assert reads["n_reads"] == 26
    Rg = run_region(gpu_lib, reads)
    check(Ro, ro, Rg)
    empty = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in reads.items()}
    empty.update(n_reads=0, n_fams=0)
    Re = region.Region(oracle_lib, region.default_params(oracle_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    for R in (Re, Rg):
        R.set_reads(empty)
        with pytest.raises(region.UvcError) as e:
            R.accumulate()
        assert e.value.code == ENOREADS, e.value
    Rg.set_reads(reads)
    Rg.accumulate()
    check(Ro, ro, Rg)
    Rg.close()


def test_one_handle_used_again(oracle_lib, gpu_lib):
    """Case 1, reset to case 5, back to case 1 on one handle: every result equals a fresh handle's (a counter that was not zeroed again -- the
    mismatch queue, the overflow list, the InDel allele counters, the error words of the preparation -- or a slot of the previous list would
    carry over)."""
    one = oracle_run(oracle_lib, "case1", lambda: synth.generate_region(**CASE1))
    five = oracle_run(oracle_lib, "case5", lambda: synth.generate_region(**CASE5))
    R = None
    for k, (reads, Ro, ro) in enumerate((one, five, one)):
        fresh = run_region(gpu_lib, reads)
        if R is None:
            R = region.Region(gpu_lib, region.default_params(gpu_lib), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        else:
            R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        R.set_reads(reads)
        R.accumulate()
        check(Ro, ro, R, "use %d: " % k)
        assert not diff_groups(fresh, R), k
        rf, rr = fresh.score(), R.score()
        assert all(np.array_equal(rf[f], rr[f]) for f in rf), k
        assert fresh.indel_alleles() == R.indel_alleles(), k
        fresh.close()
    R.close()


def test_correct_bq_rebuilds_the_work_list(oracle_lib, gpu_lib):
    """uvcgpu_region_correct_bq runs the prelude and the list build again on the same slots (an InDel read can change sides of the
    low-quality-InDel test): planes and records against the oracle's corrected run."""
    reads = synth.generate_region(**CASE1)
    Ro, qo = corrected(oracle_lib, reads, 37, 2, accumulate=True)
    Rg, qg = corrected(gpu_lib, reads, 37, 2, accumulate=True)
    assert np.array_equal(qo, qg)
    check(Ro, Ro.score(), Rg)


@pytest.mark.parametrize("arm", ["default", "iontorrent"])
def test_preparation_edges_through_the_handle(arm, oracle_lib, gpu_lib):
    """The `nesting` reads of tests/test_gpu_prep_units.py (every CIGAR shape, fragment and unit heads on the thread, wave and tile edges of the
    preparation's scans, a read without a reference-consuming op, one without bases) through set_reads and accumulate: the direct test pins
    the preparation's outputs, this one what the accumulate kernels make of them.  IonTorrent: no InDel read on the work list."""
    case = prep_unit_cases.nesting(arm)
    reads = prep_unit_cases.handle_reads(case)
    Ro = run_region(oracle_lib, reads, platform=case["platform"])
    Rg = run_region(gpu_lib, reads, platform=case["platform"])
    check(Ro, Ro.score(), Rg, arm + ": ")
    Rg.close()
