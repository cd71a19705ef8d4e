"""P2: GenericSymbol2CountCoverage::updateByAln<., SYMBOL_COUNT_SUM, true> (main.hpp:1762-2296) with dealwith_segbias.
The oracle's SEG32 / SEG64 planes, the four a1BQ / a2BQ sums of the VQ group and the SYMBOL_COUNT_SUM plane against independent Python
restatements written from the reference text, chained without the oracle in between: repeat tracks and BAQ sums (tests/rtr_cases.py) ->
P1 counters and P1b thresholds (tests/prep_restatement.py) -> the per-read CIGAR walk (tests/p2_restatement.py) calling dealwith_segbias
(tests/segbias_restatement.py).  Reads of the fuzz generator: several InDels per read, insertions next to deletions, InDels at read ends,
clips, reference skips, N bases; Illumina and IonTorrent arms, UMI / amplicon families, the normal-sample arm."""
import importlib.util
import os

import numpy as np
import pytest

from uvc_amd import region
from rtr_cases import python_tracks
from prep_restatement import prep_sets, thres_sets
from p2_restatement import update_by_aln
from segbias_restatement import SEG_FIELDS
from byte_classes import IONTORRENT_NEGATIVE, NEGATIVE_MISMA, set_params, zero_value_cells
from util import run_region

_spec = importlib.util.spec_from_file_location("fz_p2", os.path.join(os.path.dirname(__file__), "test_gpu_fuzz.py"))
fz = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(fz)

SEG32 = SEG_FIELDS[:30]; SEG64 = SEG_FIELDS[30:34]; VQ4 = SEG_FIELDS[34:38]


@pytest.mark.parametrize("seed,umi,platform,normal", [(21, False, 1, 0), (22, True, 1, 0), (23, False, 2, 0), (24, False, 1, 1), (25, True, 2, 0), (26, False, 1, 0)])
def test_updateByAln_against_the_independent_restatements(seed, umi, platform, normal, oracle_lib):
    check(oracle_lib, seed, umi, platform, normal)


@pytest.mark.parametrize("seed,umi,platform,quals_from,values", [(27, True, 1, fz.WIDE_QUALS, None), (28, False, 1, fz.QUALS, NEGATIVE_MISMA), (29, True, 2, fz.QUALS, IONTORRENT_NEGATIVE)])
def test_updateByAln_on_the_quality_byte_classes(seed, umi, platform, quals_from, values, oracle_lib):
    """Qualities of 0 and of 0x7F .. 0xFF, bq_phred_added_misma = -20, and IonTorrent with bq_phred_added_indel < bq_phred_added_misma < 0
    (tests/byte_classes.py).  Each arm has (fragment, position) pairs whose consensus counts add up to 0, counted from the restated walk: 539, 4366 and 1418; the two arms with a negative addend hold 5570 and 2864 aligned bases of a value below 0."""
    n, below = check(oracle_lib, seed, umi, platform, 0, quals_from, values)
    print("zero-value cells:", n, "values below 0:", below)
    assert n > 0 and (below > 0) == (values is not None)     # a negative addend gives values below 0, a quality byte alone never does


def check(oracle_lib, seed, umi, platform, normal, quals_from=fz.QUALS, values=None):
    reads = fz.weird_region(seed, n_frag=120 + 30 * (seed % 3), ref_len=420 + 30 * seed, umi=umi, quals_from=quals_from)
    P = set_params(region.default_params(oracle_lib, platform=platform), values)
    P.tumor_vcf_is_provided = normal
    R = run_region(oracle_lib, reads, params=P)
    rtr, baq = python_tracks(reads["refseq"], smax=P.indel_str_repeatsize_max, vmax=P.indel_vntr_repeatsize_max, bq_max=P.indel_BQ_max,
                             slip_rate=P.indel_polymerase_slip_rate, del_to_ins=P.indel_del_to_ins_err_ratio, polymerase_size=P.indel_polymerase_size,
                             str_phred_per_region=P.indel_str_phred_per_region, nonstr_phred_per_base=P.indel_nonSTR_phred_per_base)
    codes = np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(c.upper(), 4) for c in reads["refseq"]], dtype=np.int32)
    prep = prep_sets(reads, P, rtr, baq[0], np.append(codes, 4))
    thres, ip = thres_sets(prep, rtr[3], P, is_normal=bool(normal), iontorrent=(platform == 2))
    seg, bqsum = update_by_aln(reads, P, rtr, ip, baq[0], baq[1], codes, prep, thres, proton=(platform == 2))
    o32, o64, ovq, obq = R.fetch("SEG32"), R.fetch("SEG64"), R.fetch("VQ"), R.fetch("BQSUM")
    bad = {}
    for k, name in enumerate(SEG32):
        if not np.array_equal(o32[k].astype(np.int64), seg[name]): bad[name] = np.argwhere(o32[k] != seg[name])[:4].tolist()
    for k, name in enumerate(SEG64):
        if not np.array_equal(o64[k].astype(np.int64), seg[name]): bad[name] = np.argwhere(o64[k] != seg[name])[:4].tolist()
    for k, name in enumerate(VQ4):
        if not np.array_equal(ovq[k].astype(np.int64), seg[name]): bad[name] = np.argwhere(ovq[k] != seg[name])[:4].tolist()
    if not np.array_equal(obq.astype(np.int64), bqsum): bad["BQSUM"] = np.argwhere(obq != bqsum)[:4].tolist()
    assert not bad, bad
    assert obq[7:13].sum() > 0 and obq[5].sum() > 0 and obq[13].sum() > 0          # InDel symbols and both padded-deletion symbols occur
    R.close()
    return zero_value_cells(reads, P, rtr, ip, baq[0], codes, prep, thres, platform == 2) if values or quals_from is not fz.QUALS else None
