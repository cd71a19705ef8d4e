"""Preconditions of tests/test_gpu_edge_reads.py, without a GPU: every hand-placed read of tests/edge_reads.py is on the intended side of the
guard it is meant to straddle (restated there in plain Python), the oracle accepts every input, counts the clip cells and returns the
haplotype links the comparison is about, and the independent restatements (prep_, p2_, p3_restatement) agree with the oracle on the
clip and penalty inputs, so that the comparison does not rest on the oracle alone."""
import numpy as np
import pytest

from uvc_amd import region
import edge_reads as er
from edge_reads import D, I, M, N
from p2_restatement import update_by_aln
from p3_restatement import fragment_pass
from prep_restatement import PREP32, PREP64, prep_sets, thres_sets
from rtr_cases import python_tracks
from segbias_restatement import SEG_FIELDS
from util import run_region

LONG_CLIP, PCR_CLIP = PREP32.index("a_near_long_clip_dp"), PREP32.index("a_near_pcr_clip_dp")


def restatements_agree(oracle_lib, reads, R, with_p2):
    """prep_sets (every PREP32 / PREP64 counter) and, with_p2, update_by_aln (SEG32, SEG64, the four BQ sums of VQ, BQSUM) and fragment_pass
    (FRAG bDP / bTA / bTB, four VQ slots) against the oracle's handle R."""
    P = region.default_params(oracle_lib)
    rtr, baq = python_tracks(reads["refseq"], smax=P.indel_str_repeatsize_max, vmax=P.indel_vntr_repeatsize_max, bq_max=P.indel_BQ_max,
                             slip_rate=P.indel_polymerase_slip_rate, del_to_ins=P.indel_del_to_ins_err_ratio, polymerase_size=P.indel_polymerase_size,
                             str_phred_per_region=P.indel_str_phred_per_region, nonstr_phred_per_base=P.indel_nonSTR_phred_per_base)
    codes = np.array([{"A": 0, "C": 1, "G": 2, "T": 3}.get(c.upper(), 4) for c in reads["refseq"]], dtype=np.int32)
    want = prep_sets(reads, P, rtr, baq[0], np.append(codes, 4))
    got32, got64 = R.fetch("PREP32"), R.fetch("PREP64")
    bad = {}
    for k, name in enumerate(PREP32):
        w = ((want[name].astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31
        if not np.array_equal(got32[k].astype(np.int64), w): bad[name] = np.nonzero(got32[k] != w)[0][:5].tolist()
    for k, name in enumerate(PREP64):
        if not np.array_equal(got64[k].astype(np.int64), want[name]): bad[name] = np.nonzero(got64[k] != want[name])[0][:5].tolist()
    assert not bad, bad
    if with_p2:
        thres, ip = thres_sets(want, rtr[3], P, is_normal=False, iontorrent=False)
        seg, bqsum = update_by_aln(reads, P, rtr, ip, baq[0], baq[1], codes, want, thres, proton=False)
        planes = [(R.fetch("SEG32"), SEG_FIELDS[:30]), (R.fetch("SEG64"), SEG_FIELDS[30:34]), (R.fetch("VQ"), SEG_FIELDS[34:38])]
        for got, names in planes:
            for k, name in enumerate(names):
                if not np.array_equal(got[k].astype(np.int64), seg[name]): bad[name] = np.argwhere(got[k] != seg[name])[:4].tolist()
        if not np.array_equal(R.fetch("BQSUM").astype(np.int64), bqsum): bad["BQSUM"] = np.argwhere(R.fetch("BQSUM") != bqsum)[:4].tolist()
        frag, vq = fragment_pass(reads, P, rtr, ip, baq[0], codes, want, thres, seg, bqsum, False)
        of, ov = R.fetch("FRAG"), R.fetch("VQ")
        for st in range(2):
            for f, name in enumerate(("bDP", "bTA", "bTB")):
                if not np.array_equal(of[st][f].astype(np.int64), frag[st][f]): bad["%s[%d]" % (name, st)] = np.argwhere(of[st][f] != frag[st][f])[:4].tolist()
        for k, name in ((4, "bMQ"), (5, "bIAQb"), (6, "bIADb"), (7, "bIDQb")):       # UVC_VQ_* order
            if not np.array_equal(ov[k].astype(np.int64), vq[name]): bad[name] = np.argwhere(ov[k] != vq[name])[:4].tolist()
        assert not bad, bad


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("amplicon", [False, True])
def test_clips_sides_cells_and_restatement(amplicon, reverse, oracle_lib):
    case = er.clips(amplicon, reverse)
    reads, beg = case["reads"], case["reads"]["beg"]
    for p in case["placed"]:
        assert er.is_simple(p["ops"]) == (not p["control"]), p["name"]
        assert int(reads["fam_dflag"][reads["fam_id"][p["index"]]]) == (4 if amplicon else 0) and int(reads["fam_strand"][p["index"]]) == int(reverse)
        for _, ln in er.clip_cells(p["pos"], p["ops"]):
            assert ((ln & 0xFFFF) == ln) == p["fits_16_bits"], p["name"]          # does 16 bits hold the length?
            if not p["fits_16_bits"]:
                assert ln >= er.CLIP_MIN_LEN > (ln & 0xFFFF), p["name"]            # the low half alone is a short clip (0, 3, 3, 1, 4)
    assert sorted(ln for p in case["placed"] if not p["control"] for _, ln in er.clip_cells(p["pos"], p["ops"])) == [32767, 32768, 65535, 65535, 65536, 65536, 65537, 65539, 65540, 131075]
    R, Rb = run_region(oracle_lib, reads), run_region(oracle_lib, case["background"])      # accepted, or UvcError
    added = R.fetch("PREP32").astype(np.int64) - Rb.fetch("PREP32")
    want_long, want_pcr = np.zeros(R.npos, np.int64), np.zeros(R.npos, np.int64)
    for p in case["placed"]:
        for pos, ln in er.clip_cells(p["pos"], p["ops"]):
            if amplicon:
                want_pcr[pos - beg - er.NEAR_CLIP_DIST: pos - beg + er.NEAR_CLIP_DIST + 1] += 1
            elif ln >= er.CLIP_MIN_LEN:
                want_long[pos - beg] += 1
    assert np.array_equal(added[LONG_CLIP], want_long) and np.array_equal(added[PCR_CLIP], want_pcr)
    assert want_long.sum() == (0 if amplicon else 10) and want_long.max() <= 1 and want_pcr.sum() == (12 * 5 if amplicon else 0)
    control = [p for p in case["placed"] if p["control"]][0]
    assert all(want_long[pos - beg] == 0 for pos, _ in er.clip_cells(control["pos"], control["ops"]))
    restatements_agree(oracle_lib, reads, R, with_p2=(not amplicon and not reverse))


@pytest.mark.parametrize("platform", [1, 2])
@pytest.mark.parametrize("beg", [100_000, 1_000])
def test_run_offsets_sides(beg, platform, oracle_lib):
    case = er.run_offsets(beg)
    reads = case["reads"]
    assert reads["end"] - reads["beg"] == 66500
    on_list = (platform == 1 and beg >= 65536)                     # without it every InDel read takes the per-read path
    for p in case["placed"]:
        want = p["kind"] if (on_list or p["kind"] == 0) else 1
        assert er.classify(p["ops"], er.quals_of(reads, p), beg, platform) == want, p["name"]
        if "runs_b" in p:
            assert er.runs_b_ok(p["ops"]) == p["runs_b"], p["name"]
    by_name = {p["name"]: p for p in case["placed"]}
    # the long reads: sixty InDels, the extreme M runs exactly on either side of 16 bits
    for name, far in (("both offsets 65535", (65535, 65535)), ("begin offset 65536", (65536, 65535)), ("end offset 65536", (65535, 65536))):
        ops = by_name[name]["ops"]
        offs = er.run_offsets_of(ops)
        assert sum(1 for o, l in ops if o in (I, D)) == 60 and er.ref_len_of(ops) == 66000
        assert (max(a for a, b in offs), max(b for a, b in offs)) == far and not er.has_lowbq_indel(ops, er.quals_of(reads, by_name[name]))
    low = by_name["both offsets 65535, first InDel of low quality"]
    assert er.has_lowbq_indel(low["ops"], er.quals_of(reads, low)) and low["ops"] == by_name["both offsets 65535"]["ops"]
    # deletions either side of aln_runs' bound and of the 16-bit item fields; the low-quality copies take the item path
    dels = {max([l for o, l in p["ops"] if o == D] + [0]) for p in case["placed"]}
    assert {32766, 32767, 65535, 65536} <= dels and any(o == N and l == 66000 for p in case["placed"] for o, l in p["ops"])
    for p in case["placed"]:
        if p["name"].endswith("low quality"):
            assert er.has_lowbq_indel(p["ops"], er.quals_of(reads, p)), p["name"]
    # fragment spans either side of 65 536
    spans = []
    for p in case["placed"]:
        if "span" in p:
            mate = case["placed"][case["placed"].index(p) - 1]
            assert reads["frag_id"][mate["index"]] == reads["frag_id"][p["index"]] and reads["fam_id"][mate["index"]] == reads["fam_id"][p["index"]]
            spans.append(er.frag_span([(mate["pos"], mate["ops"]), (p["pos"], p["ops"])], reads["end"]))
            assert spans[-1] == p["span"] and er.runs_b_ok(p["ops"]) and er.runs_b_ok(mate["ops"])
    assert spans == [65535, 65536, 65537]
    R = run_region(oracle_lib, reads, platform=platform)           # accepted, or UvcError
    assert R.fetch("PREP32")[PREP32.index("a_at_del_dp")].sum() > 30 * 4
    R.close()


@pytest.mark.parametrize("beg", [0, 65535, 65536])
def test_region_begin_inputs(beg, oracle_lib):
    reads = er.region_begin(beg)["reads"]
    assert reads["beg"] == beg and (reads["n_cigar"] > 1).sum() > 50 and reads["pos"].min() >= beg
    n_kind2 = 0
    for i in range(int(reads["n_reads"])):
        co, so = int(reads["cigar_off"][i]), int(reads["seq_off"][i])
        ops = [(int(c) & 0xF, int(c) >> 4) for c in reads["cigars"][co:co + int(reads["n_cigar"][i])]]
        n_kind2 += er.classify(ops, reads["quals"][so:so + int(reads["l_qseq"][i])], beg, 1) == 2
    assert (n_kind2 > 0) == (beg >= 65536)                        # only the last begin puts InDel reads on the work list
    R = run_region(oracle_lib, reads)                              # accepted, or UvcError
    assert R.fetch("PREP32")[PREP32.index("a_at_ins_dp")].sum() > 0
    R.close()


@pytest.mark.parametrize("below", [False, True])
def test_nm_penalty_values_and_restatement(below, oracle_lib):
    case = er.nm_penalty(below)
    reads = case["reads"]
    got = []
    for p in case["placed"]:
        assert int(reads["nm"][p["index"]]) == 0
        got.append(er.penalty(p["ops"], 0))
        assert got[-1] == p["want"], p["name"]
    assert got == [-30000, -30000] + ([-30001] if below else [])
    R = run_region(oracle_lib, reads)                              # the oracle computes both
    restatements_agree(oracle_lib, reads, R, with_p2=True)
    R.close()


@pytest.mark.parametrize("which", er.LONG_FUZZ)
def test_long_fuzz_inputs(which, oracle_lib):
    case = er.long_fuzz(which)
    reads = case["reads"]
    spans = []
    for i in range(int(reads["n_reads"])):
        co = int(reads["cigar_off"][i])
        spans.append(sum(int(c) >> 4 for c in reads["cigars"][co:co + int(reads["n_cigar"][i])] if (int(c) & 0xF) in (M, D, N)))
    assert max(spans) >= 2900 and sum(s >= 1500 for s in spans) >= 10
    if case["placed"]:
        assert sorted(p["run"] for p in case["placed"]) == [4095] * 3 + [4096] * 3 + [4097] * 3 + [8200, 8200, 8213]
        for p in case["placed"]:
            assert er.ref_len_of(p["ops"]) == p["run"] and er.runs_b_ok(p["ops"])
            assert sum(1 for o, l in p["ops"] if o == D) == (1 if which == "runs_4096_del" else 0)
    R = run_region(oracle_lib, reads)                              # accepted, or UvcError
    R.close()


def test_planted_haplotypes_give_links(oracle_lib):
    case = er.planted_haplotypes()
    reads = case["reads"]
    n_hap = sum(p["name"] == "haplotype read" for p in case["placed"])
    assert n_hap == 40 + sum(3 + k % 3 for k in range(12))
    fams = {}
    for p in case["placed"]:
        fams.setdefault(int(reads["fam_id"][p["index"]]), []).append(int(reads["fam_strand"][p["index"]]))
    umi = [s for f, s in fams.items() if reads["fam_dflag"][f] == 0x3]
    assert len(umi) == 12 and all(3 <= len(s) <= 5 and s == sorted(s) and set(s) == {0, 1} for s in umi)
    R = run_region(oracle_lib, reads)
    links = R.hap_links()
    p0 = reads["beg"] + er.HAP_START
    for name, found in zip(("bq", "fq", "f2q"), links):
        ok = False
        for muts, fr, other in found:
            at = [pos - p0 for pos, sym in muts]
            pair = any(a[0] == b[0] == p0 + er.HAP_INS_BEFORE and a[1] > 5 and b[1] <= 5 for a, b in zip(muts, muts[1:]))   # a LINK symbol, then the base at the same position
            ok = ok or (len(muts) >= 5 and 0 in at and 640 in at and pair and min(fr) > 0)
        assert ok, (name, found)
    big = [p for p in case["placed"] if p["name"].startswith("3000M")][0]
    so = int(reads["seq_off"][big["index"]])
    ref = np.array(["ACGT".index(c) for c in reads["refseq"]])
    n_events = int((reads["bases"][so:so + 3000] != ref[big["pos"] - reads["beg"]: big["pos"] - reads["beg"] + 3000]).sum())
    assert 60 <= n_events <= 130                                   # about 90 events in one object
    R.close()
