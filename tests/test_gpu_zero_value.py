"""Quality bytes of 0 and of 0x7F .. 0xFF through every pass behind P1, through uvcgpu_region_correct_bq and through every input form.

A base whose value (quality + bq_phred_added_misma) is 0 or less adds nothing to its fragment's consensus, and the reference skips a
(fragment, position) where nothing adds up (main.hpp:2658-2726; tests/byte_classes.py).  set_reads sends a fragment with such a base to the
per-position kernels (FragRec::stat_kind 2, k_build_frags), told by a device word that the four packing kernels set when they see a quality
byte of 0, or -- with a negative addend -- by looking at the qualities.  The judge is the oracle throughout: all 14 plane groups bit-exact,
no presence violation, the InDel allele rows equal and the records within the classes of test_gpu_parity.compare_records.

B  the family and duplex passes (unit_counts, k_fam_stat, k_fam_p4d / _rest, k_fam_p5d, k_duplex, k_duplex_d) on a 2 kb x 400x duplex tile
   with a quarter of the bases low, qualities from 0 on, under the switch matrix of test_gpu_kernel_forms.py; and a hand-made tile.
C  uvcgpu_region_correct_bq with a negative increment or a cap of 0 makes bases of value 0 after set_reads decided stat_kind.
D  one quality byte of 0 where only one branch of one packing kernel sees it.
E  bytes 0x7F, 0x80, 0xC8 and 0xFF, and reads of 0xFF throughout (BAM's "no qualities").

Against a library whose k_build_frags never assigns stat_kind 2, B (but for the arms without a value-0 base on the closed forms: +3 and the two
IonTorrent arms, where every fragment takes k_frag_generic), the zeros-disappear case of C and all 24 cells of D fail, in FRAG and VQ; the cases
of C that make new zeros (a negative increment; a cap of 0 on reads too short for the tail penalty; any correction under a negative
bq_phred_added_misma) fail on a library without k_requalify_frags (DESIGN.md section 6-r6 has the cell counts).  The IonTorrent arm with values
below 0 is there for k_p2_slow / k_p2_items (the signed Item::val), the smaller-addend rule at the ends of M runs and k_frag_generic."""
import functools

import numpy as np
import pytest

from uvc_amd import region, synth
from byte_classes import iontorrent_run_end_values_below_0, set_params, simple_fragments_with_a_zero
from kernel_forms import ARMS, IONTORRENT, TILES, expected_forms, switches
from test_bq_correction import corrected, expected_quals
from test_gpu_device_reads import DeviceColumns
from test_gpu_kernel_forms import check_cell, set_switch
from test_gpu_prep_scan import FORMS, case1, lower_qualities, ran
from test_gpu_worklist import M, check, oracle_run, unpaired
from util import diff_groups, presence_violations

pytestmark = pytest.mark.gpu

TILE = "umi_duplex_2kb_400x"
EUNSUPPORTED = -3   # UVCGPU_EUNSUPPORTED
BDP, BTA, BTB = 0, 1, 2            # FRAG planes
CDP1, CDP12, CDP2, CDPD = 0, 1, 2, 7   # FAM planes (tests/p45_restatement.py FAM)
BASES = slice(0, 6)                # the BASE rows of a plane group: A C G T N and the padded deletion


def params(lib, platform=1, values=None):
    return set_params(region.default_params(lib, platform=platform), values)


def run(lib, reads, platform=1, values=None):
    R = region.Region(lib, params(lib, platform, values), reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    R.accumulate()
    return R


def check_all(Ro, ro, Rg, what=""):
    """Planes, presence, allele rows and records."""
    check(Ro, ro, Rg, what)
    assert Ro.indel_alleles() == Rg.indel_alleles(), what


# ---------------------------------------------------------------------------------------------------------------- B: families and duplexes
@functools.lru_cache(maxsize=None)
def duplex_tile(lowest):
    """TILES["umi_duplex_2kb_400x"] (5 254 reads; set_reads takes the digest form) with about a quarter of the qualities lowest..19.  Counted once
    on the CPU with lowest=0: 2 147 fragments of no more than two one-op alignments hold an aligned base of quality 0; the oracle's bDP BASE rows
    add up to 760 204 against 771 340 with lowest=1; cDP2 288 267, cDPD 75 351, DUPLEX 226 819."""
    return lower_qualities(synth.generate_region(**TILES[TILE]["gen"]), seed=51, lowest=lowest)


# arm -> (lowest quality, platform, parameters).  IonTorrent's defaults for bias_thres_PFBQ1 / 2 are 0, and dealwith_segbias divides by their squares for a
# value below them (main.hpp:1473-1474): with bq_phred_added_indel = -10 and nothing else set, the reference and the oracle end in a division by
# zero and uvcgpu_params_check refuses the setting (test_what_the_addends_may_be).  The arm therefore sets the two thresholds as well.
B_ARMS = {
    "default": (0, 1, {}),
    "fam_thres_highBQ_snv_0": (0, 1, dict(fam_thres_highBQ_snv=0)),          # `adj > 0` is the only gate in front of the family votes
    "fam_thres_highBQ_snv_minus5": (0, 1, dict(fam_thres_highBQ_snv=-5)),
    "sscs_table_low_phreds": (0, 1, ARMS["sscs_table_low_phreds"]["set"]),
    "iontorrent_sscs_primer": (0, IONTORRENT, ARMS["iontorrent_sscs_primer"]["set"]),
    "misma_plus3_word_set_no_zero_value": (0, 1, dict(bq_phred_added_misma=3)),
    "misma_minus20_word_unset": (1, 1, dict(bq_phred_added_misma=-20)),
    "iontorrent_indel_minus10": (1, IONTORRENT, dict(bq_phred_added_indel=-10, bias_thres_PFBQ1=25, bias_thres_PFBQ2=30)),
}
_b_oracle = {}


def b_oracle(oracle_lib, arm):
    if arm not in _b_oracle:
        lowest, platform, values = B_ARMS[arm]
        reads = duplex_tile(lowest)
        Ro = run(oracle_lib, reads, platform, values)
        p = params(oracle_lib, platform, values)
        _b_oracle[arm] = (reads, Ro, Ro.score(all_out=False) if p.inferred_is_vcf_generated else None)
    return _b_oracle[arm]


def test_the_duplex_tile_holds_the_class(oracle_lib):
    """Asserted on the oracle before any comparison: families of two and duplexes exist, the skip took effect, and the closed forms would have
    been taken by at least 100 fragments with a quality-0 base."""
    reads, Ro, _ = b_oracle(oracle_lib, "default")
    fam, dup = Ro.fetch("FAM"), Ro.fetch("DUPLEX")
    assert fam[:, CDP2].any() and fam[:, CDPD].any() and dup.any()
    R1 = run(oracle_lib, duplex_tile(1))
    assert int(R1.fetch("FRAG")[:, BDP, BASES].sum()) > int(Ro.fetch("FRAG")[:, BDP, BASES].sum())
    R1.close()
    assert reads["quals"].min() == 0 and simple_fragments_with_a_zero(reads) >= 100
    # the +3 arm: the word is set, no base has value 0, and the planes are those of a tile without the class
    assert simple_fragments_with_a_zero(duplex_tile(1)) == 0
    # the IonTorrent arm: 106 first or last bases of an M run, next to an op shorter than 3, have a value below 0
    lowest, _, values = B_ARMS["iontorrent_indel_minus10"]
    assert iontorrent_run_end_values_below_0(duplex_tile(lowest), values.get("bq_phred_added_misma", 8), values["bq_phred_added_indel"]) >= 100


@pytest.mark.parametrize("arm", list(B_ARMS))
def test_value_0_bases_through_the_family_and_duplex_passes(arm, oracle_lib, gpu_lib, monkeypatch, capfd):
    """(UVCGPU_FRAG32 off / on) x (UVCGPU_FAM_PATH unset / generic) x (UVCGPU_SPLIT 0 then 1 on one handle), as test_gpu_kernel_forms.py."""
    lowest, platform, values = B_ARMS[arm]
    reads, Ro, ro = b_oracle(oracle_lib, arm)
    p = params(gpu_lib, platform, values)
    failures, n_cells = [], 0
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    try:
        for frag32, fam_path, splits in switches(TILE):
            set_switch(monkeypatch, "UVCGPU_FRAG32", "1" if frag32 else None)
            set_switch(monkeypatch, "UVCGPU_FAM_PATH", fam_path)
            R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
            capfd.readouterr()
            R.set_reads(reads)
            fam_line = [l for l in capfd.readouterr().err.splitlines() if "family form" in l]
            assert len(fam_line) == 1 and fam_line[0].endswith("family form " + ("digest" if fam_path is None else "generic")), (arm, fam_path, fam_line)
            for split in splits:
                monkeypatch.setenv("UVCGPU_SPLIT", split)
                R.accumulate()
                err = capfd.readouterr().err
                label = "%s / FRAG32=%s FAM_PATH=%s SPLIT=%s" % (arm, int(frag32), fam_path or "auto", split)
                want = expected_forms(p, TILES[TILE], split, frag32=frag32, fam_generic=(fam_path == "generic"))
                failures += check_cell(label, Ro, ro, R, want, err)
                if presence_violations(R):
                    failures.append(label + ": presence violations")
                if Ro.indel_alleles() != R.indel_alleles():
                    failures.append(label + ": InDel allele rows differ")
                n_cells += 1
            R.close()
    finally:
        for name in ("UVCGPU_TIMING", "UVCGPU_FRAG32", "UVCGPU_FAM_PATH", "UVCGPU_SPLIT"):
            monkeypatch.delenv(name, raising=False)
    assert not failures, "%d of %d cells fail:\n" % (len({f.split(":")[0] for f in failures}), n_cells) + "\n".join(failures)


W = 52   # one window of the hand-made tile per shape: reads within [b + 5, b + 50) of it


def hand_made_tile():
    """Ten shapes, each alone in a window of 52 positions (b = 10 + 52 w; 592 positions in all), then a stack that makes set_reads choose the digest form.  Every read is
    one M run of quality 35 but for the bases named; families carry fam_dflag 0x1 (UMI) or 0x3 (UMI + duplex).  p = b + 27.

     w0  a read of quality 0 throughout                                              bDP: no BASE row in the window
     w1  a pair, both mates 0 at the overlapped p                                    bDP at p 0, at p +- 1 one fragment
     w2  a pair, one mate 0 at p, the other 35                                       bDP at p one fragment
     w3  a family of three fragments, each 0 at p                                    cDP1 and cDP12 at p 0, at p +- 1 one family
     w4  a family of two fragments that are 0 everywhere                             FAM and bDP: no BASE row in the window
     w5  two singleton families, both 0 at p: only value-0 bases cover p             bDP, bIADb and cDP1 at p 0 (totDP is 0 in P3b and P5b)
     w6  a 0 on a fragment's first and last aligned base                             bDP 0 there; bTA (n_cov) 39 of 40: the last base keeps its LINK_M
     w7  a 0 two positions behind a high-quality mismatch                            no bDP / bTB cell at that base; bTB (n_near) elsewhere 2 x 11 + 1
     w8  a 0 on the mismatching base itself                                          bTB: nothing in the window (no mutation), bDP at the base 0
     w9  a duplex family, the 0 at p on the two fragments of strand 0 only           cDP1 at p 0 on strand 0, 1 on strand 1; DUPLEX at p half of p +- 1
     w10 70 duplex families x 2 strands x 2 fragments, every 7th base 0"""
    n_ref = 10 + 11 * W + 10
    beg = 7_000_000
    rng = np.random.default_rng(71)
    ref = rng.integers(0, 4, n_ref)
    rows = []   # (fam, strand, frag, start, flag, mpos, isize, bases, quals)
    fam = [0]; frag = [0]; dflags = []

    def read(start, ln, strand=0, zeros=(), q=35, mism=(), flag=None, mpos=-1, isize=0):
        b = ref[start:start + ln].copy()
        for m in mism:
            b[m - start] = (b[m - start] + 1) % 4
        qq = np.full(ln, q, np.uint8)
        for z in zeros:
            qq[z - start] = 0
        rows.append((fam[0], strand, frag[0], start, (16 * strand if flag is None else flag), mpos, isize, b, qq))

    def next_frag(): frag[0] += 1
    def next_fam(dflag): dflags.append(dflag); fam[0] += 1; frag[0] += 1

    def pair(b, z1, z2):
        # R1 forward [b + 5, b + 35), R2 reverse [b + 20, b + 50): insert of 45
        read(b + 5, 30, zeros=z1, flag=0x1 | 0x2 | 0x40 | 0x20, mpos=beg + b + 20, isize=45)
        read(b + 20, 30, zeros=z2, flag=0x1 | 0x2 | 0x80 | 0x10, mpos=beg + b + 5, isize=-45)
    b = lambda w: 10 + W * w
    p = lambda w: b(w) + 27
    read(b(0) + 5, 40, q=0); next_fam(0x1)
    pair(b(1), (p(1),), (p(1),)); next_fam(0x1)
    pair(b(2), (p(2),), ()); next_fam(0x1)
    for _ in range(3): read(b(3) + 5, 40, zeros=(p(3),)); next_frag()
    next_fam(0x1)
    for _ in range(2): read(b(4) + 5, 40, q=0); next_frag()
    next_fam(0x1)
    read(b(5) + 5, 40, zeros=(p(5),)); next_fam(0x1)
    read(b(5) + 8, 40, strand=1, zeros=(p(5),)); next_fam(0x1)
    read(b(6) + 5, 40, zeros=(b(6) + 5, b(6) + 44)); next_fam(0x1)
    read(b(7) + 5, 40, zeros=(p(7) + 2,), mism=(p(7),)); next_fam(0x1)
    read(b(8) + 5, 40, zeros=(p(8),), mism=(p(8),)); next_fam(0x1)
    for strand in (0, 1):
        for _ in range(2): read(b(9) + 5, 40, strand=strand, zeros=((p(9),) if strand == 0 else ())); next_frag()
    next_fam(0x3)
    for k in range(70):
        for strand in (0, 1):
            for f in range(2):
                s = b(10) + 5 + (k % 6)
                read(s, 40, strand=strand, zeros=[z for z in range(s, s + 40) if (z + k + f) % 7 == 0]); next_frag()
        next_fam(0x3)
    n = len(rows)
    lq = np.array([len(r[7]) for r in rows], np.int32)
    reads = dict(n_reads=n, pos=np.array([beg + r[3] for r in rows], np.int32), mpos=np.array([r[5] for r in rows], np.int32), isize=np.array([r[6] for r in rows], np.int32),
                 flag=np.array([r[4] for r in rows], np.uint16), mapq=np.full(n, 60, np.uint8), nm=np.full(n, -1, np.int32), l_qseq=lq,
                 seq_off=np.concatenate(([0], np.cumsum(lq)))[:n].astype(np.int64), cigar_off=np.arange(n, dtype=np.int64), n_cigar=np.ones(n, np.int32),
                 frag_id=np.array([r[2] for r in rows], np.int32), fam_id=np.array([r[0] for r in rows], np.int32), fam_strand=np.array([r[1] for r in rows], np.uint8),
                 n_fams=len(dflags), fam_dflag=np.array(dflags, np.uint8), bases=np.concatenate([r[7] for r in rows]).astype(np.uint8),
                 quals=np.concatenate([r[8] for r in rows]), cigars=(lq.astype(np.uint32) << 4) | M, tid=1, beg=beg, end=beg + n_ref, refseq="".join("ACGT"[c] for c in ref))
    return reads, b, p


def hand_made_on_the_oracle(oracle_lib):
    """Every shape of hand_made_tile shows in the oracle plane named there."""
    reads, b, p = hand_made_tile()
    Ro = run(oracle_lib, reads)
    ro = Ro.score()
    frag, fam, dup, vq = Ro.fetch("FRAG").astype(np.int64), Ro.fetch("FAM").astype(np.int64), Ro.fetch("DUPLEX").astype(np.int64), Ro.fetch("VQ").astype(np.int64)
    bdp = frag[:, BDP, BASES].sum(axis=(0, 1))                    # fragments per position, both strands
    win = lambda w: slice(b(w), b(w) + W)
    nb = int(params(oracle_lib).syserr_mut_region_n_bases)
    assert nb == 11
    assert not frag[:, :, BASES, win(0)].any() and frag[:, BDP, 6, win(0)].any()     # (LINK_M has a value of its own: the fragment is there)
    assert bdp[p(1) - 1:p(1) + 2].tolist() == [1, 0, 1]
    assert bdp[p(2) - 1:p(2) + 2].tolist() == [1, 1, 1]
    c1 = fam[:, CDP1, BASES].sum(axis=(0, 1)); c12 = fam[:, CDP12, BASES].sum(axis=(0, 1))
    assert c1[p(3) - 1:p(3) + 2].tolist() == [1, 0, 1] and c12[p(3) - 1:p(3) + 2].tolist() == [1, 0, 1] and bdp[p(3) - 1:p(3) + 2].tolist() == [3, 0, 3]
    assert not fam[:, :, BASES, win(4)].any() and not frag[:, :, BASES, win(4)].any()
    assert bdp[p(5) - 1:p(5) + 2].tolist() == [2, 0, 2] and not vq[5:8, BASES, p(5)].any() and c1[p(5)] == 0 and vq[6, BASES, p(5) - 1].sum() > 0   # bIAQb bIADb bIDQb
    s6 = b(6) + 5
    # (a position counts as covered when either symbol type adds up: the last base still has its LINK_M, the first one never had)
    assert bdp[s6:s6 + 40].tolist() == [0] + [1] * 38 + [0] and set(frag[0, BTA, BASES, s6 + 1:s6 + 39].sum(axis=0).tolist()) == {39}
    # w7: the mutation at p reaches nb positions either side: 2 nb + 1 = 23 positions of the read, the one without a base value covered by its LINK_M
    assert bdp[p(7) + 2] == 0 and frag[0, BTB, BASES, p(7) + 2].sum() == 0 and set(frag[0, BTB, BASES, p(7) - 5:p(7) + 2].sum(axis=0).tolist()) == {2 * nb + 1}
    assert not frag[:, BTB, :, win(8)].any() and bdp[p(8) - 1:p(8) + 2].tolist() == [1, 0, 1]
    assert fam[0, CDP1, BASES, p(9)].sum() == 0 and fam[1, CDP1, BASES, p(9)].sum() == 1 and fam[0, CDP1, BASES, p(9) + 1].sum() == 1
    assert dup[:, BASES, p(9) - 1:p(9) + 2].sum(axis=(0, 1)).tolist() == [2, 1, 2]
    assert dup[:, :, win(10)].any()
    return reads, Ro, ro


def test_hand_made_shapes(oracle_lib, gpu_lib, monkeypatch, capfd):
    """The oracle's planes show every shape; then both family forms of the library against the oracle."""
    reads, Ro, ro = hand_made_on_the_oracle(oracle_lib)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    for fam_path in (None, "generic"):
        set_switch(monkeypatch, "UVCGPU_FAM_PATH", fam_path)
        capfd.readouterr()
        Rg = run(gpu_lib, reads)
        err = capfd.readouterr().err
        assert [l for l in err.splitlines() if "family form" in l][0].endswith("family form " + ("digest" if fam_path is None else "generic")), err
        check_all(Ro, ro, Rg, "family form %s: " % (fam_path or "digest"))
        Rg.close()
    Ro.close()


def test_what_the_addends_may_be(gpu_lib):
    """A base's value is never below the addend; the factor tables of k_p2_fast hold the values from -256 on, its 24-bit multiply and the 16-bit
    averages of k_frag values below 2^12 (255 + 3840).  Where a value can fall below 0, a bias_thres_PFBQ1 / 2 of 0 (the IonTorrent default) makes the
    reference divide by zero.  All of this is refused when the handle is made, not approximated."""
    reads, _, _ = hand_made_tile()

    def made(platform, values):
        p = params(gpu_lib, platform, values)
        try:
            region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"]).close()
        except region.UvcError as e:
            assert e.code == EUNSUPPORTED, e
            return str(e)
        return None
    for name in ("bq_phred_added_misma", "bq_phred_added_indel"):
        assert made(1, {name: -256}) is None and "below -256" in made(1, {name: -257})
        assert made(1, {name: 3840}) is None and "above 3840" in made(1, {name: 3841})
        assert "bias_thres_PFBQ2 of 0" in made(1, {name: -1, "bias_thres_PFBQ2": 0}) and "bias_thres_PFBQ2 of 0" in made(1, {name: -1, "bias_thres_PFBQ1": 0})
        assert made(1, {name: -1, "bias_thres_PFBQ1": -3, "bias_thres_PFBQ2": 1}) is None
    assert made(IONTORRENT, {}) is None                                    # bq_phred_added_misma is 8 there, the thresholds are 0
    assert "bias_thres_PFBQ2 of 0" in made(IONTORRENT, dict(bq_phred_added_indel=-10))
    assert "bias_thres_PFBQ2 of 0" in made(IONTORRENT, dict(bq_phred_added_misma=-1))
    assert made(IONTORRENT, B_ARMS["iontorrent_indel_minus10"][2]) is None


# ---------------------------------------------------------------------------------------------------------------- C: correct_bq
@functools.lru_cache(maxsize=None)
def bq_tile(kind):
    """kind 0 / 2: a simple paired tile, 1 kb x 40x without InDel reads or clips; a quarter of the qualities kind..19 and one in ten of those exactly 2
    (Illumina's tail marker).  2 is the tile of the (37, -2) case: no quality below 2, so the increment wraps no byte.
    "short": 400 unpaired reads of 5 .. 9 bases, qualities 20 and more: too short for the tail penalty (10 bases and more), so a cap of 0 leaves
    qualities of 0 but for the fourth and later G of a run, which the homopolymer penalty sets to 1.
    "tails": the paired tile with qualities of 21 and more, but 11 or 12 on the first and the last 16 bases of every third read.  Under
    bq_phred_added_misma = -10 every base has a value until the correction takes the tail penalty of 2 off the 16 bases at the read's 3' end."""
    if kind == "short":
        rng = np.random.default_rng(63)
        reads = unpaired([(int(s), 16 * (k % 2), [(M, 5 + k % 5)]) for k, s in enumerate(np.sort(rng.integers(5, 380, 400)))], seed=64)
        reads["quals"] = rng.choice([20, 30, 37], len(reads["quals"])).astype(np.uint8)
        return reads
    reads = synth.generate_region(seed=61, region_len=1000, depth=40, indel_every=0, clip_frac=0)
    if kind == "tails":
        rng = np.random.default_rng(65)
        q = rng.choice([21, 22, 30, 37], len(reads["quals"])).astype(np.uint8)
        for k in range(0, int(reads["n_reads"]), 3):
            so, l = int(reads["seq_off"][k]), int(reads["l_qseq"][k])
            assert l >= 40
            q[so:so + 16] = rng.choice([11, 12], 16); q[so + l - 16:so + l] = rng.choice([11, 12], 16)
        reads["quals"] = q
        return reads
    reads = lower_qualities(reads, seed=62, lowest=kind)
    q = reads["quals"].copy()
    low = np.flatnonzero(q < 20)
    q[low[::10]] = 2
    reads["quals"] = q
    assert (reads["n_cigar"] == 1).all() and q.min() == min(kind, 2) and (q == 2).sum() > 100
    return reads


# (assay_sequencing_BQ_max, assay_sequencing_BQ_inc, tile, further parameters)
BQ_CASES = {"new_zeros_from_a_negative_increment": (37, -2, 2, None), "cap_of_0": (0, 0, 2, None), "cap_of_0_short_reads": (0, 0, "short", None),
            "zeros_disappear": (37, 3, 0, None), "control": (37, 0, 2, None), "misma_minus10_tails_lowered_to_0": (37, 0, "tails", dict(bq_phred_added_misma=-10))}
_c_oracle, _c_plain = {}, {}


def corrected_with(lib, reads, bq_max, bq_inc, values):
    """test_bq_correction.corrected(accumulate=True) with further parameters set."""
    if not values:
        return corrected(lib, reads, bq_max, bq_inc, accumulate=True)
    p = params(lib, values=values)
    p.assay_sequencing_BQ_max, p.assay_sequencing_BQ_inc = bq_max, bq_inc
    R = region.Region(lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    R.set_reads(reads)
    R.correct_bq()
    q = R.read_quals(len(reads["quals"]))
    R.accumulate()
    return R, q


def c_oracle(oracle_lib, case):
    if case not in _c_oracle:
        bq_max, bq_inc, tile, values = BQ_CASES[case]
        reads = bq_tile(tile)
        Ro, qo = corrected_with(oracle_lib, reads, bq_max, bq_inc, values)
        want = expected_quals(reads, bq_max, bq_inc).astype(np.uint8)
        assert np.array_equal(qo, want)
        _c_oracle[case] = (reads, Ro, Ro.score(), qo)
    return _c_oracle[case]


def sweep_lines(err):
    return [l for l in err.splitlines() if l.startswith("[uvcgpu correct_bq] fragments looked at again")]


def frag_generic_of(err):
    return [l.split("frag_generic=")[1].split()[0] for l in err.splitlines() if l.startswith("[uvcgpu accumulate] forms ")]


@pytest.mark.parametrize("case", list(BQ_CASES))
def test_correct_bq_makes_or_removes_zeros(case, oracle_lib, gpu_lib, monkeypatch, capfd):
    """set_reads, correct_bq, accumulate in both libraries: the corrected qualities equal the restatement of test_bq_correction.py and each other,
    then planes, allele rows and records.  A fragment that gains a base of value 0 must leave the closed forms; the default path (an increment
    of 0 or more under a positive cap) looks at no fragment again and launches what it launched before: no sweep list on this tile."""
    bq_max, bq_inc, tile, values = BQ_CASES[case]
    reads, Ro, ro, qo = c_oracle(oracle_lib, case)
    no_value = -(values or {}).get("bq_phred_added_misma", 0)      # a quality of this or less has no value
    if case == "new_zeros_from_a_negative_increment":
        assert reads["quals"].min() == 2 and (qo == 0).sum() > 100
    if case == "cap_of_0":
        # NOT a case of new zeros: with a cap of 0 no quality reaches 20, the tail scan runs through every read of this tile, and the tail penalty's
        # floor is 1.  The fragments are looked at again and none joins; the case would pass without k_requalify_frags.
        assert qo.min() == 1 and qo.max() == 1
    if case == "cap_of_0_short_reads":
        assert (qo == 0).sum() > 1000 and qo.max() <= 1
    if case == "zeros_disappear":
        assert reads["quals"].min() == 0 and qo.min() > 0
    if case == "misma_minus10_tails_lowered_to_0":
        assert reads["quals"].min() == 11 > no_value and (qo <= no_value).sum() > 100
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    capfd.readouterr()
    Rg, qg = corrected_with(gpu_lib, reads, bq_max, bq_inc, values)
    err = capfd.readouterr().err
    assert np.array_equal(qo, qg), np.flatnonzero(qo != qg)[:10]
    check_all(Ro, ro, Rg, case + ": ")
    if bq_inc < 0 or bq_max <= 0 or no_value > 0:
        assert len(sweep_lines(err)) == 1 and frag_generic_of(err) == ["sweep" if (qo <= no_value).any() else "none"], err
        assert ("looked at again: 0 joined" in sweep_lines(err)[0]) == (not (qo <= no_value).any()), err
    else:
        assert not sweep_lines(err), err
        assert frag_generic_of(err) == [("sweep" if tile == 0 else "none")], err
    Rg.close()


@pytest.mark.parametrize("case", list(BQ_CASES))
def test_correct_bq_on_a_used_handle(case, oracle_lib, gpu_lib):
    """The case, then a tile without zeros on the same handle, then the case again."""
    bq_max, bq_inc, tile, values = BQ_CASES[case]
    one = c_oracle(oracle_lib, case)
    if values:
        if case not in _c_plain:
            Rp = run(oracle_lib, bq_tile(2), values=values)
            _c_plain[case] = (bq_tile(2), Rp, Rp.score())
        plain = _c_plain[case]
    else:
        plain = oracle_run(oracle_lib, "zero_value_plain", lambda: bq_tile(2))
    p = params(gpu_lib, values=values)
    p.assay_sequencing_BQ_max, p.assay_sequencing_BQ_inc = bq_max, bq_inc
    reads = one[0]
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    for k, (reads, Ro, ro, with_bq) in enumerate(((one[0], one[1], one[2], True), (plain[0], plain[1], plain[2], False), (one[0], one[1], one[2], True))):
        if k:
            R.reset(reads["tid"], reads["beg"], reads["end"], reads["refseq"])
        R.set_reads(reads)
        if with_bq:
            R.correct_bq()
            assert np.array_equal(R.read_quals(len(reads["quals"])), one[3])
        R.accumulate()
        check_all(Ro, ro, R, "%s, use %d: " % (case, k))
    R.close()


# ---------------------------------------------------------------------------------------------------------------- D: the zero word
def stack_300(even):
    """300 unpaired one-op reads over 400 positions, qualities 20 and more.  even=False: lengths 41 .. 71 of both parities, 16 777 bases (no
    multiple of 8: k_pack_bq has a tail, the compact form takes k_pack_bq4_reads); even=True: lengths 40 .. 70, all even, 16 456 bases (a multiple
    of 8: the compact form takes k_pack_bq4_dense)."""
    rng = np.random.default_rng(81)
    starts = np.sort(rng.integers(5, 320, 300))
    lens = [(40 + 2 * (k % 16)) if even else (41 + (k * 7) % 31) for k in range(300)]
    if even:
        lens[-1] += 8 - sum(lens) % 8 if sum(lens) % 8 else 0
    reads = unpaired([(int(s), 16 * (k % 2), [(M, lens[k])]) for k, s in enumerate(starts)], seed=82)
    reads["quals"] = np.random.default_rng(83).choice([20, 30, 37], len(reads["quals"])).astype(np.uint8)
    n = len(reads["quals"])
    assert (n % 8 == 0) == even and (np.asarray(reads["l_qseq"]) % 2 == 1).any() != even
    return reads


def placements(reads):
    """Where the one quality byte of 0 goes -> index into the quality column."""
    so, lq = np.asarray(reads["seq_off"]), np.asarray(reads["l_qseq"])
    n = len(reads["quals"])
    odd = int(np.flatnonzero(lq % 2 == 1)[7]) if (lq % 2 == 1).any() else None
    out = {"first_byte_of_the_column": 0,
           "inside_a_wide_turn": int(so[150]) + 19,
           "last_byte_of_the_column": n - 1,                         # in the n % 8 tail of k_pack_bq where there is one
           "bases_8_to_15_of_a_read": int(so[200]) + 11}
    if odd is not None:
        out["last_base_of_an_odd_length_read"] = int(so[odd] + lq[odd] - 1)   # one of the 1 .. 7 bases k_pack_bq4_reads takes one by one
    return out


INPUT_FORMS = ("host", "device_aligned", "device_one_byte_off", "compact")
_d_oracle = {}


def d_oracle(oracle_lib, even, where):
    key = (even, where)
    if key not in _d_oracle:
        reads = dict(stack_300(even))
        if where is not None:
            q = reads["quals"].copy()
            q[placements(reads)[where]] = 0
            reads["quals"] = q
        Ro = run(oracle_lib, reads)
        _d_oracle[key] = (reads, Ro, Ro.score())
        if where is not None:
            assert (reads["quals"] == 0).sum() == 1 and reads["quals"][reads["quals"] > 0].min() >= 20
            plain = d_oracle(oracle_lib, even, None)[1]
            d = plain.fetch("FRAG").astype(np.int64)[:, BDP, BASES].sum(axis=(0, 1)) - Ro.fetch("FRAG").astype(np.int64)[:, BDP, BASES].sum(axis=(0, 1))
            assert d.sum() == 1 and d.max() == 1                     # the oracle misses one fragment at one position
    return _d_oracle[key]


WHERE = ("first_byte_of_the_column", "inside_a_wide_turn", "last_byte_of_the_column", "last_base_of_an_odd_length_read", "bases_8_to_15_of_a_read")
# every placement through the four input forms of the mixed-length stack; the even-length stack is there for k_pack_bq4_dense alone and has no odd read
D_CELLS = [(False, w, f) for w in WHERE for f in INPUT_FORMS] + [(True, w, "compact") for w in WHERE if w != "last_base_of_an_odd_length_read"]


@pytest.mark.parametrize("even,where,form", D_CELLS, ids=["%s-%s-%s" % ("even_lengths" if e else "mixed_lengths", w, f) for e, w, f in D_CELLS])
def test_one_zero_byte_reaches_the_zero_word(even, where, form, oracle_lib, gpu_lib, monkeypatch, capfd):
    """Exactly one aligned base of quality 0 in the column: its fragment is a simple one, so a packing branch that does not set the word leaves it
    to the closed forms, one fragment too many in bDP at that position and wrong bTA / bTB along the fragment.  host / device columns take
    k_pack_bq (the last n % 8 bytes in block 0's tail), columns one byte off k_pack_bq1, the compact form k_pack_bq4_reads (mixed lengths) or
    k_pack_bq4_dense (even lengths, a multiple of 8 bases); which one ran is read from the library's timing line."""
    reads, Ro, ro = d_oracle(oracle_lib, even, where)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    capfd.readouterr()
    p = region.default_params(gpu_lib)
    R = region.Region(gpu_lib, p, reads["tid"], reads["beg"], reads["end"], reads["refseq"])
    cols = None
    if form == "host":
        R.set_reads(reads)
    elif form == "compact":
        comp = region.compact_form(reads)
        assert (2 * comp["bases4"].size == reads["bases"].size) == even
        R.set_reads(comp)
    else:
        cols = DeviceColumns(reads, misalign=(1 if form == "device_one_byte_off" else 0))
        assert (cols.soa.quals % 8 != 0) == (form == "device_one_byte_off")
        R.set_reads_device((cols.soa, cols))
    want = {"host": "k_pack_bq", "device_aligned": "k_pack_bq", "device_one_byte_off": "k_pack_bq1", "compact": "k_pack_bq4_dense" if even else "k_pack_bq4_reads"}[form]
    err = capfd.readouterr().err
    assert [l.split()[-1] for l in err.splitlines() if l.startswith("[uvcgpu pack_bq]")] == [want], err
    R.accumulate()
    check_all(Ro, ro, R, "%s / %s: " % (where, form))
    R.close()
    if cols is not None:
        cols.free()


# ---------------------------------------------------------------------------------------------------------------- E: bytes of 0x7F and above
HIGH_BYTES = (0x7F, 0x80, 0xC8, 0xFF)


@functools.lru_cache(maxsize=None)
def high_byte_reads():
    """Case 1 of test_gpu_prep_scan.py (qualities from 0 on) with 5 % of the qualities 0x7F, 0x80, 0xC8 or 0xFF and every 17th read 0xFF throughout."""
    reads = dict(case1())
    rng = np.random.default_rng(91)
    q = reads["quals"].copy()
    hit = rng.random(len(q)) < 0.05
    q[hit] = rng.choice(HIGH_BYTES, int(hit.sum()))
    for k in range(0, int(reads["n_reads"]), 17):
        q[int(reads["seq_off"][k]):int(reads["seq_off"][k]) + int(reads["l_qseq"][k])] = 0xFF
    reads["quals"] = q
    assert all((q == v).sum() > 500 for v in HIGH_BYTES) and (q == 0).any()
    return reads


_e_oracle = {}


def e_oracle(oracle_lib, highBQ):
    if highBQ not in _e_oracle:
        reads = high_byte_reads()
        Ro = run(oracle_lib, reads, values=({} if highBQ is None else dict(bias_thres_highBQ=highBQ)))
        _e_oracle[highBQ] = (reads, Ro, Ro.score())
    return _e_oracle[highBQ]


@pytest.mark.parametrize("highBQ", [None, 20, 128, 200])
def test_high_quality_bytes_in_both_forms_of_p1(highBQ, oracle_lib, gpu_lib, monkeypatch, capfd):
    """The whole chain without correct_bq, by k_prep_fast<false> and by k_prep_scan, each against the oracle and one against the other; with
    bias_thres_highBQ at its default and at 20, 128 and 200, so that the threshold of the byte-parallel tests lies above 0x7F too."""
    reads, Ro, ro = e_oracle(oracle_lib, highBQ)
    values = {} if highBQ is None else dict(bias_thres_highBQ=highBQ)
    monkeypatch.setenv("UVCGPU_TIMING", "1")
    monkeypatch.delenv("UVCGPU_SPLIT", raising=False)
    out = {}
    for f in FORMS:
        monkeypatch.setenv("UVCGPU_PREP", f)
        capfd.readouterr()
        out[f] = run(gpu_lib, reads, values=values)
        assert ran(capfd.readouterr().err) == [FORMS[f]]
    for f in FORMS:
        check_all(Ro, ro, out[f], "%s: " % f)
    assert not diff_groups(out["window"], out["scan"])
    for R in out.values():
        R.close()


def test_high_quality_bytes_through_correct_bq(oracle_lib, gpu_lib):
    """The same reads with uvcgpu_region_correct_bq at its defaults, as on the command line: every quality is capped at 37."""
    reads = high_byte_reads()
    Ro, qo = corrected(oracle_lib, reads, 37, 0, accumulate=True)
    Rg, qg = corrected(gpu_lib, reads, 37, 0, accumulate=True)
    assert qo.max() == 37 and np.array_equal(qo, expected_quals(reads, 37, 0).astype(np.uint8)) and np.array_equal(qo, qg)
    check_all(Ro, Ro.score(), Rg)
    Ro.close(); Rg.close()
