"""The quality-byte classes the suite covers besides ordinary Phred values, and how a test shows that its data holds them.

A base whose value (quality + bq_phred_added_misma; at the ends of an IonTorrent M run the smaller of two qualities + the smaller addend) is 0 or
less adds nothing to its fragment's consensus counts (incSymbolCount<BASE_QUALITY_MAX> keeps the larger of the count and the value, main.hpp:339-349),
and a (fragment, position) whose BASE counts add up to 0 is skipped by the fragment pass and never reaches a family (main.hpp:2658-2726).  Such
bases come from a quality byte of 0, or from a negative addend on a quality at or below its size.  Bytes of 0x80 and above (BAM's "no qualities"
marker is 0xFF throughout a read) are ordinary large values to the reference, which reads qualities as unsigned bytes."""
import numpy as np

from p2_restatement import read_events

NEGATIVE_MISMA = dict(bq_phred_added_misma=-20)                                     # qualities 2, 8, 15, 20 of the fuzz generator's list lose their value
# IonTorrent with bq_phred_added_indel < bq_phred_added_misma < 0: the smaller addend applies at the end of an M run next to an op shorter than 3,
# to the smaller of the base's quality and its neighbour's -- or 1 where the read ends there (main.hpp:1953-1975).  Values fall below 0 here, so
# bias_thres_PFBQ1 / 2 are set too: IonTorrent's defaults for them are 0, and dealwith_segbias divides by their squares for a value below them
# (main.hpp:1473-1474) -- with everything else at its IonTorrent default the reference, and the oracle with it, ends in a division by zero, and
# uvcgpu_params_check refuses the setting.
IONTORRENT_NEGATIVE = dict(bq_phred_added_indel=-10, bq_phred_added_misma=-5, bias_thres_PFBQ1=25, bias_thres_PFBQ2=30)


def set_params(P, values):
    for k, v in (values or {}).items():
        assert hasattr(P, k), k
        setattr(P, k, v)
    return P


def zero_value_cells(reads, P, rtr, ip, baq, codes, prep, thres, proton):
    """The number of (fragment, position) pairs at which the fragment has an aligned base and its BASE consensus counts add up to 0, from the
    restated per-read walk (tests/p2_restatement.py read_events) merged per fragment as the fragment pass merges it -- no oracle value enters;
    and the number of aligned bases whose value is below 0."""
    n = int(reads["n_reads"])
    cells = below = 0
    i = 0
    while i < n:
        j = i
        while j < n and (reads["fam_id"][j], reads["fam_strand"][j], reads["frag_id"][j]) == (reads["fam_id"][i], reads["fam_strand"][i], reads["frag_id"][i]):
            j += 1
        best = {}
        for k in range(i, j):
            ev = read_events(reads, k, P, rtr, ip, baq, codes, prep, thres, proton, with_bias=False)[0]
            for _, v, p, s, _, _, _ in ev:
                if s <= 5:                                   # BASE_A .. BASE_NN
                    best[p] = max(best.get(p, 0), 0, v)      # the sum over the symbols is 0 exactly when the largest count is
                    below += v < 0
        cells += sum(1 for v in best.values() if v == 0)
        i = j
    return cells, int(below)


def simple_fragments_with_a_zero(reads, at_most=0):
    """Fragments of no more than two one-op alignments (the ones the closed forms of the fragment pass take) that hold an aligned base of
    quality `at_most` or less."""
    M = 0
    frag = np.asarray(reads["frag_id"]); n = int(reads["n_reads"])
    simple, low = {}, {}
    for k in range(n):
        f = (int(reads["fam_id"][k]), int(reads["fam_strand"][k]), int(frag[k]))
        one_op = int(reads["n_cigar"][k]) == 1 and (int(reads["cigars"][int(reads["cigar_off"][k])]) & 0xF) == M
        simple[f] = simple.get(f, 0) + (1 if one_op else 100)
        so, l = int(reads["seq_off"][k]), int(reads["l_qseq"][k])
        if one_op and (reads["quals"][so:so + l] <= at_most).any():
            low[f] = True
    return sum(1 for f in low if simple[f] <= 2)


def iontorrent_run_end_values_below_0(reads, add_b, add_l):
    """Aligned bases whose value is below 0 under the IonTorrent rule for the first and last base of an M run (main.hpp:1953-1975): the smaller of
    the base's quality and its inner neighbour's (1 where the read ends there), plus the smaller addend where the op next to it is shorter than 3,
    bq_phred_added_misma otherwise.  Restated from the columns alone; with add_b >= 0 no other base can have a value below 0."""
    assert add_b >= 0
    n = 0
    for k in range(int(reads["n_reads"])):
        co, nc, so, lq = int(reads["cigar_off"][k]), int(reads["n_cigar"][k]), int(reads["seq_off"][k]), int(reads["l_qseq"][k])
        cig = [(int(c) & 0xF, int(c) >> 4) for c in reads["cigars"][co:co + nc]]
        Q = reads["quals"][so:so + lq]
        qpos = 0
        for ci, (op, ln) in enumerate(cig):
            if op in (0, 7, 8):                                          # M = X
                for i2 in sorted({0, ln - 1}):
                    q = qpos + i2
                    inner = 1
                    if i2 != 0 and q + 1 < lq: inner = int(Q[q + 1])       # (sic: behind the first base the neighbour is the one after it,
                    if i2 == 0 and q > 0: inner = int(Q[q - 1])            # at the first base the one in front)
                    adj = 100
                    if i2 == ln - 1 and ci + 1 < nc: adj = min(adj, cig[ci + 1][1])
                    if i2 == 0 and ci > 0: adj = min(adj, cig[ci - 1][1])
                    n += min(int(Q[q]), inner) + (min(add_b, add_l) if adj < 3 else add_b) < 0
                qpos += ln
            elif op in (1, 4):                                           # I S
                qpos += ln
    return n
