// TEST INFRASTRUCTURE -- NOT PART OF THE PRODUCT.
// C wrapper around the reference's own math headers (main_conversion.hpp, main_consensus.hpp, the macros of common.hpp), which compile
// without htslib once oracle/ref_shim/ stands in for the two htslib headers they include.  Built by `make -C oracle ref_math` from the
// sources where they lie, into oracle/_ref/libref_math.so: everything the functions below reach is REFERENCE code.
// tests/test_ref_math_cpu.py pins the oracle's primitives on it bit for bit; tests/test_gpu_math_probe.py the device's.
//
// Every math wrapper has one shape: n rows of `in` (row-major, the arguments in the reference's order, integers carried as doubles)
// give n rows of `out`, so a whole grid costs one call.
#include "main_conversion.hpp"
#include "main_consensus.hpp"

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#define ROWS(n_in, n_out) for (int64_t i = 0; i < n; i++) { const double *a = in + i * (n_in); double *o = out + i * (n_out); (void)a; (void)o;
#define END_ROWS }

extern "C" {
// ---- common.hpp:82-88, 188-200 ----
void ref_phred2nat(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = phred2nat(a[0]); END_ROWS }
void ref_numstates2phred(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = numstates2phred(a[0]); END_ROWS }
void ref_numstates2deciphred(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = (double)numstates2deciphred(a[0]); END_ROWS }
void ref_non_neg_minus(int64_t n, const double *in, double *out) { ROWS(2, 1) o[0] = (double)non_neg_minus(a[0], a[1]); END_ROWS }
void ref_non_neg_minus_i64(int64_t n, const double *in, double *out) { ROWS(2, 1) o[0] = (double)non_neg_minus((int64_t)a[0], (int64_t)a[1]); END_ROWS }
void ref_mathsquare(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = mathsquare(a[0]); END_ROWS }
// ---- main_conversion.hpp ----
void ref_mathcube(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = mathcube(a[0]); END_ROWS }
void ref_prob2odds(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = prob2odds(a[0]); END_ROWS }
void ref_odds2prob(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = odds2prob(a[0]); END_ROWS }
void ref_logit(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = logit(a[0]); END_ROWS }
void ref_logit2(int64_t n, const double *in, double *out) { ROWS(2, 1) o[0] = logit2(a[0], a[1]); END_ROWS }
// prob, a, b, TIsBiDirectional, TSetMaxProbToOne
void ref_binom_llr(int64_t n, const double *in, double *out) {
    ROWS(5, 1)
        const bool bidir = (a[3] != 0), maxone = (a[4] != 0);
        o[0] = bidir ? (maxone ? calc_binom_10log10_likeratio<true, true>(a[0], a[1], a[2]) : calc_binom_10log10_likeratio<true, false>(a[0], a[1], a[2]))
                     : (maxone ? calc_binom_10log10_likeratio<false, true>(a[0], a[1], a[2]) : calc_binom_10log10_likeratio<false, false>(a[0], a[1], a[2]));
    END_ROWS
}
// TBidirectional, TIsOverseqFracDisabled, then the eleven arguments in order
void ref_dp4(int64_t n, const double *in, double *out) {
    ROWS(13, 2)
        const bool bidir = (a[0] != 0), dis = (a[1] != 0);
        const double *b = a + 2;
#define DP4_ARGS b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9], b[10]
        const std::array<double, 2> r = bidir ? (dis ? dp4_to_pcFA<true, true>(DP4_ARGS) : dp4_to_pcFA<true, false>(DP4_ARGS))
                                              : (dis ? dp4_to_pcFA<false, true>(DP4_ARGS) : dp4_to_pcFA<false, false>(DP4_ARGS));
#undef DP4_ARGS
        o[0] = r[0]; o[1] = r[1];
    END_ROWS
}
// v; a NaN base asks for the defaults (base = pow(10, 0.1), thres = 10)
void ref_calc_non_negative(int64_t n, const double *in, double *out) { ROWS(3, 1) o[0] = (a[1] != a[1]) ? calc_non_negative<double>(a[0]) : calc_non_negative<double>(a[0], a[1], a[2]); END_ROWS }
// the instantiation of the one call site, main.hpp:6206: T = float, defaults
void ref_calc_non_negative_float(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = (double)calc_non_negative<float>((float)a[0]); END_ROWS }
void ref_calc_score_with_penal_at_low_val(int64_t n, const double *in, double *out) { ROWS(3, 1) o[0] = calc_score_with_penal_at_low_val<double>(a[0], a[1], a[2]); END_ROWS }
void ref_phred2prob(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = phred2prob((uvc1_qual_t)a[0]); END_ROWS }
void ref_prob2phred(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = (double)prob2phred(a[0]); END_ROWS }
void ref_prob2realphred(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = prob2realphred(a[0]); END_ROWS }
void ref_proton_cigarlen2phred(int64_t n, const double *in, double *out) { ROWS(1, 1) o[0] = (double)proton_cigarlen2phred((uint32_t)a[0]); END_ROWS }
// 16 bucket counts, max_qual, dec_qual, totDP -> maxvqual, argmaxAD, argmaxBQ
void ref_infer_max_qual(int64_t n, const double *in, double *out) {
    ROWS(19, 3)
        std::array<int, NUM_BUCKETS> distr;
        for (int k = 0; k < NUM_BUCKETS; k++) distr[k] = (int)a[k];
        uvc1_qual_t maxvqual = 0, argmaxBQ = 0; uvc1_readnum_t argmaxAD = 0;
        infer_max_qual_assuming_independence<int>(maxvqual, argmaxAD, argmaxBQ, (uvc1_qual_t)a[16], (uvc1_qual_t)a[17], distr, (uvc1_readnum_t)a[18], 0);
        o[0] = maxvqual; o[1] = argmaxAD; o[2] = argmaxBQ;
    END_ROWS
}
// the same for a histogram with one bucket filled: bucket index, its count, max_qual, dec_qual, totDP
void ref_infer_max_qual_one(int64_t n, const double *in, double *out) {
    ROWS(5, 3)
        std::array<int, NUM_BUCKETS> distr;
        for (int k = 0; k < NUM_BUCKETS; k++) distr[k] = (k == (int)a[0]) ? (int)a[1] : 0;
        uvc1_qual_t maxvqual = 0, argmaxBQ = 0; uvc1_readnum_t argmaxAD = 0;
        infer_max_qual_assuming_independence<int>(maxvqual, argmaxAD, argmaxBQ, (uvc1_qual_t)a[2], (uvc1_qual_t)a[3], distr, (uvc1_readnum_t)a[4], 0);
        o[0] = maxvqual; o[1] = argmaxAD; o[2] = argmaxBQ;
    END_ROWS
}
void ref_symbols_mutated(int64_t n, const double *in, double *out) { ROWS(2, 1) o[0] = areSymbolsMutated((AlignmentSymbol)(int)a[0], (AlignmentSymbol)(int)a[1]) ? 1 : 0; END_ROWS }
// symbol -> isSymbolIns, isSymbolDel, isSymbolSubstitution
void ref_symbol_kind(int64_t n, const double *in, double *out) {
    ROWS(1, 3) const AlignmentSymbol s = (AlignmentSymbol)(int)a[0]; o[0] = isSymbolIns(s) ? 1 : 0; o[1] = isSymbolDel(s) ? 1 : 0; o[2] = isSymbolSubstitution(s) ? 1 : 0; END_ROWS
}
// length -> insLenToSymbol, delLenToSymbol
void ref_len_to_symbol(int64_t n, const double *in, double *out) {
    char qname[2] = "q";
    bam1_t b; b.core.tid = 0; b.core.pos = 0; b.qname_ = qname;
    ROWS(1, 2) o[0] = (double)insLenToSymbol((uvc1_readpos_t)a[0], &b); o[1] = (double)delLenToSymbol((uvc1_readpos_t)a[0], &b); END_ROWS
}
// op, oplen -> qpos and rpos after the call from (0, 0), and the value thrown (0: none)
void ref_process_cigar(int64_t n, const double *in, double *out) {
    ROWS(2, 3)
        int64_t qpos = 0, rpos = 0; int thrown = 0;
        try { process_cigar(qpos, rpos, (uint32_t)a[0], (uint32_t)a[1]); } catch (int e) { thrown = e; }
        o[0] = (double)qpos; o[1] = (double)rpos; o[2] = thrown;
    END_ROWS
}
// common.hpp:133-138
void ref_sequencing_platforms(int32_t *out4) { out4[0] = SEQUENCING_PLATFORM_AUTO; out4[1] = SEQUENCING_PLATFORM_ILLUMINA; out4[2] = SEQUENCING_PLATFORM_IONTORRENT; out4[3] = SEQUENCING_PLATFORM_OTHER; }
// CHAR_TO_SYMBOL.data (128 entries)
void ref_char_to_symbol(int32_t *out128) { for (int c = 0; c < 128; c++) out128[c] = (int32_t)CHAR_TO_SYMBOL.data[c]; }

// ---- main_consensus.hpp: ConsensusBlockSet as one (family, strand) unit uses it ----
// The events of the unit's reads -- (fragment index, ConsensusBlockCigarType, position, bases as text, qualities) in read order, as
// updateByRead1Aln hands them to incByPosSeqQual (main.hpp:2115, 2279; the first-op clip already reversed) -- go fragment by fragment
// into block sets of their own, and every fragment's sets are folded into the family's with incByMajorMinusMinor (main.hpp:1722).
// fragment_level != 0: no folding, the one fragment's own sets are returned.  Blocks come out by (type, position): out_blocks[4 * k] =
// type, position, rows, first row; rows of 8 int32.  Returns the number of blocks, or -1 where a capacity is too small.
int64_t ref_conblock_unit(int64_t n_events, const int32_t *ev_frag, const int32_t *ev_type, const int32_t *ev_pos, const int64_t *ev_off, const int32_t *ev_len,
                          const char *seq, const int8_t *qual, int fragment_level, int32_t *out_blocks, int64_t block_capacity, int32_t *out_rows, int64_t row_capacity) {
    std::array<ConsensusBlockSet, NUM_CONSENSUS_BLOCK_CIGAR_TYPES> fam, frag;
    auto fold = [&]() { for (size_t t = 0; t < fam.size(); t++) { fam[t].incByMajorMinusMinor(frag[t]); frag[t] = ConsensusBlockSet(); } };
    for (int64_t e = 0; e < n_events; e++) {
        if (e > 0 && ev_frag[e] != ev_frag[e - 1] && !fragment_level) fold();
        const std::string s(seq + ev_off[e], seq + ev_off[e] + ev_len[e]);
        const std::vector<int8_t> q(qual + ev_off[e], qual + ev_off[e] + ev_len[e]);
        frag[ev_type[e]].incByPosSeqQual(ev_pos[e], s, q);
    }
    if (!fragment_level && n_events > 0) fold();
    const auto &res = (fragment_level ? frag : fam);
    int64_t nb = 0, nr = 0;
    for (size_t t = 0; t < res.size(); t++) for (const auto &pb : res[t].pos2conblock) {
        if (nb >= block_capacity || nr + (int64_t)pb.second.size() > row_capacity) return -1;
        out_blocks[4 * nb] = (int32_t)t; out_blocks[4 * nb + 1] = pb.first; out_blocks[4 * nb + 2] = (int32_t)pb.second.size(); out_blocks[4 * nb + 3] = (int32_t)nr;
        for (const auto &row : pb.second) { for (int k = 0; k < 8; k++) out_rows[8 * nr + k] = row[k]; nr++; }
        nb++;
    }
    return nb;
}
// consensusBlockToSeqQual of a block (rows of 8 int32), after ConsensusBlock_trim where trim_perc_dp >= 0; out4 = base, quality, family_size,
// family_identity per element; returns the number of elements
int32_t ref_conblock_to_seq(const int32_t *rows, int32_t len, int32_t right_to_left, int32_t trim_perc_dp, int32_t trim_n_consec, int32_t *out4) {
    ConsensusBlock cb;
    for (int32_t i = 0; i < len; i++) { BaseToCount r; for (int k = 0; k < 8; k++) r[k] = rows[8 * i + k]; cb.push_back(r); }
    const FastqConsensusSeqSegment s = consensusBlockToSeqQual(trim_perc_dp >= 0 ? ConsensusBlock_trim(cb, trim_perc_dp, trim_n_consec) : cb, right_to_left != 0);
    for (size_t i = 0; i < s.size(); i++) { out4[4 * i] = s[i].base; out4[4 * i + 1] = s[i].quality; out4[4 * i + 2] = s[i].family_size; out4[4 * i + 3] = s[i].family_identity; }
    return (int32_t)s.size();
}
}
