// uvc_rules.h -- the pure integer rules of the reference that more than one kernel, or a kernel and host code, apply: each one once.
// No memory access and no HIP type in here, so the same text compiles for the host (uvc_conblock.cpp, uvc_prep.hip's host side and
// tests/native/rules_host_main.cpp, which checks the pair rules against the generic consensus they stand in for) and, force-inlined, into
// the kernels (uvc_device.h includes it).
#ifndef UVC_RULES_H
#define UVC_RULES_H

#include <stdint.h>
#include "uvcgpu.h"
#if defined(__HIPCC__)
#define UVC_RULE __host__ __device__ inline __attribute__((always_inline))
#else
#define UVC_RULE inline
#endif
UVC_RULE int imin(int a, int b) { return a < b ? a : b; }
UVC_RULE int imax(int a, int b) { return a > b ? a : b; }

// ---- a read base as the kernels fetch it: base | qual << 8 (RegionDev::bq) ----
UVC_RULE int bq_sym(int x) { return x & 0xFF; }
UVC_RULE int bq_qual(int x) { return (x >> 8) & 0xFF; }
UVC_RULE int base_value(int q, const UvcParams &P) { return q + P.bq_phred_added_misma; }   // what a base of quality q adds to its symbol (not IonTorrent)
// The quality at or below which a base has no value (on IonTorrent the smaller of two qualities + the smaller addend): a fragment with
// such a base takes the per-position kernels (FRAG_STAT_ZERO_VALUE)
UVC_RULE int zero_value_qual(const UvcParams &P) { return -((UVC_PLATFORM_IONTORRENT == P.inferred_sequencing_platform) ? imin(P.bq_phred_added_misma, P.bq_phred_added_indel) : P.bq_phred_added_misma); }
// ---- RegionDev::dirty: A C G T N (a reference base) and LINK_M are written at nearly every position, so their planes are zero-filled without a look at the marks ----
UVC_RULE bool sym_always_filled(int s) { return s < UVC_BASE_NN || s == UVC_LINK_M; }
// ---- assay predicates.  UvcReadSoA::fam_dflag bits (MolecularBarcode::duplexflag, grouping.cpp:931) ----
enum { UVC_DFLAG_UMI = 0x1, UVC_DFLAG_DUPLEX = 0x2, UVC_DFLAG_AMPLICON = 0x4 };
UVC_RULE bool normal_filters_primers(const UvcParams &P) { return P.tn_is_paired && (0x1 & P.primer_flag); }
UVC_RULE bool is_assay_amplicon(int dflag, const UvcParams &P) { return (dflag & UVC_DFLAG_AMPLICON) || ((P.primerlen > 0) && !(0x2 & P.primer_flag)); }
UVC_RULE bool amplicon_gated(int dflag, const UvcParams &P) { return is_assay_amplicon(dflag, P) && !normal_filters_primers(P); }   // reads are gated by their primer window, main.hpp:1872-1875, 1895
UVC_RULE bool unit_may_be_good(int dflag, const UvcParams &P) { return (dflag & UVC_DFLAG_UMI) || (P.fam_flag & 0x2); }
UVC_RULE bool is_fam_good(int cc, int ct, int dflag, const UvcParams &P) { return (P.fam_thres_dup1add <= ct) && (cc * 100 >= ct * P.fam_thres_dup1perc) && unit_may_be_good(dflag, P); }   // main.hpp:2988-2989
// GenericSymbol2Count::_fillConsensusCounts<TIsRefCountedOnlyOnce>, main.hpp:374-402
template <class Arr>
UVC_RULE void fill_consensus(const Arr &c, int &argmax, int &cmax, int &csum, int st, bool ref_once_in_link, bool ignore_padded_del) {
    const int b = (st == UVC_BASE_SYMBOL ? UVC_BASE_A : UVC_LINK_M);
    const int e = (st == UVC_BASE_SYMBOL ? (ignore_padded_del ? UVC_BASE_T : UVC_BASE_NN) : UVC_LINK_NN);
    const bool once = (st == UVC_LINK_SYMBOL && ref_once_in_link);
    argmax = e; cmax = 0; csum = 0;
    for (int s = b; s <= e; s++) {
        const int v = c[s];
        if (once) {
            if (cmax < v || (UVC_LINK_M == argmax && (0 < v))) { argmax = s; cmax = v; csum = cmax; }
        } else {
            if (cmax < v) { argmax = s; cmax = v; }
            csum += v;
        }
    }
}

// ---- pair rules: a plain fragment (<= 2 simple alignments, every base of value 1 or more) at one position, in registers ----
// Base consensus of the two mates, written with selects (BASE_QUALITY_MAX merge, main.hpp:339-349): what fill_consensus gives over
// cnt[b] = max(cnt[b], value) per mate present -- (cs, cc, ct) over A..NN, (cs4, cc4, ct4) over A..T when padded deletions are ignored
// (fillConsensusCounts<false, true>, main.hpp:410), else the same again.  in0 / in1: the mate covers the position; bq0 / bq1: its base | qual << 8 (anything for a mate that does not)
struct PairCons { int cs, cc, ct, cs4, cc4, ct4; };
UVC_RULE PairCons pair_consensus_of(bool in0, bool in1, int b0, int b1, int v0, int v1, bool padded_ignored) {   // b: symbol, v: value (>= 1) of each mate
    const int A = (in0 ? v0 : 0), B = (in1 ? v1 : 0);
    const bool diff = (in0 && in1 && b0 != b1);
    const bool first = (v0 > v1) || (v0 == v1 && b0 < b1);
    PairCons c; c.cc = imax(A, B); c.ct = (diff ? A + B : c.cc);
    c.cs = ((in0 && (!diff || first)) ? b0 : b1);
    c.cs4 = c.cs; c.cc4 = c.cc; c.ct4 = c.ct;
    if (padded_ignored) {
        const int A4 = ((in0 && b0 <= UVC_BASE_T) ? v0 : 0), B4 = ((in1 && b1 <= UVC_BASE_T) ? v1 : 0);
        const bool first4 = (A4 > B4) || (A4 == B4 && b0 < b1);
        c.cc4 = imax(A4, B4); c.ct4 = (diff ? A4 + B4 : c.cc4);
        c.cs4 = ((A4 == 0 && B4 == 0) ? UVC_BASE_T : (diff ? (first4 ? b0 : b1) : c.cs));
    }
    return c;
}
UVC_RULE PairCons pair_consensus(bool in0, bool in1, int bq0, int bq1, const UvcParams &P, bool padded_ignored) {
    return pair_consensus_of(in0, in1, bq_sym(bq0), bq_sym(bq1), base_value(bq_qual(bq0), P), base_value(bq_qual(bq1), P), padded_ignored);
}
// LINK_M value of the better mate (main.hpp:1919-1923): lk0 / lk1: the mate has a link at the position (from the second base of a run on);
// noindel80: the position's InDel phred capped at 80; nogap: the mate's micro_nogap_penal.  0: no link.
UVC_RULE int link_better_mate(bool lk0, bool lk1, int noindel80, int nogap0, int nogap1) { return imax(lk0 ? imax(noindel80 - nogap0, 0) + 1 : 0, lk1 ? imax(noindel80 - nogap1, 0) + 1 : 0); }
#endif
