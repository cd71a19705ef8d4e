// Host check of uvc_amd/csrc/uvc_rules.h (tests/test_rules_cpu.py builds this with -fsanitize=undefined and runs it).
//   1. pair_consensus against the generic path it stands in for: cnt[b] = max(cnt[b], value) per mate present, then fill_consensus over
//      A..NN, and over A..T when padded deletions are ignored.  Presence {0 only, 1 only, both} x b0, b1 in 0..4 x padded_ignored 0 / 1 x
//      values {1, 2, 3, 40, 41, 255, 300} per mate = 7 350 cases.  Values of 1 or more only: a fragment with a base of value 0 or less
//      never reaches the pair form (FRAG_STAT_ZERO_VALUE), and there the two forms differ by design.  A mate that is absent keeps its
//      symbol and value in the call (the kernels pass whatever bytes they fetched for it); the generic path does not look at them.
//      The packed form (base | qual << 8 + bq_phred_added_misma) is held against the value form wherever one addend expresses both values
//      with 8-bit qualities.
//   2. zero_value_qual for both platforms and addends of both signs.
//   3. is_fam_good at the fam_thres_dup1perc / fam_thres_dup1add boundaries and for the three sources of unit_may_be_good.
#include <cstdio>
#include <cstring>
#include "../../uvc_amd/csrc/uvc_rules.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static UvcParams params() { UvcParams P; memset(&P, 0, sizeof(P)); P.struct_size = (int32_t)sizeof(P); return P; }

static int check_pair_consensus() {
    static const int values[7] = { 1, 2, 3, 40, 41, 255, 300 };
    int n = 0, n_packed = 0;
    for (int presence = 0; presence < 3; presence++) for (int b0 = 0; b0 <= 4; b0++) for (int b1 = 0; b1 <= 4; b1++) for (int pad = 0; pad < 2; pad++)
    for (int i0 = 0; i0 < 7; i0++) for (int i1 = 0; i1 < 7; i1++) {
        const bool in0 = (presence != 1), in1 = (presence != 0);
        const int v0 = values[i0], v1 = values[i1];
        int cnt[UVC_NUM_SYMBOLS] = { 0 };
        if (in0) cnt[b0] = imax(cnt[b0], v0);
        if (in1) cnt[b1] = imax(cnt[b1], v1);
        int cs, cc, ct, cs4, cc4, ct4;
        fill_consensus(cnt, cs, cc, ct, UVC_BASE_SYMBOL, false, false);
        fill_consensus(cnt, cs4, cc4, ct4, UVC_BASE_SYMBOL, false, pad != 0);
        const PairCons c = pair_consensus_of(in0, in1, b0, b1, v0, v1, pad != 0);
        const bool ok = (c.cc == cc && c.ct == ct && c.cc4 == cc4 && c.ct4 == ct4 && (ct == 0 || c.cs == cs) && (ct4 == 0 || c.cs4 == cs4));
        CHECK(ok, "presence %d b %d %d pad %d values %d %d: pair (%d %d %d | %d %d %d) generic (%d %d %d | %d %d %d)", presence, b0, b1, pad, v0, v1,
              c.cs, c.cc, c.ct, c.cs4, c.cc4, c.ct4, cs, cc, ct, cs4, cc4, ct4);
        n++;
        const int add = imax(0, imax(v0, v1) - 255);
        if (imin(v0, v1) - add >= 0) {
            UvcParams P = params(); P.bq_phred_added_misma = add;
            const PairCons d = pair_consensus(in0, in1, b0 | ((v0 - add) << 8), b1 | ((v1 - add) << 8), P, pad != 0);
            CHECK(d.cs == c.cs && d.cc == c.cc && d.ct == c.ct && d.cs4 == c.cs4 && d.cc4 == c.cc4 && d.ct4 == c.ct4, "packed form, presence %d b %d %d pad %d values %d %d", presence, b0, b1, pad, v0, v1);
            n_packed++;
        }
    }
    CHECK(n_packed == 5850, "%d", n_packed);   // all but 300 beside a value below 45: 10 of the 49 value pairs
    return n;
}

static int check_zero_value_qual() {
    static const int addends[6][2] = { { 0, 0 }, { 5, -3 }, { -5, 3 }, { -7, -2 }, { 4, 9 }, { -256, 3840 } };   // (misma, indel)
    int n = 0;
    for (const auto &a : addends) {
        UvcParams P = params(); P.bq_phred_added_misma = a[0]; P.bq_phred_added_indel = a[1];
        P.inferred_sequencing_platform = UVC_PLATFORM_ILLUMINA;
        CHECK(zero_value_qual(P) == -a[0], "illumina %d %d: %d", a[0], a[1], zero_value_qual(P));
        P.inferred_sequencing_platform = UVC_PLATFORM_IONTORRENT;
        CHECK(zero_value_qual(P) == -(a[0] < a[1] ? a[0] : a[1]), "iontorrent %d %d: %d", a[0], a[1], zero_value_qual(P));
        n += 2;
    }
    return n;
}

static int check_is_fam_good() {
    UvcParams P = params(); P.fam_thres_dup1add = 2; P.fam_thres_dup1perc = 80;
    int n = 0;
    // (cc, ct, dflag, fam_flag) -> expected
    static const int cases[][5] = {
        { 4, 5, UVC_DFLAG_UMI, 0, 1 }, { 3, 5, UVC_DFLAG_UMI, 0, 0 },       // 80 % of 5 is 4
        { 8, 10, UVC_DFLAG_UMI, 0, 1 }, { 7, 10, UVC_DFLAG_UMI, 0, 0 },
        { 799, 1000, UVC_DFLAG_UMI, 0, 0 }, { 800, 1000, UVC_DFLAG_UMI, 0, 1 },
        { 1, 1, UVC_DFLAG_UMI, 0, 0 }, { 2, 2, UVC_DFLAG_UMI, 0, 1 },       // fam_thres_dup1add <= ct
        { 5, 5, 0, 0, 0 }, { 5, 5, UVC_DFLAG_DUPLEX | UVC_DFLAG_AMPLICON, 0, 0 }, { 5, 5, 0, 0x1, 0 },   // no UMI and fam_flag & 0x2 not set
        { 5, 5, 0, 0x2, 1 }, { 5, 5, UVC_DFLAG_UMI | UVC_DFLAG_AMPLICON, 0, 1 },
    };
    for (const auto &c : cases) {
        P.fam_flag = c[3];
        CHECK((is_fam_good(c[0], c[1], c[2], P) ? 1 : 0) == c[4], "cc %d ct %d dflag %d fam_flag %d", c[0], c[1], c[2], c[3]);
        CHECK(unit_may_be_good(c[2], P) == (((c[2] & 0x1) || (c[3] & 0x2)) ? true : false), "dflag %d fam_flag %d", c[2], c[3]);
        n++;
    }
    return n;
}

int main() {
    const int n_pair = check_pair_consensus(), n_zero = check_zero_value_qual(), n_good = check_is_fam_good();
    printf("pair_consensus %d cases, zero_value_qual %d, is_fam_good %d, %d failures\n", n_pair, n_zero, n_good, failures);
    return failures ? 1 : 0;
}
