// Host run of uvc_amd/csrc/uvc_hap.cpp (tests/test_hap_host_cpu.py builds this with -fsanitize=undefined,address and runs it): reads a file
// of cases, calls uvc_hap_build on each event buffer and uvc_hap_phase_string for every (position, symbol) that occurs in it, and prints
// the links and strings as text.  The expectation lives in Python (tests/hap_restatement.py); nothing is judged here.
//   input:   n_cases, then per case "beg npos max_count min_ad max_detail_cnt n_ints" and n_ints event words (uvc_hap.h: the device's format)
//   output:  "case <i>", per link "L <level> <fw> <rv> <other fw> <other rv> <n> (<pos> <symbol>) x n" in vector order, per (level, position,
//            symbol) with a non-empty string "S <level> <pos> <symbol> <string>", then "end <i>"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "../../uvc_amd/csrc/uvc_hap.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    long n_cases = 0;
    if (fscanf(fh, "%ld", &n_cases) != 1) return 2;
    for (long c = 0; c < n_cases; c++) {
        long beg, npos, max_count, min_ad, max_detail_cnt, n_ints;
        if (fscanf(fh, "%ld %ld %ld %ld %ld %ld", &beg, &npos, &max_count, &min_ad, &max_detail_cnt, &n_ints) != 6) return 2;
        std::vector<int32_t> ev((size_t)n_ints);
        for (long k = 0; k < n_ints; k++) { long v; if (fscanf(fh, "%ld", &v) != 1) return 2; ev[(size_t)k] = (int32_t)v; }
        std::vector<UvcHapLinkHost> out[3];
        uvc_hap_build(ev.data(), (int64_t)n_ints, (int32_t)beg, (int64_t)npos, (int32_t)max_count, (int32_t)min_ad, (int32_t)max_detail_cnt, out);
        printf("case %ld\n", c);
        for (int w = 0; w < 3; w++) for (const UvcHapLinkHost &h : out[w]) {
            printf("L %d %d %d %d %d %zu", w, h.fr[0], h.fr[1], h.other[0], h.other[1], h.form.size());
            for (const auto &ps : h.form) printf(" %d %d", ps.first, ps.second);
            printf("\n");
        }
        std::set<std::pair<int32_t, int32_t>> seen;   // every (position, symbol) of every slot, whatever its kind and count
        for (int64_t at = 0; at + 2 <= n_ints;) {
            const int32_t head = ev[(size_t)at], count = ev[(size_t)at + 1];
            if (head < 0) break;
            for (int32_t k = 0; k < count; k++) { const int32_t word = ev[(size_t)(at + 2 + k)]; seen.insert(std::make_pair((int32_t)beg + (word >> 4), word & 15)); }
            at += 2 + (head >> 8);
        }
        for (int w = 0; w < 3; w++) for (const auto &ps : seen) {
            const std::string s = uvc_hap_phase_string(out[w], ps.first, ps.second);
            if (!s.empty()) printf("S %d %d %d %s\n", w, ps.first, ps.second, s.c_str());
        }
        printf("end %ld\n", c);
    }
    fclose(fh);
    return 0;
}
