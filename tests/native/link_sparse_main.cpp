// Host check of the sparse completion pass's rules in uvc_amd/csrc/uvc_link.h (tests/test_link_sparse_cpu.py builds this with
// -fsanitize=address,undefined and runs it), against a stub of the device side: the marks, the window list and its count in one buffer, a
// mark step that lists a window when it is the first to set its need byte, a sparse pass that walks the list and a dense pass that walks the marks.
//   1. uvc_link_slice: for every length 0..200, every W in {4, 8, 16} (W / 4 slices per class) and a few offsets the slices are contiguous, in
//      order, inside [lo, hi), cover it exactly once and differ in length by at most one;
//   2. layout: the count and the list lie behind link_done, aligned, inside uvc_link_buffer_bytes, which never shrinks when the region grows;
//   3. scopes: keys give POSITIONS, sites give POSITIONS, the ALL and NONE cases are those of uvc_link_score_scope;
//   4. the state machine of an accumulate with an early and a final INDEL phase, then POSITIONS (sparse and dense) and ALL: every window is
//      run at most once, and exactly once where somebody asked; the list never outgrows nwin.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../uvc_amd/csrc/uvc_link.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Stub {
    long long npos, nwin, ndblk; std::vector<uint8_t> buf; uint8_t *need, *done; int32_t *cnt, *list; std::vector<uint32_t> occ; std::vector<int> runs; int sparse_blocks = 0;
    explicit Stub(long long n) : npos(n), nwin((n + 63) / 64), ndblk((n + 4095) >> 12) {
        const size_t dirty = (size_t)3 * UVC_NUM_SYMBOLS * (size_t)ndblk;
        buf.assign(uvc_link_buffer_bytes(dirty, nwin), 0xAB);
        need = buf.data() + uvc_link_marks_off(dirty); done = need + uvc_link_marks_stride(nwin);
        cnt = (int32_t *)(buf.data() + uvc_link_list_cnt_off(dirty, nwin)); list = (int32_t *)(buf.data() + uvc_link_list_off(dirty, nwin));
        occ.assign((size_t)n, 0); runs.assign((size_t)nwin, 0);
    }
    void zero() { memset(buf.data(), 0, buf.size()); std::fill(runs.begin(), runs.end(), 0); }   // zero_state: one fill
    void ask(long long w) {   // k_link_mark: the first to set the need byte lists the window, unless the pass has been there
        if (need[w]) return;
        need[w] = 1;
        if (!done[w]) { const int i = (*cnt)++; if (i < nwin) list[i] = (int32_t)w; }
    }
    void mark(int scope, const std::vector<int> &xs) {
        if (scope == UVC_LINK_ALL) memset(need, 1, (size_t)nwin);
        else if (scope == UVC_LINK_POSITIONS) { for (int x : xs) if (x >= 0 && x < npos) ask(x >> 6); }
        else for (long long x = 0; x < npos; x++) if (uvc_link_occ_marks(occ[(size_t)x])) ask(x >> 6);
    }
    void sparse() {   // k_p2_link_sparse: the blocks stride over the list
        const int n = (*cnt < nwin ? *cnt : (int)nwin);
        for (int i = 0; i < n; i++) {
            const int w = list[i];
            if (w < 0 || w >= nwin) { CHECK(false, "list entry %d = %d outside the windows", i, w); continue; }
            if (uvc_link_window_runs(need[w], done[w])) { runs[(size_t)w]++; done[w] = 1; sparse_blocks++; }
        }
    }
    void dense() { for (long long w = 0; w < nwin; w++) if (uvc_link_window_runs(need[w], done[w])) { runs[(size_t)w]++; done[w] = 1; } }
    void launch(int scope, const std::vector<int> &xs, bool force_dense = false) {   // uvc_launch_link_complete
        mark(scope, xs);
        if (scope == UVC_LINK_ALL || force_dense || (scope == UVC_LINK_POSITIONS && uvc_link_positions_dense((int64_t)xs.size(), nwin))) dense(); else sparse();
    }
};

int main() {
    // 1. the slice rule
    for (int W : { 4, 8, 16 }) {
        const int ns = W / 4;
        for (int lo : { 0, 1, 63, 1000003 }) for (int len = 0; len <= 200; len++) {
            const int hi = lo + len;
            int at = lo, shortest = 1 << 30, longest = 0;
            for (int s = 0; s < ns; s++) {
                int a = -1, b = -1;
                uvc_link_slice(lo, hi, s, ns, &a, &b);
                CHECK(a == at && b >= a && a >= lo && b <= hi, "W %d [%d, %d) slice %d = [%d, %d), expected to begin at %d", W, lo, hi, s, a, b, at);
                at = b;
                if (b - a < shortest) shortest = b - a;
                if (b - a > longest) longest = b - a;
            }
            CHECK(at == hi, "W %d [%d, %d): the slices end at %d", W, lo, hi, at);
            CHECK(longest - shortest <= 1 && longest == (len + ns - 1) / ns, "W %d length %d: slices of %d to %d records", W, len, shortest, longest);
        }
        int a, b;
        uvc_link_slice(10, 5, ns - 1, ns, &a, &b);   // hi < lo (an empty class): an empty slice at lo
        CHECK(a == 10 && b == 10, "W %d: [10, 5) gives [%d, %d)", W, a, b);
    }
    // 2. layout
    const long long NPOS[11] = { 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1000001 };
    size_t prev_bytes = 0;
    for (long long npos : NPOS) {
        Stub s(npos);
        const size_t dirty = (size_t)3 * UVC_NUM_SYMBOLS * (size_t)s.ndblk;
        CHECK((uint8_t *)s.cnt == s.done + uvc_link_marks_stride(s.nwin) && uvc_link_list_cnt_off(dirty, s.nwin) % 8 == 0, "npos %lld: the count follows link_done, aligned", npos);
        CHECK((uint8_t *)s.list >= (uint8_t *)s.cnt + 4 && uvc_link_list_off(dirty, s.nwin) % 4 == 0, "npos %lld: the list follows the count", npos);
        CHECK((uint8_t *)(s.list + s.nwin) == s.buf.data() + s.buf.size(), "npos %lld: the list ends with the buffer", npos);
        CHECK(s.buf.size() >= prev_bytes, "npos %lld: the buffer shrank", npos);
        prev_bytes = s.buf.size();
        CHECK(uvc_link_buffer_bytes((size_t)3 * UVC_NUM_SYMBOLS * (size_t)((npos >> 12) + 2), s.nwin) >= s.buf.size(), "npos %lld: allocation too small", npos);
    }
    // 3. scopes
    CHECK(uvc_link_score_scope_at(0, 0, 0, 0, 0, 2) == UVC_LINK_NONE, "default gate");
    CHECK(uvc_link_score_scope_at(0, 0, 1, 5, 0, 2) == UVC_LINK_POSITIONS, "tumor keys");
    CHECK(uvc_link_score_scope_at(0, 0, 1, 0, 0, 2) == UVC_LINK_ALL, "a normal sample without keys");
    CHECK(uvc_link_score_scope_at(0, 0, 0, 0, 3, 2) == UVC_LINK_POSITIONS, "forced sites");
    for (int keys : { 0, 5 }) for (int sites : { 0, 3 }) for (int tn : { 0, 1 }) {
        CHECK(uvc_link_score_scope_at(1, 0, tn, keys, sites, 2) == UVC_LINK_ALL && uvc_link_score_scope_at(0, 1, tn, keys, sites, 2) == UVC_LINK_ALL, "-A with %d keys, %d sites", keys, sites);
        CHECK(uvc_link_score_scope_at(0, 0, tn, keys, sites, 0) == UVC_LINK_ALL && uvc_link_score_scope_at(0, 0, tn, keys, sites, -1) == UVC_LINK_ALL, "min_altdp_thres <= 0 with %d keys, %d sites", keys, sites);
        // never narrower than a request needs, never wider than the scope without positions
        const int old = uvc_link_score_scope(0, 0, tn, sites, 2), now = uvc_link_score_scope_at(0, 0, tn, keys, sites, 2);
        CHECK((old == UVC_LINK_NONE) == (now == UVC_LINK_NONE) && now <= old, "tn %d keys %d sites %d: scope %d, was %d", tn, keys, sites, now, old);
    }
    CHECK(uvc_link_positions_dense(0, 1000) == false && uvc_link_positions_dense(249, 1000) == false && uvc_link_positions_dense(250, 1000) == true, "the limit of the dense form");
    // 4. the state machine
    for (long long npos : { 65LL, 257LL, 4097LL, 100001LL }) {
        Stub s(npos);
        UvcLinkState link;
        const long long last = (npos - 1) >> 6;
        for (int round = 0; round < 3; round++) {
            s.zero(); link.planes_zeroed();
            std::fill(s.occ.begin(), s.occ.end(), 0u);
            // the CIGAR walk's marks exist at the early phase
            s.occ[0] = 1u << UVC_LINK_I1; s.occ[1] = 1u << UVC_LINK_D1; s.occ[(size_t)npos - 1] = 1u << UVC_LINK_D2; if (npos > 200) s.occ[130] = 1u << UVC_LINK_M;
            s.launch(UVC_LINK_INDEL, {});
            long long early = 0; for (int v : s.runs) early += v;
            CHECK(early == (last ? 2 : 1) && s.runs[0] == 1 && s.runs[(size_t)last] == 1, "npos %lld: the early phase ran %lld windows", npos, early);
            // the fragment and family kernels add marks: in a window already run, and in a new one
            s.occ[5] = 1u << UVC_LINK_I2; if (last >= 1) s.occ[64] = 1u << UVC_LINK_NN;
            s.launch(UVC_LINK_INDEL, {});
            link.accumulated(false);
            long long total = 0; for (int v : s.runs) total += v;
            CHECK(total == early + (last >= 2 ? 1 : 0) &&(last < 1 || s.runs[1] == 1), "npos %lld: the final phase left %lld windows run", npos, total);
            const int blocks = s.sparse_blocks;
            s.launch(UVC_LINK_INDEL, {});   // nothing new: no block does anything
            CHECK(s.sparse_blocks == blocks, "npos %lld: a third phase ran %d windows", npos, s.sparse_blocks - blocks);
            // POSITIONS twice (duplicates, out-of-range entries), sparse then dense, then ALL
            if (link.wants(true, false, UVC_LINK_POSITIONS)) { s.launch(UVC_LINK_POSITIONS, { 63, 64, 63, -5, (int)npos, (int)npos + 70, 0 }); link.enqueued(UVC_LINK_POSITIONS); }
            if (link.wants(true, false, UVC_LINK_POSITIONS)) { s.launch(UVC_LINK_POSITIONS, { 63, 64, 63, -5, (int)npos, (int)npos + 70, 0 }); link.enqueued(UVC_LINK_POSITIONS); }
            if (link.wants(true, false, UVC_LINK_POSITIONS)) { s.launch(UVC_LINK_POSITIONS, { 129, 64 }, true); link.enqueued(UVC_LINK_POSITIONS); }
            CHECK(s.runs[0] == 1 && (last < 1 || s.runs[1] == 1) && (last < 2 || s.runs[2] == 1), "npos %lld: POSITIONS", npos);
            CHECK(*s.cnt <= s.nwin, "npos %lld: %d windows listed of %lld", npos, *s.cnt, s.nwin);
            if (link.wants(true, false, UVC_LINK_ALL)) { s.launch(UVC_LINK_ALL, {}); link.enqueued(UVC_LINK_ALL); }
            CHECK(!link.wants(true, false, UVC_LINK_POSITIONS) && !link.wants(true, false, UVC_LINK_ALL), "npos %lld: a pass behind ALL", npos);
            for (long long w = 0; w < s.nwin; w++) CHECK(s.runs[(size_t)w] == 1, "npos %lld round %d: window %lld ran %d times", npos, round, w, s.runs[(size_t)w]);
        }
        // every window asked for one by one: the list holds each once and never outgrows nwin
        s.zero();
        std::vector<int> xs;
        for (int rep = 0; rep < 3; rep++) { for (long long x = 0; x < npos; x += 17) xs.push_back((int)x); xs.push_back((int)npos - 1); }
        s.mark(UVC_LINK_POSITIONS, xs); s.sparse(); s.mark(UVC_LINK_POSITIONS, xs); s.sparse();
        CHECK(*s.cnt == s.nwin, "npos %lld: %d windows listed of %lld", npos, *s.cnt, s.nwin);
        for (long long w = 0; w < s.nwin; w++) CHECK(s.runs[(size_t)w] == 1, "npos %lld, every window: window %lld ran %d times", npos, w, s.runs[(size_t)w]);
    }
    printf("sparse link rules: %d failures\n", failures);
    return failures ? 1 : 0;
}
