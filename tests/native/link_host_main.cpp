// Host check of uvc_amd/csrc/uvc_link.h (tests/test_link_lazy_cpu.py builds this with -fsanitize=undefined,address and runs it): the rules
// of the lazy completion of LINK_M against a stub of the device side -- two byte arrays and a pass that walks them the way the kernel does.
//   1. layout of the marks for npos in {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1 000 001}: need and done disjoint from the dirty
//      marks and from each other, 4-byte aligned, long enough for the word reads of the wave-per-window form (4 windows per block of 256
//      positions), inside uvc_link_marks_bytes, which never shrinks when the region grows (a handle keeps its buffer for shorter regions);
//   2. which entry asks for which scope;
//   3. the state machine: INDEL at the end of an accumulate, POSITIONS, ALL, each window run exactly once per accumulate whatever the order of
//      the calls, nothing enqueued after ALL, everything again after the planes were zeroed, nothing on released planes or before an accumulate.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../uvc_amd/csrc/uvc_link.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the device side: the marks buffer of a handle and what the kernels do to it
struct Stub {
    long long npos, nwin, ndblk; std::vector<uint8_t> buf; uint8_t *need, *done; std::vector<uint32_t> occ; std::vector<int> runs; int launches = 0;
    explicit Stub(long long n) : npos(n), nwin((n + 63) / 64), ndblk((n + 4095) >> 12) {
        const size_t dirty = (size_t)3 * UVC_NUM_SYMBOLS * (size_t)ndblk;
        buf.assign(uvc_link_marks_bytes(dirty, nwin), 0xAB);
        need = buf.data() + uvc_link_marks_off(dirty); done = need + uvc_link_marks_stride(nwin);
        occ.assign((size_t)n, 0); runs.assign((size_t)nwin, 0);
    }
    void zero() { memset(buf.data(), 0, buf.size()); }   // zero_state: one fill over the dirty marks and both arrays
    void pass() {   // k_p2_fast<true, false>, wave-per-window form: a block per 256 positions reads its four windows as one word
        launches++;
        for (long long b = 0; b < (npos + 255) / 256; b++) {
            uint32_t nd, dn; memcpy(&nd, need + 4 * b, 4); memcpy(&dn, done + 4 * b, 4);
            if (!(nd & ~dn & 0x01010101u)) continue;
            for (long long w = 4 * b; w < 4 * b + 4 && w < nwin; w++) if (uvc_link_window_runs(need[w], done[w])) { runs[(size_t)w]++; done[w] = 1; }
        }
    }
    void launch(int scope, const std::vector<int> &xs) {   // uvc_launch_link_complete
        if (scope == UVC_LINK_ALL) memset(need, 1, (size_t)nwin);
        else if (scope == UVC_LINK_POSITIONS) { for (int x : xs) if (x >= 0 && x < npos) need[x >> 6] = 1; }
        else for (long long x = 0; x < npos; x++) if (uvc_link_occ_marks(occ[(size_t)x])) need[x >> 6] = 1;
        pass();
    }
};
// the host side: link_complete of uvc_host.cpp
struct Handle {
    Stub &d; UvcLinkState link; bool accumulated = false, released = false;
    explicit Handle(Stub &s) : d(s) {}
    void accumulate(bool eager) { d.zero(); link.planes_zeroed(); std::fill(d.runs.begin(), d.runs.end(), 0); d.launch(eager ? UVC_LINK_ALL : UVC_LINK_INDEL, {}); link.accumulated(eager); accumulated = true; released = false; }
    void read(int scope, const std::vector<int> &xs = {}) { if (!link.wants(accumulated, released, scope)) return; d.launch(scope, xs); link.enqueued(scope); }
};

int main() {
    const long long NPOS[11] = { 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1000001 };
    size_t prev_bytes = 0;
    for (long long npos : NPOS) {
        Stub s(npos);
        const size_t dirty = (size_t)3 * UVC_NUM_SYMBOLS * (size_t)s.ndblk, stride = uvc_link_marks_stride(s.nwin);
        CHECK(uvc_link_marks_off(dirty) >= dirty && uvc_link_marks_off(dirty) % 8 == 0 && stride % 8 == 0, "npos %lld: alignment", npos);
        CHECK(stride >= (size_t)(4 * ((npos + 255) / 256)), "npos %lld: stride %zu shorter than the word reads", npos, stride);
        CHECK(s.done + stride == s.buf.data() + s.buf.size(), "npos %lld: the arrays end with the buffer", npos);
        CHECK(s.buf.size() >= prev_bytes, "npos %lld: the buffer shrank", npos);
        prev_bytes = s.buf.size();
        // the allocation of configure_region: for the longest region a handle has seen, with its bound of the dirty blocks
        CHECK(uvc_link_marks_bytes((size_t)3 * UVC_NUM_SYMBOLS * (size_t)((npos >> 12) + 2), s.nwin) >= s.buf.size(), "npos %lld: allocation too small", npos);
    }
    // 2. scopes
    CHECK(uvc_link_score_scope(0, 0, 0, 0, 2) == UVC_LINK_NONE, "default gate");
    CHECK(uvc_link_score_scope(1, 0, 0, 0, 2) == UVC_LINK_ALL && uvc_link_score_scope(0, 1, 0, 0, 2) == UVC_LINK_ALL, "-A");
    CHECK(uvc_link_score_scope(0, 0, 1, 0, 2) == UVC_LINK_ALL, "tumor keys");
    CHECK(uvc_link_score_scope(0, 0, 0, 3, 2) == UVC_LINK_ALL, "forced sites");
    CHECK(uvc_link_score_scope(0, 0, 0, 0, 0) == UVC_LINK_ALL && uvc_link_score_scope(0, 0, 0, 0, -1) == UVC_LINK_ALL, "min_altdp_thres <= 0 opens every group");
    for (int g = 0; g < UVC_NUM_FIELD_GROUPS; g++)
        CHECK(uvc_link_fetch_scope(g) == ((g == UVC_F_SEG32 || g == UVC_F_SEG64 || g == UVC_F_VQ) ? UVC_LINK_ALL : UVC_LINK_NONE), "fetch of group %d", g);
    CHECK(uvc_link_columns_scope() == UVC_LINK_POSITIONS && uvc_link_presence_scope() == UVC_LINK_NONE, "columns / presence");
    for (int sym = 0; sym < UVC_NUM_SYMBOLS; sym++)
        CHECK(uvc_link_occ_marks(1u << sym) == (sym > UVC_LINK_M), "occ bit of symbol %d", sym);
    // 3. the state machine
    for (long long npos : { 65LL, 257LL, 4097LL }) {
        Stub s(npos); Handle h(s);
        h.read(UVC_LINK_ALL);
        CHECK(s.launches == 0, "npos %lld: a pass before the first accumulate", npos);
        s.occ[0] = 1u << UVC_LINK_I1; s.occ[(size_t)npos - 1] = 1u << UVC_LINK_D2; s.occ[1] = 1u << UVC_BASE_NN; if (npos > 200) s.occ[130] = 1u << UVC_LINK_M;   // (neither marks a window)
        const long long last = (npos - 1) >> 6;
        for (int round = 0; round < 3; round++) {
            h.accumulate(false);
            long long n = 0; for (int v : s.runs) n += v;
            CHECK(s.runs[0] == 1 && s.runs[(size_t)last] == 1 && n == (last ? 2 : 1), "npos %lld: INDEL ran %lld windows", npos, n);
            h.read(uvc_link_presence_scope()); h.read(uvc_link_score_scope(0, 0, 0, 0, 2));
            for (int v : s.runs) n -= v;
            CHECK(n == 0 && !h.link.all_done, "npos %lld: the default gate or the presence check completed something", npos);
            h.read(UVC_LINK_POSITIONS, { 63, 64, -5, (int)npos, (int)npos + 70 });
            CHECK(s.runs[0] == 1 && s.runs[1] == 1, "npos %lld: POSITIONS at 63 | 64", npos);
            const int before = s.launches;
            h.read(UVC_LINK_ALL); h.read(UVC_LINK_ALL); h.read(UVC_LINK_POSITIONS, { 1 }); h.read(uvc_link_fetch_scope(UVC_F_VQ));
            CHECK(s.launches == before + 1, "npos %lld: %d launches behind ALL", npos, s.launches - before);
            for (long long w = 0; w < s.nwin; w++) CHECK(s.runs[(size_t)w] == 1, "npos %lld round %d: window %lld ran %d times", npos, round, w, s.runs[(size_t)w]);
        }
        h.accumulate(true);
        const int before = s.launches;
        h.read(UVC_LINK_ALL); h.read(UVC_LINK_POSITIONS, { 0 });
        for (long long w = 0; w < s.nwin; w++) CHECK(s.runs[(size_t)w] == 1, "npos %lld eager: window %lld ran %d times", npos, w, s.runs[(size_t)w]);
        CHECK(s.launches == before, "npos %lld: a pass behind an eager accumulate", npos);
        h.accumulate(false); h.released = true;
        const int b2 = s.launches;
        h.read(UVC_LINK_ALL);
        CHECK(s.launches == b2, "npos %lld: a pass on released planes", npos);
    }
    printf("link rules: %d failures\n", failures);
    return failures ? 1 : 0;
}
