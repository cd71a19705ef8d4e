// Host check of uvc_amd/csrc/uvc_score_rows.h (tests/test_score_layout_cpu.py builds this with -fsanitize=undefined and runs it).
//   1. The row block (score_rows_layout), the scratch of a one-call score (scratch_layout) and the row set of a streamed chunk (set_layout)
//      over (c, gc) in {1, 2, 15, 16, 17, 2047, 2048, 2049, 100000}^2, with and without the kept copy, and npos in {0, 1, 31, 32, 33, 1024,
//      1025}: every block 16-aligned, in order, not overlapping, with room for rows x length x element size; total = the end of the last
//      block; the rows per group min(gc, c) long; zero_bytes = the counters and the tile states of the scans, nothing behind them.
//      (Inside the zeroed head the words are 8-byte ones and 8-aligned; the head as a whole and everything behind it is 16-aligned.)
//   2. The bytes per record from the table, and uvc_score_set_bytes, against the values of the commit before this header existed.
#include <cstdio>
#include <initializer_list>
#include "../../uvc_amd/csrc/uvc_score_rows.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const long long SIZES[9] = { 1, 2, 15, 16, 17, 2047, 2048, 2049, 100000 };
static const long long NPOS[7] = { 0, 1, 31, 32, 33, 1024, 1025 };
struct Block { const char *name; size_t off, need; };

// blocks in order from `begin`: 16-aligned, each ends at or in front of the next, the last at or in front of `end`
static void check_blocks(const char *what, long long a, long long b, int k, const Block *bl, int n, size_t begin, size_t end) {
    size_t at = begin;
    for (int i = 0; i < n; i++) {
        CHECK(bl[i].off % 16 == 0, "%s(%lld, %lld, %d) %s at %zu", what, a, b, k, bl[i].name, bl[i].off);
        CHECK(bl[i].off >= at, "%s(%lld, %lld, %d) %s at %zu overlaps its predecessor, which ends at %zu", what, a, b, k, bl[i].name, bl[i].off, at);
        at = bl[i].off + bl[i].need;
    }
    CHECK(at <= end && end % 16 == 0 && end - at < 16, "%s(%lld, %lld, %d) the last block ends at %zu, the layout at %zu", what, a, b, k, at, end);
}
// the row block as Blocks (behind bl[n0 ...]); returns the count
static int row_blocks(const ScoreRows &L, long long c, long long gc, Block *bl) {
    static const char *names[NSROW] = {
#define X(n, T, rows, by_group) #n,
        SCORE_ROW_LIST(X)
#undef X
    };
    const long long glen = (gc < c ? gc : c);
    for (int i = 0; i < NSROW; i++) bl[i] = Block{ names[i], L.off[i], (size_t)SCORE_ROWS[i].rows * (size_t)(SCORE_ROWS[i].by_group ? glen : c) * (size_t)SCORE_ROWS[i].elem };
    return NSROW;
}

static int check_rows_and_sets() {
    int n = 0;
    for (long long c : SIZES) for (long long gc : SIZES) {
        const long long glen = (gc < c ? gc : c);
        for (size_t at : { (size_t)0, (size_t)16, (size_t)4096 + 48 }) {
            const ScoreRows L = score_rows_layout(at, c, gc);
            Block bl[NSROW]; row_blocks(L, c, gc, bl);
            check_blocks("rows", c, gc, (int)at, bl, NSROW, at, L.end);
            CHECK(L.c == c && L.gc == glen, "rows(%lld, %lld): c %lld gc %lld", c, gc, L.c, L.gc);
            // the rows per group are exactly min(gc, c) long: the block in front of `rh` is no longer than that (plus padding)
            CHECK(L.off[SROW_tot] - L.off[SROW_grp] == score_align16((size_t)NGR * glen * 4) && L.off[SROW_rh] - L.off[SROW_tot] == score_align16((size_t)NTOT * glen * 8)
                  && L.end - L.off[SROW_keptoff] == score_align16((size_t)glen * 4), "rows(%lld, %lld): the rows per group are not min(gc, c) long", c, gc);
            n++;
        }
        for (int kept = 0; kept < 2; kept++) {
            const SetLayout Q = set_layout(c, gc, kept);
            const size_t rec = (size_t)UVC_NUM_SCORE_FIELDS * (size_t)c * 4, tiles = ((size_t)glen + GS_TILE - 1) / GS_TILE;
            Block bl[NSROW + 2]; int m = row_blocks(Q.rows, c, gc, bl);
            bl[m++] = Block{ "fields", Q.fields, rec };
            bl[m++] = Block{ "kept", Q.kept, kept ? rec : 0 };
            check_blocks("set", c, gc, kept, bl, m, Q.zero_bytes, Q.total);
            // the zeroed head: 16 bytes of record counts, the counters, the keep scan's tile states (one per tile at least), then the rows
            CHECK(Q.cnt == 16 && Q.status2 == Q.cnt + NCNT * 4 && Q.status2 % 8 == 0 && Q.zero_bytes >= Q.status2 + tiles * 8 && Q.zero_bytes == Q.rows.off[0] && Q.zero_bytes % 16 == 0,
                  "set(%lld, %lld, %d): head cnt %zu status2 %zu zero_bytes %zu rows %zu", c, gc, kept, Q.cnt, Q.status2, Q.zero_bytes, Q.rows.off[0]);
            CHECK(Q.zero_bytes <= score_align16(Q.status2 + (tiles + 1) * 8), "set(%lld, %lld, %d): zero_bytes %zu reaches behind the tile states", c, gc, kept, Q.zero_bytes);
            CHECK(Q.fields == Q.rows.end, "set(%lld, %lld, %d): fields %zu, the rows end at %zu", c, gc, kept, Q.fields, Q.rows.end);
            CHECK(Q.total <= 96 + (size_t)c * score_set_bytes_per_record() + 16 * (NSROW + 2), "set(%lld, %lld, %d): %zu bytes, more than bytes_per_record allows", c, gc, kept, Q.total);
            n++;
        }
    }
    return n;
}

static int check_scratch() {
    int n = 0;
    for (long long npos : NPOS) for (long long c : SIZES) {
        const ScratchLayout L = scratch_layout(npos, c);
        const long long ngroups = 2 * npos, gc = (ngroups > 0 ? ngroups : 1), glen = (gc < c ? gc : c);
        const size_t tiles1 = ((size_t)ngroups + GATE_TILE - 1) / GATE_TILE, tiles2 = ((size_t)(ngroups < c ? ngroups : c) + GS_TILE - 1) / GS_TILE;
        Block bl[NSROW + 4]; int m = 0;
        bl[m++] = Block{ "offsets", L.offsets, ((size_t)ngroups + 1) * 8 };
        bl[m++] = Block{ "active", L.active, (size_t)ngroups * 4 };
        m += row_blocks(L.rows, c, gc, bl + m);
        bl[m++] = Block{ "force_mask", L.force_mask, (((size_t)npos + 31) / 32) * 4 };
        bl[m++] = Block{ "zpos_tab", L.zpos_tab, (size_t)npos * 4 };
        check_blocks("scratch", npos, c, 0, bl, m, L.zero_bytes, L.total);
        CHECK(L.rows.c == c && L.rows.gc == glen, "scratch(%lld, %lld): rows for c %lld gc %lld", npos, c, L.rows.c, L.rows.gc);
        CHECK(L.cnt == 16 && L.status1 == L.cnt + NCNT * 4 && L.status1 % 8 == 0 && L.status2 >= L.status1 + tiles1 * 8 && L.status2 % 8 == 0
              && L.zero_bytes >= L.status2 + tiles2 * 8 && L.zero_bytes == L.offsets && L.zero_bytes % 16 == 0,
              "scratch(%lld, %lld): head cnt %zu status1 %zu status2 %zu zero_bytes %zu offsets %zu", npos, c, L.cnt, L.status1, L.status2, L.zero_bytes, L.offsets);
        CHECK(L.status2 == L.status1 + (tiles1 + 1) * 8 && L.zero_bytes <= score_align16(L.status2 + (tiles2 + 1) * 8), "scratch(%lld, %lld): zero_bytes %zu reaches behind the tile states", npos, c, L.zero_bytes);
        n++;
    }
    return n;
}

static int check_parent_values() {
    // read from the build of commit 4a90cce ("Accumulate kernels: shared rules in uvc_rules.h, record words by name"), the last one that
    // spelled the sum and the two layouts out by hand: uvc_score_set_bytes_per_record() and uvc_score_set_bytes(c, ngroups, with_kept)
    size_t table = 0;
    for (int i = 0; i < NSROW; i++) table += (size_t)SCORE_ROWS[i].rows * (size_t)SCORE_ROWS[i].elem;
    const size_t extras = 2 * (size_t)UVC_NUM_SCORE_FIELDS * 4 /* the records and their kept copy */ + 1 /* the tile states */;
    CHECK(score_set_bytes_per_record() == table + extras, "bytes per record %zu, table %zu + extras %zu", score_set_bytes_per_record(), table, extras);
    CHECK(score_set_bytes_per_record() == 2485, "bytes per record %zu, 2485 at 4a90cce", score_set_bytes_per_record());
    CHECK(2 * (score_set_bytes_per_record() + 4 * (size_t)UVC_NUM_SCORE_FIELDS) == 6058, "uvcgpu_score_stream_bytes_per_record would be %zu, 6058 in INTEGRATION.md", 2 * (score_set_bytes_per_record() + 4 * (size_t)UVC_NUM_SCORE_FIELDS));
    static const struct { long long c, ngroups; int kept; size_t bytes; } at_parent[4] = {
        { 1, 2, 0, 2032 }, { 4096, 1600, 1, 8447296 }, { 4096, 100000, 1, 10174544 }, { 100000, 1600, 0, 125907264 } };
    for (const auto &q : at_parent) CHECK(set_layout(q.c, q.ngroups, q.kept).total == q.bytes, "set_bytes(%lld, %lld, %d) = %zu, %zu at 4a90cce", q.c, q.ngroups, q.kept, set_layout(q.c, q.ngroups, q.kept).total, q.bytes);
    // the one-call scratch where the capacity does not exceed the groups (unchanged), and where it does (the rows per group now follow the groups)
    CHECK(scratch_layout(1024, 2047).total == 2886528 && scratch_layout(1025, 2048).total == 2887984 && scratch_layout(33, 17).total == 24816, "scratch bytes at capacity <= groups changed");
    CHECK(scratch_layout(33, 100000).total < 139601056 && scratch_layout(1024, 100000).total < 139628896, "scratch bytes at capacity > groups did not shrink");
    return 4;
}

int main() {
    const int n_sets = check_rows_and_sets(), n_scratch = check_scratch(), n_lit = check_parent_values();
    printf("row blocks and sets %d cases, scratch %d, set_bytes literals %d, %d failures\n", n_sets, n_scratch, n_lit, failures);
    return failures ? 1 : 0;
}
