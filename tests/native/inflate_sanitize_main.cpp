// TEST INFRASTRUCTURE: the two host-compilable DEFLATE decoders (uvc_inflate_core.h at both table widths, uvc_inflate_fast.h) on case files
// written by tests/test_inflate.py, as a stand-alone program so that it can be built with -fsanitize=address,undefined and run as a child
// process.  Every input and output buffer is a heap block of exactly the case's size: a read behind the stream or a write behind ISIZE is
// the sanitizer's to report.  Not part of any shipped library.
//
// case file: "UVCINFL1", u32 n, then per case: u32 kind (0 valid, 1 valid and the fast decoder may decline, 2 invalid), u32 name_len,
// u32 comp_len, u32 isize, u32 want_len, name, comp, want (little-endian; want_len is isize for a valid case and 0 for an invalid one)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../uvc_amd/csrc/uvc_inflate_core.h"
#include "../../uvc_amd/csrc/uvc_inflate_fast.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    char magic[8]; uint32_t n = 0;
    if (!f || !rd(f, magic, 8) || memcmp(magic, "UVCINFL1", 8) || !rd(f, &n, 4)) { fprintf(stderr, "bad case file\n"); return 2; }
    static InflStateT<9, 7> S97; static InflStateT<10, 9> S109;
    int bad = 0, declined = 0;
    for (uint32_t c = 0; c < n; c++) {
        uint32_t h[5];
        if (!rd(f, h, sizeof(h))) { fprintf(stderr, "truncated case file\n"); return 2; }
        const uint32_t kind = h[0], comp_len = h[2], isize = h[3], want_len = h[4];
        std::string name(h[1], ' ');
        std::vector<uint8_t> want(want_len);
        uint8_t *comp = (uint8_t *)malloc(comp_len ? comp_len : 1);
        if (!rd(f, &name[0], h[1]) || !rd(f, comp, comp_len) || !rd(f, want.data(), want_len)) { fprintf(stderr, "truncated case file\n"); return 2; }
        for (int dec = 0; dec < 3; dec++) {
            uint8_t *out = (uint8_t *)malloc(isize ? isize : 1);
            memset(out, 0xAB, isize ? isize : 1);
            int ok;   // 1 decoded, 0 refused
            if (dec == 0) ok = uvc_inflate_block_t<false, 9, 7>(comp, comp_len, out, isize, S97, 0u) == 0;
            else if (dec == 1) ok = uvc_inflate_block_t<false, 10, 9>(comp, comp_len, out, isize, S109, 0u) == 0;
            else ok = uvc_fast_inflate::inflate(comp, comp_len, out, isize) ? 1 : 0;
            const char *what = dec == 0 ? "core<9,7>" : dec == 1 ? "core<10,9>" : "fast";
            if (kind == 2) { if (ok) { printf("FAIL %s: %s accepts an invalid stream\n", name.c_str(), what); bad++; } }
            else if (!ok) {
                if (dec == 2 && kind == 1) declined++;
                else { printf("FAIL %s: %s refuses a valid stream\n", name.c_str(), what); bad++; }
            } else if (want_len != isize || (isize && memcmp(out, want.data(), isize))) { printf("FAIL %s: %s decodes other bytes\n", name.c_str(), what); bad++; }
            free(out);
        }
        free(comp);
    }
    fclose(f);
    printf("%u cases, %d failures, fast decoder declined %d\n", n, bad, declined);
    return bad ? 1 : 0;
}
