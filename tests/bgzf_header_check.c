/* pf_bgzf_header (pomfret_amd/csrc/pf_bgzf.h) on every prefix of a valid
 * block, each prefix in an allocation of exactly its size, and on the
 * malformed headers of tests/_bgzf.py.  tests/test_bam.py builds this with
 * -fsanitize=address,undefined and runs it: a read at or past `avail` aborts. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pf_bgzf.h"

static int ask(const uint8_t *src, size_t n, pf_bgzf_hdr *hd) {
    uint8_t *p = malloc(n);
    if (n) memcpy(p, src, n);
    const int r = pf_bgzf_header(p, n, hd);
    free(p);
    return r;
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (n = %zu)\n", __LINE__, #c, n); return 1; } } while (0)

int main(void) {
    enum { BS6 = 40, BS12 = 46 };
    uint8_t b6[BS6] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, BS6 - 1, 0};
    uint8_t b12[BS12] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 12, 0, 'X', 'Y', 2, 0, 7, 7, 'B', 'C', 2, 0, BS12 - 1, 0};
    const struct { const uint8_t *b; uint32_t xlen, bsize; } ok[2] = {{b6, 6, BS6}, {b12, 12, BS12}};
    pf_bgzf_hdr hd;
    size_t n;
    for (int k = 0; k < 2; k++) {
        int prev = 0;
        for (n = 0; n < ok[k].bsize; n++) {           /* "need N": more than it has, growing, at most the block */
            const int r = ask(ok[k].b, n, &hd);
            CHECK(r > (int)n && r >= prev && r <= (int)ok[k].bsize);
            prev = r;
        }
        CHECK(ask(ok[k].b, n, &hd) == 0 && hd.xlen == ok[k].xlen && hd.bsize == ok[k].bsize);
    }
    const struct { int at; uint8_t val; } bad[5] = {{1, 138}, {3, 0}, {13, 'X'}, {14, 3}, {16, 10}};
    for (n = 0; n < 5; n++) {
        uint8_t m[BS6];
        memcpy(m, b6, BS6);
        m[bad[n].at] = bad[n].val;
        CHECK(ask(m, BS6, &hd) == PF_BGZF_MALFORMED);
    }
    n = 17;                                           /* a header cut short is not a block either */
    CHECK(ask(b6, n, &hd) == 18);
    puts("ok");
    return 0;
}
