/* pf_bgzf.h -- the BGZF block header rule, once, for the host reader
 * (pf_bam.c) and the device ingest's block scans (pf_ingest.hip); C11 and
 * C++17.
 *
 * A BGZF block is a gzip member (SAMv1 4.1): magic 31 139, CM 8, FLG with
 * FEXTRA, XLEN at byte 10 and the extra field from byte 12, among whose
 * subfields (SI1 SI2 SLEN data) the one named "BC" with SLEN 2 holds
 * BSIZE = block size - 1.  The block must hold its header and the 8 footer
 * bytes and be at most 65536 bytes.  The footer (CRC32, ISIZE) stays with
 * the callers that read it. */
#ifndef PF_BGZF_H
#define PF_BGZF_H
#include <stdint.h>

typedef struct pf_bgzf_hdr {
    uint32_t xlen;            /* extra field bytes: the DEFLATE payload starts at 12 + xlen */
    uint32_t bsize;           /* the whole block, header to footer */
} pf_bgzf_hdr;

#define PF_BGZF_MALFORMED (-1)

/* The header of the block at h, of which `avail` bytes are valid: 0 with
 * *out set once the whole block lies inside them; N > avail when at least N
 * bytes are needed to say more (the answers grow as the bytes arrive, up to
 * the block's size); PF_BGZF_MALFORMED.  Reads nothing at or past avail. */
static inline int pf_bgzf_header(const uint8_t *h, uint64_t avail, pf_bgzf_hdr *out) {
    if (avail < 18) return 18;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) return PF_BGZF_MALFORMED;
    const uint32_t xlen = (uint32_t)h[10] | ((uint32_t)h[11] << 8);
    if (avail < 12ull + xlen) return (int)(12 + xlen);
    uint32_t bsize = 0;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint8_t *sf = h + 12 + x;
        const uint32_t slen = (uint32_t)sf[2] | ((uint32_t)sf[3] << 8);
        if (sf[0] == 'B' && sf[1] == 'C' && slen == 2) {
            /* (a BC subfield that starts within the last 5 bytes of the extra
             * field has its value past it: taken all the same, as ever) */
            if (avail < 12ull + x + 6) return (int)(12 + x + 6);
            bsize = ((uint32_t)sf[4] | ((uint32_t)sf[5] << 8)) + 1;
        }
        x += 4 + slen;
    }
    if (bsize < 12 + xlen + 8 || bsize > 65536) return PF_BGZF_MALFORMED;
    if (avail < bsize) return (int)bsize;
    out->xlen = xlen;
    out->bsize = bsize;
    return 0;
}

#endif
