/*
 * pf_ref.c -- the reference FASTA on the host (pf_ref_t) and the MD rule
 * ("MD synthesis"): MD:Z as a function of CIGAR, SEQ and the
 * reference, for BAMs whose records carry no MD tag.
 *
 * The FASTA is read once, front to back, through zlib (plain and gzipped
 * files alike, as pf_windows.c reads VCFs).  Every contig is stored as packed
 * nibbles, high nibble first, in BAM SEQ's code: A 1, C 2, G 4, T/U 8, any
 * other byte 15.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "../../include/pomfret_amd.h"
#include "pf_host.h"

typedef struct {
    char *name;
    uint8_t *nib;                /* (len + 1) / 2 bytes (+ pad) */
    uint64_t len, cap;           /* bases; bytes allocated */
} ref_contig_t;

struct pf_ref {
    uint32_t n, cap;
    ref_contig_t *c;
};

static int contig_put(ref_contig_t *c, uint8_t code) {
    const uint64_t byte = c->len >> 1;
    if (byte + 1 > c->cap) {
        const uint64_t ncap = c->cap ? 2 * c->cap : 1 << 16;
        uint8_t *np = (uint8_t *)realloc(c->nib, ncap);
        if (!np) return PF_ERR_NOMEM;
        memset(np + c->cap, 0, ncap - c->cap);
        c->nib = np;
        c->cap = ncap;
    }
    if (c->len & 1) c->nib[byte] |= code;
    else c->nib[byte] = (uint8_t)(code << 4);
    c->len++;
    return PF_OK;
}

/* pf_mdsynth.hip: a context's device copy of these nibbles goes with them */
void pf_mdsynth_forget(const uint8_t *nib);

void pf_ref_free(pf_ref_t *r) {
    if (!r) return;
    for (uint32_t i = 0; i < r->n; i++) {
        if (r->c[i].nib) pf_mdsynth_forget(r->c[i].nib);
        free(r->c[i].name);
        free(r->c[i].nib);
    }
    free(r->c);
    free(r);
}

int pf_ref_open(const char *path, pf_ref_t **out) {
    if (!path || !out) return PF_ERR_ARG;
    *out = NULL;
    gzFile fp = gzopen(path, "rb");
    if (!fp) return -1;
    pf_ref_t *r = (pf_ref_t *)calloc(1, sizeof(pf_ref_t));
    const size_t BUF = 1 << 20;
    uint8_t *buf = (uint8_t *)malloc(BUF);
    char *name = NULL;
    size_t name_n = 0, name_cap = 0;
    int rc = (r && buf) ? PF_OK : PF_ERR_NOMEM;
    uint8_t code[256];
    memset(code, 15, sizeof code);
    code['A'] = code['a'] = 1; code['C'] = code['c'] = 2; code['G'] = code['g'] = 4;
    code['T'] = code['t'] = code['U'] = code['u'] = 8;
    /* state: 0 line start, 1 inside a sequence line, 2 header name, 3 header rest */
    int state = 0;
    ref_contig_t *cur = NULL;
    while (!rc) {
        const int nr = gzread(fp, buf, (unsigned)BUF);
        if (nr < 0) { rc = -1; break; }
        if (nr == 0) break;
        for (int i = 0; i < nr && !rc; i++) {
            const uint8_t ch = buf[i];
            if (state == 2 || state == 3) {
                const int ws = ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n' || ch == '\v' || ch == '\f';
                if (state == 2 && !ws) {
                    if (name_n + 2 > name_cap) {
                        name_cap = name_cap ? 2 * name_cap : 64;
                        char *np = (char *)realloc(name, name_cap);
                        if (!np) { rc = PF_ERR_NOMEM; break; }
                        name = np;
                    }
                    name[name_n++] = (char)ch;
                } else if (state == 2) state = 3;
                if (ch != '\n') continue;
                /* header complete: a new contig */
                if (!name) { name = (char *)malloc(1); if (!name) { rc = PF_ERR_NOMEM; break; } }
                name[name_n] = 0;
                for (uint32_t k = 0; k < r->n; k++)
                    if (strcmp(r->c[k].name, name) == 0) rc = PF_ERR_ARG;      /* duplicate name */
                if (rc) break;
                if (r->n == r->cap) {
                    const uint32_t ncap = r->cap ? 2 * r->cap : 32;
                    ref_contig_t *np = (ref_contig_t *)realloc(r->c, ncap * sizeof(ref_contig_t));
                    if (!np) { rc = PF_ERR_NOMEM; break; }
                    r->c = np;
                    r->cap = ncap;
                }
                cur = &r->c[r->n++];
                memset(cur, 0, sizeof *cur);
                cur->name = strdup(name);
                if (!cur->name) { rc = PF_ERR_NOMEM; break; }
                name_n = 0;
                state = 0;
                continue;
            }
            if (ch == '\n') { state = 0; continue; }
            if (state == 0 && ch == '>') { state = 2; name_n = 0; continue; }
            state = 1;
            if (ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f') continue;
            if (!cur) { rc = PF_ERR_ARG; break; }                              /* sequence before a header */
            rc = contig_put(cur, code[ch]);
        }
    }
    if (!rc && (state == 2 || state == 3)) {
        /* a header as the last line, without its newline: an empty contig */
        char *nm = (char *)malloc(name_n + 1);
        if (!nm) rc = PF_ERR_NOMEM;
        else {
            memcpy(nm, name ? name : "", name_n);
            nm[name_n] = 0;
            for (uint32_t k = 0; k < r->n && !rc; k++)
                if (strcmp(r->c[k].name, nm) == 0) rc = PF_ERR_ARG;
            ref_contig_t *np = rc ? NULL : (ref_contig_t *)realloc(r->c, (r->n + 1ull) * sizeof(ref_contig_t));
            if (!rc && !np) rc = PF_ERR_NOMEM;
            if (!rc) {
                r->c = np;
                r->cap = r->n + 1;
                memset(&r->c[r->n], 0, sizeof(ref_contig_t));
                r->c[r->n++].name = nm;
                nm = NULL;
            }
            free(nm);
        }
    }
    gzclose(fp);
    free(buf);
    free(name);
    if (rc) { pf_ref_free(r); return rc; }
    *out = r;
    return PF_OK;
}

uint32_t pf_ref_n(const pf_ref_t *r) { return r ? r->n : 0; }

const char *pf_ref_name(const pf_ref_t *r, uint32_t i) { return r && i < r->n ? r->c[i].name : NULL; }

int pf_ref_contig(const pf_ref_t *r, const char *name, const uint8_t **nib, uint64_t *len) {
    if (!r || !name) return PF_ERR_ARG;
    for (uint32_t i = 0; i < r->n; i++) {
        if (strcmp(r->c[i].name, name)) continue;
        if (nib) *nib = r->c[i].nib ? r->c[i].nib : (const uint8_t *)"";
        if (len) *len = r->c[i].len;
        return PF_OK;
    }
    return PF_ERR_ARG;
}

/* ------------------------------------------------------------------ */
/* the MD rule, one record */

static inline uint32_t nib_at(const uint8_t *p, uint64_t i) { return (p[i >> 1] >> ((~i & 1) << 2)) & 0xfu; }

static int md_put(uint8_t **md, uint64_t *n, uint64_t *cap, const void *src, uint64_t k) {
    if (*n + k > *cap) {
        uint64_t ncap = *cap ? 2 * *cap : 1 << 12;
        while (ncap < *n + k) ncap *= 2;
        uint8_t *np = (uint8_t *)realloc(*md, ncap);
        if (!np) return PF_ERR_NOMEM;
        *md = np;
        *cap = ncap;
    }
    memcpy(*md + *n, src, k);
    *n += k;
    return PF_OK;
}

static int md_put_dec(uint8_t **md, uint64_t *n, uint64_t *cap, uint64_t u) {
    char t[24];
    int k = 0;
    do { t[k++] = (char)('0' + u % 10); u /= 10; } while (u);
    char s[24];
    for (int i = 0; i < k; i++) s[i] = t[k - 1 - i];
    return md_put(md, n, cap, s, (uint64_t)k);
}

/* cig: n_cigar little-endian u32 (len << 4 | op), any alignment; appends the
 * record's MD to (*md, *n, *cap) */
int pf_md_synth_rec(const uint8_t *cig, uint32_t ncig, const uint8_t *seq, uint32_t l_seq, uint32_t pos,
                    const uint8_t *ref_nib, uint64_t ref_len, uint8_t **md, uint64_t *n, uint64_t *cap) {
    static const char L[] = "=ACMGRSVTWYHKDBN";
    uint64_t x = pos, y = 0, u = 0;
    int rc = PF_OK;
    for (uint32_t i = 0; i < ncig && !rc; i++) {
        const uint32_t w = (uint32_t)cig[4ull * i] | (uint32_t)cig[4ull * i + 1] << 8 |
                           (uint32_t)cig[4ull * i + 2] << 16 | (uint32_t)cig[4ull * i + 3] << 24;
        const uint32_t op = w & 15u;
        const uint64_t l = w >> 4;
        if (op == 0 || op == 7 || op == 8) {
            if (x + l > ref_len) return PF_ERR_ARG;
            for (uint64_t j = 0; j < l && !rc; j++) {
                const uint32_t c1 = y + j < l_seq ? nib_at(seq, y + j) : 15u, c2 = nib_at(ref_nib, x + j);
                if (c1 == 0 || (c1 == c2 && c1 != 15)) { u++; continue; }
                rc = md_put_dec(md, n, cap, u);
                if (!rc) rc = md_put(md, n, cap, &L[c2], 1);
                u = 0;
            }
            x += l; y += l;
        } else if (op == 2) {
            if (x + l > ref_len) return PF_ERR_ARG;
            rc = md_put_dec(md, n, cap, u);
            if (!rc) rc = md_put(md, n, cap, "^", 1);
            for (uint64_t j = 0; j < l && !rc; j++) rc = md_put(md, n, cap, &L[nib_at(ref_nib, x + j)], 1);
            u = 0;
            x += l;
        } else if (op == 1 || op == 4) y += l;
        else if (op == 3) x += l;
    }
    if (!rc) rc = md_put_dec(md, n, cap, u);
    return rc;
}

int pf_md_synth_host(const pf_read_aln_batch_t *reads, const uint8_t *ref_nib, uint64_t ref_len, uint64_t **md_off,
                     uint8_t **md) {
    if (!reads || !md_off || !md || (!ref_nib && ref_len)) return PF_ERR_ARG;
    *md_off = NULL;
    *md = NULL;
    const uint32_t N = reads->n_reads;
    uint64_t *off = (uint64_t *)malloc((N + 1ull) * sizeof(uint64_t));
    uint8_t *buf = (uint8_t *)malloc(1 << 12);
    uint64_t n = 0, cap = 1 << 12;
    if (!off || !buf) { free(off); free(buf); return PF_ERR_NOMEM; }
    int rc = PF_OK;
    off[0] = 0;
    for (uint32_t r = 0; r < N && !rc; r++) {
        rc = pf_md_synth_rec((const uint8_t *)(reads->cigar + reads->cigar_off[r]),
                             (uint32_t)(reads->cigar_off[r + 1] - reads->cigar_off[r]),
                             reads->seq + reads->seq_off[r], reads->seq_len[r], reads->start[r], ref_nib, ref_len, &buf,
                             &n, &cap);
        off[r + 1] = n;
    }
    if (rc) { free(off); free(buf); return rc; }
    *md_off = off;
    *md = buf;
    return PF_OK;
}

void pf_md_free(uint64_t *md_off, uint8_t *md) {
    free(md_off);
    free(md);
}
