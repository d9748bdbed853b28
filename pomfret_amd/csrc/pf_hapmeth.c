/*
 * pf_hapmeth.c -- `pomfret-amd hapmeth`: per-haplotype CpG methylation of a
 * haplotagged BAM (the output of methphase --write-bam, of varhaptag, or of
 * any other haplotagger), and where the two haplotypes differ.  No reference
 * counterpart.
 *
 *   pf_write_hapmeth: the sites of a pileup (pf_batch_pileup) as BED lines
 *                     with the allele-specific methylation p-value (host only);
 *   pf_hapmeth_main:  contigs in header order (or one region), cut into
 *                     consecutive windows of chunk_size bases -- the fetch
 *                     unit; a window the index holds no chunk for is skipped
 *                     without a fetch -- and run as jobs of job_windows windows
 *                     one after another on one device: fetch with no read-back
 *                     margin (a read overlapping two windows is decoded in
 *                     both and counted in each inside that window's range, so
 *                     nothing counts twice), pileup under the records' HP
 *                     tags, write.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/pomfret_amd.h"

int pf_write_hapmeth(const char *path, const char *chrom, const pf_pileup_t *p, uint32_t w0, uint32_t w1, int header) {
    if (!path || w1 < w0 || (w1 > w0 && (!p || !chrom || w1 > p->n_windows || !p->win_off))) return PF_ERR_ARG;
    FILE *fp = fopen(path, header ? "w" : "a");
    if (!fp) return -1;
    if (header)
        fprintf(fp, "#chrom\tstart\tend\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tother_meth\tother_unmeth\tasm_p\n");
    if (w1 > w0)
        for (uint64_t i = p->win_off[w0]; i < p->win_off[w1]; i++) {
            const uint32_t *c = p->cnt + 6 * i;
            double two = 1.0;
            (void)pf_fisher_exact((int)c[0], (int)c[1], (int)c[2], (int)c[3], NULL, NULL, &two);
            fprintf(fp, "%s\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%.6g\n", chrom, p->pos[i], p->pos[i] + 1u, c[0], c[1], c[2],
                    c[3], c[4], c[5], two);
        }
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

/* "chrom" or "chrom:beg-end" / "chrom:beg" (1-based inclusive, commas allowed)
 * -> tid and the 0-based [*s, *e); a name that holds ':' itself is tried whole
 * first */
static int parse_region(const pf_bam_t *bam, const char *region, int32_t *tid, uint32_t *s, uint32_t *e) {
    int32_t t = pf_bam_tid(bam, region);
    if (t >= 0) { *tid = t; *s = 0; *e = pf_bam_target_len(bam, t); return PF_OK; }
    const char *colon = strrchr(region, ':');
    if (!colon || colon == region) return PF_ERR_ARG;
    char *name = (char *)malloc((size_t)(colon - region) + 1);
    if (!name) return PF_ERR_NOMEM;
    memcpy(name, region, (size_t)(colon - region));
    name[colon - region] = 0;
    t = pf_bam_tid(bam, name);
    free(name);
    if (t < 0) return PF_ERR_ARG;
    uint64_t v[2] = {0, 0};
    int k = 0, digits = 0;
    for (const char *q = colon + 1; *q; q++) {
        if (*q == ',') continue;
        if (*q == '-' && k == 0 && digits) { k = 1; digits = 0; continue; }
        if (*q < '0' || *q > '9') return PF_ERR_ARG;
        v[k] = v[k] * 10 + (uint64_t)(*q - '0');
        if (v[k] > UINT32_MAX) return PF_ERR_ARG;
        digits++;
    }
    if (!digits && k == 0) return PF_ERR_ARG;
    const uint32_t len = pf_bam_target_len(bam, t);
    uint64_t b = v[0] ? v[0] - 1 : 0, en = k && digits ? v[1] : len;
    if (en > len) en = len;
    if (b > en) b = en;
    *tid = t; *s = (uint32_t)b; *e = (uint32_t)en;
    return PF_OK;
}

typedef struct {
    const pf_hapmeth_opts_t *o;
    pf_bam_t *bam;
    pf_ctx_t *ctx;
    pf_cfg_t cfg;
    pf_load_cfg_t lc;
    char *path;
    pf_hapmeth_stats_t st;
} hm_t;

/* one job: the windows ws/we[0, n) of chrom */
static int hm_job(hm_t *H, const char *chrom, uint32_t n, const uint32_t *ws, const uint32_t *we) {
    pf_dbatch_t *db = NULL;
    pf_bam_dev_fetch_t *F = NULL;
    pf_bam_records_t *recs = NULL;
    pf_pileup_t *pile = NULL;
    int rc;
    if (H->o->host_fetch) {
        rc = pf_bam_fetch_windows(H->bam, chrom, n, ws, we, 0, H->o->threads > 0 ? H->o->threads : 1, &recs);
        if (!rc) {
            H->st.n_records += recs->aln.n_recs;
            rc = pf_batch_upload_aln(H->ctx, &H->cfg, &H->lc, &recs->aln, &db);
        }
    } else {
        rc = pf_batch_upload_bam(H->ctx, &H->cfg, &H->lc, H->bam, chrom, n, ws, we, 0, 0, &db, &F);
        if (!rc) H->st.n_records += F->n_recs;
    }
    if (rc == PF_ERR_LIMIT)
        fprintf(stderr, "[E::pf_hapmeth_main] %s:%u-%u: a window exceeds a device limit (65,535 records per window); "
                "try a smaller --chunk-size\n", chrom, ws[0] + 1, we[n - 1]);
    if (!rc) rc = pf_batch_pileup(H->ctx, db, NULL, 0, &pile);
    if (!rc) rc = pf_write_hapmeth(H->path, chrom, pile, 0, n, 0);
    if (!rc) {
        H->st.n_sites += pile->n_sites;
        H->st.ms_kernels += pile->ms_kernels;
    }
    pf_pileup_free(pile);
    if (db) pf_batch_free(db);
    if (F) pf_bam_dev_fetch_free(F);
    if (recs) pf_bam_records_free(recs);
    return rc;
}

/* [s, e) of contig tid in windows of `chunk` bases, jobs of at most jw windows */
static int hm_span(hm_t *H, int32_t tid, uint32_t s, uint32_t e, uint32_t chunk, uint32_t jw, uint32_t *ws, uint32_t *we) {
    const char *chrom = pf_bam_target_name(H->bam, tid);
    uint32_t n = 0;
    int rc = PF_OK;
    for (uint64_t a = s; a < e && !rc; a += chunk) {
        const uint64_t b = a + chunk < e ? a + chunk : e;
        H->st.n_windows++;
        /* the fetch's region of this window: htslib's 0-based [max(a-1, 0), b) */
        const int64_t nc = pf_bam_query_chunks(H->bam, tid, a > 0 ? (int64_t)a - 1 : 0, (int64_t)b, NULL, 0);
        if (nc < 0) return (int)nc;
        if (nc == 0) { H->st.n_skipped++; continue; }
        ws[n] = (uint32_t)a;
        we[n] = (uint32_t)b;
        if (++n == jw) { rc = hm_job(H, chrom, n, ws, we); n = 0; }
    }
    if (!rc && n) rc = hm_job(H, chrom, n, ws, we);
    return rc;
}

int pf_hapmeth_main(const pf_hapmeth_opts_t *o, pf_hapmeth_stats_t *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (!o || !o->bam_path || !o->out_prefix || !o->out_prefix[0]) return PF_ERR_ARG;
    hm_t H;
    memset(&H, 0, sizeof H);
    H.o = o;
    H.lc = o->load;
    /* the batch's phasing parameters are not used by the pileup: the reference's defaults */
    H.cfg.k = 3; H.cfg.k_span = 5000; H.cfg.cov_for_selection = 6; H.cfg.n_cand = 15; H.cfg.hard_cov = 15;
    const uint32_t chunk = o->chunk_size ? o->chunk_size : 100000u;
    const uint32_t jw = o->job_windows ? o->job_windows : 1024u;
    int rc = pf_bam_open(o->bam_path, NULL, &H.bam);
    if (rc) {
        fprintf(stderr, "[E::pf_hapmeth_main] cannot open %s or its index\n", o->bam_path);
        return rc;
    }
    pf_bam_set_threads(H.bam, o->threads > 0 ? o->threads : 1);
    int32_t tid0 = 0, tid1 = pf_bam_n_targets(H.bam);
    uint32_t s = 0, e = 0;
    if (o->region) {
        rc = parse_region(H.bam, o->region, &tid0, &s, &e);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] bad region \"%s\"\n", o->region);
        tid1 = tid0 + 1;
    }
    uint32_t *ws = NULL, *we = NULL;
    int made = 0;
    if (!rc) {
        rc = pf_ctx_create(o->device, &H.ctx);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] no usable GPU (device %d): %s\n", o->device, pf_strerror(rc));
    }
    if (!rc) {
        const size_t l = strlen(o->out_prefix) + 16;
        H.path = (char *)malloc(l);
        ws = (uint32_t *)malloc(4ull * jw);
        we = (uint32_t *)malloc(4ull * jw);
        if (!H.path || !ws || !we) rc = PF_ERR_NOMEM;
        else snprintf(H.path, l, "%s.hapmeth.bed", o->out_prefix);
    }
    if (!rc) {
        rc = pf_write_hapmeth(H.path, NULL, NULL, 0, 0, 1);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.path);
        else made = 1;
    }
    for (int32_t t = tid0; t < tid1 && !rc; t++) {
        if (!o->region) { s = 0; e = pf_bam_target_len(H.bam, t); }
        rc = hm_span(&H, t, s, e, chunk, jw, ws, we);
    }
    if (rc && made) (void)unlink(H.path);              /* no truncated output behind a failure */
    if (!rc && o->verbose)
        fprintf(stderr, "[M::pf_hapmeth_main] %llu windows (%llu without reads in the index, skipped), %llu records, "
                "%llu sites, pileup kernels %.3f ms\n", (unsigned long long)H.st.n_windows,
                (unsigned long long)H.st.n_skipped, (unsigned long long)H.st.n_records,
                (unsigned long long)H.st.n_sites, H.st.ms_kernels);
    if (stats) *stats = H.st;
    free(ws);
    free(we);
    free(H.path);
    if (H.ctx) pf_ctx_destroy(H.ctx);
    pf_bam_close(H.bam);
    return rc;
}
