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
 *                     tags, write;
 *   pf_dmr_acc_*:     the stitching of pf_dmr_regions results of consecutive
 *                     ranges of one contig (host only);
 *   pf_write_dmr:     the stitched regions as BED lines (host only);
 *   pf_hapmeth_run:   pf_hapmeth_main, and with --dmr the regions of every
 *                     contig: each job's sites through pf_dmr_regions into the
 *                     contig's accumulator, flushed and appended at its end;
 *   pf_hapmeth_run_perm: pf_hapmeth_run, and with --dmr-perm a second pass at
 *                     each contig's end: its regions become the windows of
 *                     jobs fetched like the first pass's and tested by
 *                     pf_batch_permtest, and pf_write_dmr_perm's three columns
 *                     follow pf_write_dmr's;
 *   pf_write_assign:  the scored untagged reads of a pf_batch_assign result as
 *                     lines of {prefix}.hapmeth.assign.tsv (host only);
 *   pf_hapmeth_run_assign: pf_hapmeth_run_perm, and with --assign the same
 *                     second pass (each job fetched once, for the test and the
 *                     assignment alike) scores every region's untagged reads
 *                     against the region's tagged ones (pf_batch_assign);
 *   pf_write_tagcheck, pf_write_tagcheck_regions: a pf_batch_tagcheck result as
 *                     lines of {prefix}.hapmeth.tagcheck.tsv and
 *                     {prefix}.hapmeth.tagcheck.regions.tsv (host only);
 *   pf_hapmeth_run_tagcheck: pf_hapmeth_run_assign, and with --tag-check the
 *                     same second pass, on the same fetched batch, scores every
 *                     region's tagged reads leave-one-out (pf_batch_tagcheck);
 *   pf_hapmeth_run_hmm: pf_hapmeth_run_tagcheck, and with --dmr-hmm the regions
 *                     of a contig come from one pf_dmr_hmm_regions call over
 *                     the informative sites its jobs left on the host;
 *   pf_bh_adjust, pf_write_regions: Benjamini-Hochberg q-values of a run's
 *                     tested regions, and {prefix}.hapmeth.regions.bed (host only);
 *   pf_hapmeth_run_regions: pf_hapmeth_run_hmm, and with --regions the regions
 *                     come from a BED: each job's sites through pf_region_sums,
 *                     the records added per region, the second pass on the
 *                     eligible ones, the file written at the run's end;
 *   pf_rank_p, pf_bh_adjust_p, pf_write_rank: the rank test's p-value, q-values
 *                     of doubles, and {prefix}.hapmeth.rank.tsv (host only);
 *   pf_hapmeth_run_rank: pf_hapmeth_run_regions, and with --dmr-rank the second
 *                     pass also runs pf_batch_ranktest on its batch; one record
 *                     per region, the file written at the run's end;
 *   pf_rank_exact_p, pf_write_rank_exact, pf_hapmeth_run_rank_exact: with
 *                     --dmr-rank-exact pf_batch_rankexact follows the rank test
 *                     on the same batch and the rank file gains exact_p, best_p
 *                     and best_q;
 *   pf_write_rank_tiles, pf_hapmeth_run_tiles: with --tile the first pass also
 *                     tests every fixed-width tile of its windows: after a
 *                     job's pileup one pf_batch_rankranges call on the same
 *                     batch, one record per tile with a read, and
 *                     {prefix}.hapmeth.tiles.tsv at the run's end.
 */
#include <math.h>
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

/* ---- allele-specific regions: stitching and the writer */
struct pf_dmr_acc {
    pf_dmr_cfg_t cfg;
    uint32_t *brk;
    uint32_t n_brk;
    pf_dmr_run_t *runs;        /* closed and kept, ascending */
    size_t n, m;
    pf_dmr_run_t carry;        /* the run still open to the right */
    int have;
    uint32_t last_end;         /* parts must ascend */
    uint64_t n_inf;
};

pf_dmr_acc_t *pf_dmr_acc_new(const pf_dmr_cfg_t *cfg, const uint32_t *breaks, uint32_t n_breaks) {
    if (!cfg || (n_breaks && !breaks)) return NULL;
    for (uint32_t i = 1; i < n_breaks; i++)
        if (breaks[i] < breaks[i - 1]) return NULL;
    pf_dmr_acc_t *a = (pf_dmr_acc_t *)calloc(1, sizeof *a);
    if (!a) return NULL;
    a->cfg = *cfg;
    if (n_breaks) {
        a->brk = (uint32_t *)malloc(4ull * n_breaks);
        if (!a->brk) { free(a); return NULL; }
        memcpy(a->brk, breaks, 4ull * n_breaks);
        a->n_brk = n_breaks;
    }
    return a;
}

void pf_dmr_acc_free(pf_dmr_acc_t *a) {
    if (!a) return;
    free(a->brk);
    free(a->runs);
    free(a);
}

/* breaks <= p */
static uint32_t acc_rank(const pf_dmr_acc_t *a, uint32_t p) {
    uint32_t lo = 0, hi = a->n_brk;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a->brk[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* a run closes: min_sites applies here */
static int acc_close(pf_dmr_acc_t *a, const pf_dmr_run_t *r) {
    if (r->n_sites < a->cfg.min_sites) return PF_OK;
    if (a->n == a->m) {
        const size_t nm = a->m ? a->m * 2 : 64;
        pf_dmr_run_t *p = (pf_dmr_run_t *)realloc(a->runs, nm * sizeof *p);
        if (!p) return PF_ERR_NOMEM;
        a->runs = p;
        a->m = nm;
    }
    a->runs[a->n] = *r;
    a->runs[a->n].open = 0;
    a->runs[a->n].reserved = 0;
    a->n++;
    return PF_OK;
}

int pf_dmr_acc_add(pf_dmr_acc_t *a, const pf_dmr_t *part) {
    if (!a || !part || (part->n_runs && !part->runs)) return PF_ERR_ARG;
    if (part->n_informative == 0) return part->n_runs ? PF_ERR_ARG : PF_OK;     /* the carry stays open */
    for (uint64_t i = 0; i < part->n_runs; i++) {
        const pf_dmr_run_t *r = part->runs + i;
        const uint32_t lo = i ? part->runs[i - 1].end : a->last_end;
        if (r->end <= r->start || r->start < lo || (r->sign != 1 && r->sign != -1) ||
            ((r->open & PF_DMR_OPEN_LEFT) && i != 0) || ((r->open & PF_DMR_OPEN_RIGHT) && i + 1 != part->n_runs))
            return PF_ERR_ARG;
    }
    a->n_inf += part->n_informative;
    uint64_t i = 0;
    int rc = PF_OK;
    if (a->have) {
        const pf_dmr_run_t *r0 = part->n_runs && (part->runs[0].open & PF_DMR_OPEN_LEFT) ? part->runs : NULL;
        const uint32_t last = a->carry.end - 1u;             /* the carry's last member */
        if (r0 && r0->sign == a->carry.sign && r0->start - last <= a->cfg.max_gap &&
            acc_rank(a, last) == acc_rank(a, r0->start)) {
            a->carry.end = r0->end;
            a->carry.n_sites += r0->n_sites;
            for (int k = 0; k < 4; k++) a->carry.sum[k] += r0->sum[k];
            i = 1;
            if (!(r0->open & PF_DMR_OPEN_RIGHT)) { rc = acc_close(a, &a->carry); a->have = 0; }
        } else {
            rc = acc_close(a, &a->carry);
            a->have = 0;
        }
    }
    for (; i < part->n_runs && !rc; i++) {
        const pf_dmr_run_t *r = part->runs + i;
        if (r->open & PF_DMR_OPEN_RIGHT) { a->carry = *r; a->have = 1; }
        else rc = acc_close(a, r);
    }
    if (part->n_runs) a->last_end = part->runs[part->n_runs - 1].end;
    return rc;
}

int pf_dmr_acc_flush(pf_dmr_acc_t *a, pf_dmr_t **final) {
    if (!a || !final) return PF_ERR_ARG;
    *final = NULL;
    if (a->have) {
        const int rc = acc_close(a, &a->carry);
        if (rc) return rc;
        a->have = 0;
    }
    pf_dmr_t *d = (pf_dmr_t *)calloc(1, sizeof *d);
    if (!d) return PF_ERR_NOMEM;
    d->n_runs = a->n;
    d->runs = a->runs;                                       /* handed over: pf_dmr_free */
    d->n_informative = a->n_inf;
    a->runs = NULL;
    a->n = a->m = 0;
    a->n_inf = 0;
    a->last_end = 0;
    *final = d;
    return PF_OK;
}

/* perm NULL: pf_write_dmr's eleven columns; else window k of perm is run k and
 * three columns follow.  n_lines: lines written; n_dot: of those, with "." */
static int write_dmr(const char *path, const char *chrom, const pf_dmr_t *d, const pf_perm_t *perm, double max_p,
                     int header, uint64_t *n_lines, uint64_t *n_dot) {
    if (n_lines) *n_lines = 0;
    if (n_dot) *n_dot = 0;
    const uint64_t n = d ? d->n_runs : 0;
    if (!path || (n && (!chrom || !d->runs))) return PF_ERR_ARG;
    if (perm && n && (perm->n_windows < n || !perm->n_reads || !perm->hits || !perm->status)) return PF_ERR_ARG;
    for (uint64_t i = 0; i < n; i++)
        for (int k = 0; k < 4; k++)
            if (d->runs[i].sum[k] > (uint64_t)INT32_MAX) return PF_ERR_LIMIT;
    FILE *fp = fopen(path, header ? "w" : "a");
    if (!fp) return -1;
    if (header)
        fprintf(fp, "#chrom\tstart\tend\tn_sites\tdir\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta\tpooled_p%s\n",
                perm ? "\treads_h1\treads_h2\tperm_p" : "");
    for (uint64_t i = 0; i < n; i++) {
        const pf_dmr_run_t *r = d->runs + i;
        const uint64_t m1 = r->sum[0], u1 = r->sum[1], m2 = r->sum[2], u2 = r->sum[3];
        double two = 1.0;
        (void)pf_fisher_exact((int)m1, (int)u1, (int)m2, (int)u2, NULL, NULL, &two);
        if (two > max_p) continue;
        const double delta = (m1 + u1 ? (double)m1 / (double)(m1 + u1) : 0.0) - (m2 + u2 ? (double)m2 / (double)(m2 + u2) : 0.0);
        fprintf(fp, "%s\t%u\t%u\t%u\t%s\t%llu\t%llu\t%llu\t%llu\t%.4f\t%.6g", chrom, r->start, r->end, r->n_sites,
                r->sign > 0 ? "h1>h2" : "h1<h2", (unsigned long long)m1, (unsigned long long)u1, (unsigned long long)m2,
                (unsigned long long)u2, delta, two);
        if (perm) {
            fprintf(fp, "\t%u\t%u\t", perm->n_reads[2 * i], perm->n_reads[2 * i + 1]);
            if (perm->status[i] == 0)
                fprintf(fp, "%.6g", ((double)perm->hits[i] + 1.0) / ((double)perm->n_perm + 1.0));
            else {
                fputc('.', fp);
                if (n_dot) ++*n_dot;
            }
        }
        fputc('\n', fp);
        if (n_lines) ++*n_lines;
    }
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

int pf_write_dmr(const char *path, const char *chrom, const pf_dmr_t *dmr, double max_p, int header) {
    return write_dmr(path, chrom, dmr, NULL, max_p, header, NULL, NULL);
}

int pf_write_dmr_perm(const char *path, const char *chrom, const pf_dmr_t *dmr, const pf_perm_t *perm, double max_p,
                      int header) {
    if (!perm) return PF_ERR_ARG;
    return write_dmr(path, chrom, dmr, perm, max_p, header, NULL, NULL);
}

int pf_write_assign(const char *path, const char *chrom, const pf_assign_t *a, const uint32_t *win_start,
                    const uint32_t *win_end, const uint32_t *rec_of_read, const uint64_t *qname_off, const char *qname,
                    int header, uint64_t *n_lines) {
    if (n_lines) *n_lines = 0;
    const uint32_t W = a ? a->n_windows : 0;
    if (!path) return PF_ERR_ARG;
    if (W && (!chrom || !win_start || !win_end || !a->win_read_off || a->win_read_off[W] > a->n_reads)) return PF_ERR_ARG;
    if (W && a->win_read_off[W] && (!a->n_used || !a->llr || !a->hp || !qname_off || !qname)) return PF_ERR_ARG;
    for (uint32_t w = 0; w < W; w++)
        if (a->win_read_off[w] > a->win_read_off[w + 1]) return PF_ERR_ARG;
    FILE *fp = fopen(path, header ? "w" : "a");
    if (!fp) return -1;
    if (header) fprintf(fp, "#qname\tchrom\tstart\tend\tn_calls\tllr\thp\n");
    for (uint32_t w = 0; w < W; w++)
        for (uint32_t r = a->win_read_off[w]; r < a->win_read_off[w + 1]; r++) {
            if (a->n_used[r] < 1u) continue;
            const uint32_t rec = rec_of_read ? rec_of_read[r] : r;
            fprintf(fp, "%.*s\t%s\t%u\t%u\t%u\t%.4f\t%s\n", (int)(qname_off[rec + 1] - qname_off[rec]), qname + qname_off[rec],
                    chrom, win_start[w], win_end[w], a->n_used[r], (double)a->llr[r] / 65536.0,
                    a->hp[r] == 0 ? "1" : a->hp[r] == 1 ? "2" : ".");
            if (n_lines) ++*n_lines;
        }
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

int pf_write_tagcheck(const char *path, const char *chrom, const pf_tagcheck_t *t, const uint32_t *win_start,
                      const uint32_t *win_end, const uint32_t *rec_of_read, const uint64_t *qname_off, const char *qname,
                      int header, uint64_t *n_lines) {
    if (n_lines) *n_lines = 0;
    const uint32_t W = t ? t->n_windows : 0;
    if (!path) return PF_ERR_ARG;
    if (W && (!chrom || !win_start || !win_end || !t->win_read_off || t->win_read_off[W] > t->n_reads)) return PF_ERR_ARG;
    if (W && t->win_read_off[W] && (!t->n_used || !t->llr || !t->verdict || !t->hp || !qname_off || !qname)) return PF_ERR_ARG;
    for (uint32_t w = 0; w < W; w++)
        if (t->win_read_off[w] > t->win_read_off[w + 1]) return PF_ERR_ARG;
    FILE *fp = fopen(path, header ? "w" : "a");
    if (!fp) return -1;
    if (header) fprintf(fp, "#qname\tchrom\tstart\tend\thp\tn_calls\tllr\tverdict\n");
    for (uint32_t w = 0; w < W; w++)
        for (uint32_t r = t->win_read_off[w]; r < t->win_read_off[w + 1]; r++) {
            if (t->hp[r] > 1u || t->n_used[r] < 1u) continue;
            const uint32_t rec = rec_of_read ? rec_of_read[r] : r;
            const uint8_t v = t->verdict[r];
            fprintf(fp, "%.*s\t%s\t%u\t%u\t%s\t%u\t%.4f\t%s\n", (int)(qname_off[rec + 1] - qname_off[rec]),
                    qname + qname_off[rec], chrom, win_start[w], win_end[w], t->hp[r] == 0 ? "1" : "2", t->n_used[r],
                    (double)t->llr[r] / 65536.0, v == PF_TAGCHECK_OK ? "ok" : v == PF_TAGCHECK_FLIP ? "flip" : ".");
            if (n_lines) ++*n_lines;
        }
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

int pf_write_tagcheck_regions(const char *path, const char *chrom, const pf_tagcheck_t *t, const uint32_t *win_start,
                              const uint32_t *win_end, int header, uint64_t *n_lines) {
    if (n_lines) *n_lines = 0;
    const uint32_t W = t ? t->n_windows : 0;
    if (!path || (W && (!chrom || !win_start || !win_end || !t->win_n))) return PF_ERR_ARG;
    FILE *fp = fopen(path, header ? "w" : "a");
    if (!fp) return -1;
    if (header)
        fprintf(fp, "#chrom\tstart\tend\treads_h1\tscored_h1\tok_h1\tflip_h1\treads_h2\tscored_h2\tok_h2\tflip_h2\n");
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t *n = t->win_n + 8ull * w;
        fprintf(fp, "%s\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", chrom, win_start[w], win_end[w], n[0], n[1], n[2], n[3],
                n[4], n[5], n[6], n[7]);
        if (n_lines) ++*n_lines;
    }
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

/* ---- given regions: the q-values and the writer */
typedef struct { uint32_t hits; uint64_t i; } bh_ent_t;

static int cmp_bh(const void *a, const void *b) {
    const bh_ent_t *x = (const bh_ent_t *)a, *y = (const bh_ent_t *)b;
    if (x->hits != y->hits) return x->hits < y->hits ? -1 : 1;
    return x->i < y->i ? -1 : x->i > y->i;
}

int pf_bh_adjust(const uint32_t *hits, const uint8_t *tested, uint64_t n, uint32_t n_perm, double *q) {
    if (n && (!hits || !tested || !q)) return PF_ERR_ARG;
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++) {
        q[i] = NAN;
        if (tested[i]) m++;
    }
    if (!m) return PF_OK;
    bh_ent_t *v = (bh_ent_t *)malloc(m * sizeof *v);
    if (!v) return PF_ERR_NOMEM;
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++)
        if (tested[i]) { v[k].hits = hits[i]; v[k].i = i; k++; }
    qsort(v, m, sizeof *v, cmp_bh);
    /* from the largest hits down: a group of equal hits [a, b) has rank b, and
     * the minimum over everything at or above it is the running one */
    double run = 0.0;
    int have = 0;
    for (uint64_t b = m; b > 0;) {
        uint64_t a = b - 1;
        while (a > 0 && v[a - 1].hits == v[b - 1].hits) a--;
        const double p = ((double)v[a].hits + 1.0) / ((double)n_perm + 1.0);
        const double x = (p * (double)m) / (double)b;
        if (!have || x < run) run = x;
        have = 1;
        for (uint64_t j = a; j < b; j++) q[v[j].i] = run < 1.0 ? run : 1.0;
        b = a;
    }
    free(v);
    return PF_OK;
}

int pf_write_regions(const char *path, const pf_region_rec_t *rec, uint64_t n, int perm, uint32_t n_perm,
                     uint64_t *n_tested) {
    if (n_tested) *n_tested = 0;
    if (!path || (n && !rec)) return PF_ERR_ARG;
    double *q = NULL;
    if (perm && n) {
        uint32_t *hits = (uint32_t *)malloc(4ull * n);
        uint8_t *tested = (uint8_t *)malloc(n);
        q = (double *)malloc(8ull * n);
        int rc = hits && tested && q ? PF_OK : PF_ERR_NOMEM;
        for (uint64_t i = 0; i < n && !rc; i++) {
            hits[i] = rec[i].hits;
            tested[i] = (rec[i].flags & PF_REGION_ELIGIBLE) && rec[i].status == 0;
        }
        if (!rc) rc = pf_bh_adjust(hits, tested, n, n_perm, q);
        free(hits);
        free(tested);
        if (rc) { free(q); return rc; }
    }
    FILE *fp = fopen(path, "w");
    if (!fp) { free(q); return -1; }
    fprintf(fp, "#chrom\tstart\tend\tname\tn_cpg\tn_sites\tn_h1gt\tn_h2gt\tdir\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta"
            "\tpooled_p\tllr_bits\tblock%s\n", perm ? "\treads_h1\treads_h2\tperm_p\tperm_q" : "");
    for (uint64_t i = 0; i < n; i++) {
        const pf_region_rec_t *r = rec + i;
        const uint64_t m1 = r->s.sum[0], u1 = r->s.sum[1], m2 = r->s.sum[2], u2 = r->s.sum[3];
        const unsigned __int128 lhs = (unsigned __int128)m1 * (m2 + u2), rhs = (unsigned __int128)m2 * (m1 + u1);
        const double delta = (m1 + u1 ? (double)m1 / (double)(m1 + u1) : 0.0) - (m2 + u2 ? (double)m2 / (double)(m2 + u2) : 0.0);
        fprintf(fp, "%s\t%u\t%u\t%s\t%u\t%u\t%u\t%u\t%s\t%llu\t%llu\t%llu\t%llu\t%.4f\t", r->chrom ? r->chrom : ".", r->start,
                r->end, r->name ? r->name : ".", r->s.n_cpg, r->s.n_sites, r->s.n_pos, r->s.n_neg,
                lhs > rhs ? "h1>h2" : lhs < rhs ? "h1<h2" : ".", (unsigned long long)m1, (unsigned long long)u1,
                (unsigned long long)m2, (unsigned long long)u2, delta);
        if ((m1 | u1 | m2 | u2) > (uint64_t)INT32_MAX) fputc('.', fp);
        else {
            double two = 1.0;
            (void)pf_fisher_exact((int)m1, (int)u1, (int)m2, (int)u2, NULL, NULL, &two);
            fprintf(fp, "%.6g", two);
        }
        fprintf(fp, "\t%.3f\t%s", (double)r->s.evidence / 65536.0, (r->flags & PF_REGION_SPLIT) ? "split" : "ok");
        if (perm) {
            if (!(r->flags & PF_REGION_ELIGIBLE)) fprintf(fp, "\t.\t.\t.\t.");
            else if (r->status != 0) fprintf(fp, "\t%u\t%u\t.\t.", r->reads[0], r->reads[1]);
            else {
                fprintf(fp, "\t%u\t%u\t%.6g\t%.6g", r->reads[0], r->reads[1],
                        ((double)r->hits + 1.0) / ((double)n_perm + 1.0), q[i]);
                if (n_tested) ++*n_tested;
            }
        }
        fputc('\n', fp);
    }
    free(q);
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

/* ---- the rank test: the p-value, the q-values of doubles and the writer */
int pf_rank_p(uint64_t u2, uint32_t n1, uint32_t n2, uint64_t ties, double *auc, double *z, double *p) {
    if (n1 == 0 || n2 == 0 || u2 > 2ull * (uint64_t)n1 * (uint64_t)n2) return PF_ERR_ARG;
    const double a = (double)n1 * (double)n2;
    const double n = (double)n1 + (double)n2;
    const double u = (double)u2;
    const double var = (a / 12.0) * ((n + 1.0) - (double)ties / (n * (n - 1.0)));
    double zz = 0.0, pp = 1.0;
    if (var > 0.0) {
        double d = fabs(u - a) / 2.0 - 0.5;
        if (!(d > 0.0)) d = 0.0;
        zz = d / sqrt(var);
        pp = erfc(zz / sqrt(2.0));
        if (pp > 1.0) pp = 1.0;
    }
    if (auc) *auc = u / (2.0 * a);
    if (z) *z = zz;
    if (p) *p = pp;
    return PF_OK;
}

typedef struct { double p; uint64_t i; } bhp_ent_t;

static int cmp_bhp(const void *a, const void *b) {
    const bhp_ent_t *x = (const bhp_ent_t *)a, *y = (const bhp_ent_t *)b;
    if (x->p != y->p) return x->p < y->p ? -1 : 1;
    return x->i < y->i ? -1 : x->i > y->i;
}

int pf_bh_adjust_p(const double *p, const uint8_t *tested, uint64_t n, double *q) {
    if (n && (!p || !tested || !q)) return PF_ERR_ARG;
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++)
        if (tested[i]) {
            if (p[i] != p[i]) return PF_ERR_ARG;
            m++;
        }
    for (uint64_t i = 0; i < n; i++) q[i] = NAN;
    if (!m) return PF_OK;
    bhp_ent_t *v = (bhp_ent_t *)malloc(m * sizeof *v);
    if (!v) return PF_ERR_NOMEM;
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++)
        if (tested[i]) { v[k].p = p[i]; v[k].i = i; k++; }
    qsort(v, m, sizeof *v, cmp_bhp);
    /* as pf_bh_adjust: from the largest p down, a group of equal p [a, b) has rank b */
    double run = 0.0;
    int have = 0;
    for (uint64_t b = m; b > 0;) {
        uint64_t a = b - 1;
        while (a > 0 && v[a - 1].p == v[b - 1].p) a--;
        const double x = (v[a].p * (double)m) / (double)b;
        if (!have || x < run) run = x;
        have = 1;
        for (uint64_t j = a; j < b; j++) q[v[j].i] = run < 1.0 ? run : 1.0;
        b = a;
    }
    free(v);
    return PF_OK;
}

int pf_rank_exact_p(uint64_t count, uint64_t total, double *p) {
    if (total == 0 || count > total) return PF_ERR_ARG;
    if (p) *p = (double)count / (double)total;
    return PF_OK;
}

/* the rank file; with xrec the three columns of the exact test after
 * pf_write_rank's line, with trec the six columns of a tile (a split tile is
 * not tested) */
static int rank_file(const char *path, const pf_rank_rec_t *rec, const pf_rank_exact_rec_t *xrec,
                     const pf_rank_tile_rec_t *trec, uint64_t n, int bh, uint64_t *n_tested, uint64_t *n_exact) {
    if (n_tested) *n_tested = 0;
    if (n_exact) *n_exact = 0;
    if (!path || (n && !rec)) return PF_ERR_ARG;
    double *pv = NULL, *q = NULL, *bp = NULL, *bq = NULL;
    uint8_t *tested = NULL, *best = NULL;
    if (n) {
        const int x = xrec != NULL;
        pv = (double *)malloc(8ull * n);
        q = (double *)malloc(8ull * n);
        tested = (uint8_t *)malloc(n);
        bp = x ? (double *)malloc(8ull * n) : NULL;
        bq = x ? (double *)malloc(8ull * n) : NULL;
        best = x ? (uint8_t *)malloc(n) : NULL;
        int rc = pv && q && tested && (!x || (bp && bq && best)) ? PF_OK : PF_ERR_NOMEM;
        for (uint64_t i = 0; i < n && !rc; i++) {
            pv[i] = 1.0;
            tested[i] = rec[i].status == 0 && !(trec && trec[i].split);
            if (tested[i]) rc = pf_rank_p(rec[i].u2, rec[i].reads[0], rec[i].reads[1], rec[i].ties, NULL, NULL, pv + i);
            if (x && !rc) {
                bp[i] = pv[i];
                best[i] = tested[i];
                if (xrec[i].status == 0) {
                    rc = pf_rank_exact_p(xrec[i].two, xrec[i].total, bp + i);
                    best[i] = 1;
                }
            }
        }
        if (!rc && bh) rc = pf_bh_adjust_p(pv, tested, n, q);
        if (!rc && bh && x) rc = pf_bh_adjust_p(bp, best, n, bq);
        if (rc) { free(pv); free(q); free(tested); free(bp); free(bq); free(best); return rc; }
    }
    FILE *fp = fopen(path, "w");
    if (!fp) { free(pv); free(q); free(tested); free(bp); free(bq); free(best); return -1; }
    fprintf(fp, "#chrom\tstart\tend\treads_h1\treads_h2\tshort_h1\tshort_h2\tallmeth_h1\tallunmeth_h1\tmixed_h1\tallmeth_h2"
            "\tallunmeth_h2\tmixed_h2\tauc\tz\trank_p\trank_q%s%s\n", xrec ? "\texact_p\tbest_p\tbest_q" : "",
            trec ? "\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta\tblock" : "");
    for (uint64_t i = 0; i < n; i++) {
        const pf_rank_rec_t *r = rec + i;
        fprintf(fp, "%s\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u", r->chrom ? r->chrom : ".", r->start, r->end,
                r->reads[0], r->reads[1], r->n_short[0], r->n_short[1], r->cls[0], r->cls[1], r->cls[2], r->cls[3], r->cls[4],
                r->cls[5]);
        if (!tested[i]) fprintf(fp, "\t.\t.\t.\t.");
        else {
            double auc = 0.0, z = 0.0, p = 1.0;
            (void)pf_rank_p(r->u2, r->reads[0], r->reads[1], r->ties, &auc, &z, &p);
            fprintf(fp, "\t%.4f\t%.3f\t%.6g\t", auc, z, p);
            if (bh) fprintf(fp, "%.6g", q[i]); else fprintf(fp, ".");
            if (n_tested) ++*n_tested;
        }
        if (xrec) {
            if (xrec[i].status == 0) {
                fprintf(fp, "\t%.6g", bp[i]);
                if (n_exact) ++*n_exact;
            } else fprintf(fp, "\t.");
            if (!best[i]) fprintf(fp, "\t.\t.");
            else {
                fprintf(fp, "\t%.6g\t", bp[i]);
                if (bh) fprintf(fp, "%.6g", bq[i]); else fprintf(fp, ".");
            }
        }
        if (trec) {
            const uint64_t *c = trec[i].sum;
            fprintf(fp, "\t%llu\t%llu\t%llu\t%llu\t", (unsigned long long)c[0], (unsigned long long)c[1],
                    (unsigned long long)c[2], (unsigned long long)c[3]);
            if (c[0] + c[1] && c[2] + c[3])
                fprintf(fp, "%.4f", (double)c[0] / (double)(c[0] + c[1]) - (double)c[2] / (double)(c[2] + c[3]));
            else fputc('.', fp);
            fprintf(fp, "\t%s", trec[i].split ? "split" : "ok");
        }
        fputc('\n', fp);
    }
    free(pv);
    free(q);
    free(tested);
    free(bp);
    free(bq);
    free(best);
    const int bad = ferror(fp);
    if (fclose(fp) != 0 || bad) return -1;
    return PF_OK;
}

int pf_write_rank(const char *path, const pf_rank_rec_t *rec, uint64_t n, int bh, uint64_t *n_tested) {
    return rank_file(path, rec, NULL, NULL, n, bh, n_tested, NULL);
}

int pf_write_rank_tiles(const char *path, const pf_rank_rec_t *rec, const pf_rank_tile_rec_t *trec, uint64_t n,
                        uint64_t *n_tested) {
    if (n_tested) *n_tested = 0;
    if (n && !trec) return PF_ERR_ARG;
    static const pf_rank_tile_rec_t none = {{0, 0, 0, 0}, 0};
    return rank_file(path, rec, NULL, trec ? trec : &none, n, 1, n_tested, NULL);
}

int pf_write_rank_exact(const char *path, const pf_rank_rec_t *rec, const pf_rank_exact_rec_t *xrec, uint64_t n, int bh,
                        uint64_t *n_tested, uint64_t *n_exact) {
    if (n_tested) *n_tested = 0;
    if (n_exact) *n_exact = 0;
    if (n && !xrec) return PF_ERR_ARG;
    static const pf_rank_exact_rec_t none = {0, 0, 1};
    return rank_file(path, rec, xrec ? xrec : &none, NULL, n, bh, n_tested, n_exact);
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
    /* --dmr */
    const pf_hapmeth_dmr_t *dmr;
    char *dpath;
    pf_gaps_t *blocks;         /* dmr->blocks_path's phase blocks */
    uint32_t *brk;             /* the current contig's breaks */
    uint32_t n_brk;
    pf_dmr_acc_t *acc;         /* the current contig's accumulator */
    pf_hapmeth_dmr_stats_t dst;
    /* --dmr-perm */
    const pf_hapmeth_perm_t *perm;
    uint32_t jw;               /* windows per job */
    pf_hapmeth_perm_stats_t pst;
    /* --assign */
    const pf_hapmeth_assign_t *assign;
    char *apath;
    pf_hapmeth_assign_stats_t ast;
    /* --tag-check */
    const pf_hapmeth_tagcheck_t *tagcheck;
    const pf_hapmeth_assign_t *rule;   /* the thresholds it checks; NULL: the defaults */
    char *tpath, *trpath;
    pf_hapmeth_tagcheck_stats_t tst;
    /* --dmr-hmm */
    const pf_hapmeth_hmm_t *hmm;
    uint32_t *hpos, *hcnt;     /* the current contig's informative sites: position, six counts */
    uint64_t hn, hcap;
    pf_hapmeth_hmm_stats_t hst;
    /* --regions */
    const pf_hapmeth_regions_t *regions;
    pf_region_list_t *rlist;
    char *rpath;
    pf_region_rec_t *rec;      /* the run's kept regions, in the file's order */
    size_t nrec, mrec;
    uint32_t *ks, *ke, *kmax;  /* the current contig's kept regions: start, end, the largest end so far */
    uint64_t kn;
    size_t rec0;               /* rec + rec0: the current contig's */
    pf_hapmeth_regions_stats_t rst;
    /* --dmr-rank */
    const pf_hapmeth_rank_t *rank;
    char *kpath;
    pf_rank_rec_t *krec;       /* the run's regions of the second pass, in the pass's order */
    size_t nk, mk;
    pf_hapmeth_rank_stats_t kst;
    /* --dmr-rank-exact */
    const pf_hapmeth_rank_exact_t *exact;
    pf_rank_exact_rec_t *xrec; /* parallel to krec */
    size_t mx;
    pf_hapmeth_rank_exact_stats_t xst;
    /* --tile */
    const pf_hapmeth_tiles_t *tiles;
    char *lpath;
    pf_rank_rec_t *lrec;       /* the run's tiles with a participating read, in genome order */
    pf_rank_tile_rec_t *ltrec; /* parallel to lrec */
    size_t nl, ml;
    pf_hapmeth_tiles_stats_t lst;
} hm_t;

/* pf_rank.hip: pf_batch_rankranges on a batch whose load stage has just run (not in the public header) */
int pf_batch_rankranges_loaded(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                               const uint64_t *rng_off, const uint32_t *rng_start, const uint32_t *rng_end, pf_rank_t **out);

/* the fetch of one job, the same in both passes: the records of the windows
 * ws/we[0, n) of chrom as a record-level batch, no read-back margin */
static int hm_fetch(hm_t *H, const char *chrom, uint32_t n, const uint32_t *ws, const uint32_t *we, pf_dbatch_t **db,
                    pf_bam_dev_fetch_t **F, pf_bam_records_t **recs, uint64_t *n_records) {
    int rc;
    if (H->o->host_fetch) {
        rc = pf_bam_fetch_windows(H->bam, chrom, n, ws, we, 0, H->o->threads > 0 ? H->o->threads : 1, recs);
        if (!rc) {
            *n_records += (*recs)->aln.n_recs;
            rc = pf_batch_upload_aln(H->ctx, &H->cfg, &H->lc, &(*recs)->aln, db);
        }
    } else {
        rc = pf_batch_upload_bam(H->ctx, &H->cfg, &H->lc, H->bam, chrom, n, ws, we, 0, 0, db, F);
        if (!rc) *n_records += (*F)->n_recs;
    }
    return rc;
}

/* --dmr-hmm: the job's informative sites join the contig's */
static int hm_keep(hm_t *H, const pf_pileup_t *pile) {
    const uint32_t mc = H->dmr->cfg.min_cov;
    for (uint64_t i = 0; i < pile->n_sites; i++) {
        const uint32_t *c = pile->cnt + 6 * i;
        if (c[0] + c[1] < mc || c[2] + c[3] < mc) continue;
        if (H->hn == H->hcap) {
            const uint64_t nc = H->hcap ? H->hcap * 2 : 4096;
            uint32_t *p = (uint32_t *)realloc(H->hpos, 4ull * nc);
            if (!p) return PF_ERR_NOMEM;
            H->hpos = p;
            uint32_t *q = (uint32_t *)realloc(H->hcnt, 24ull * nc);
            if (!q) return PF_ERR_NOMEM;
            H->hcnt = q;
            H->hcap = nc;
        }
        H->hpos[H->hn] = pile->pos[i];
        memcpy(H->hcnt + 6 * H->hn, c, 16);
        H->hcnt[6 * H->hn + 4] = H->hcnt[6 * H->hn + 5] = 0;
        H->hn++;
    }
    return PF_OK;
}

/* --dmr-hmm: the contig's kept sites as one range through the model */
static int hm_model(hm_t *H, pf_dmr_t **fin) {
    *fin = NULL;
    const uint64_t off[2] = {0, H->hn};
    pf_pileup_t one;
    memset(&one, 0, sizeof one);
    one.n_windows = 1; one.n_sites = H->hn; one.win_off = off; one.pos = H->hpos; one.cnt = H->hcnt;
    pf_dmr_hmm_t *h = NULL;
    int rc = pf_dmr_hmm_regions(H->ctx, &one, 0, 1, &H->dmr->cfg, &H->hmm->cfg, H->brk, H->n_brk, 0, 0, &h);
    H->hn = 0;
    if (rc) return rc;
    pf_dmr_t *d = (pf_dmr_t *)calloc(1, sizeof *d);
    pf_dmr_run_t *r = h->n_runs ? (pf_dmr_run_t *)malloc(h->n_runs * sizeof *r) : NULL;
    if (!d || (h->n_runs && !r)) { free(d); free(r); pf_dmr_hmm_free(h); return PF_ERR_NOMEM; }
    if (h->n_runs) memcpy(r, h->runs, h->n_runs * sizeof *r);
    d->n_runs = h->n_runs;
    d->runs = r;                                             /* pf_dmr_free */
    d->n_informative = h->n_informative;
    H->dst.ms_kernels += h->ms_kernels;
    H->hst.ms_kernels += h->ms_kernels;
    H->hst.n_chains += h->n_chains;
    pf_dmr_hmm_free(h);
    *fin = d;
    return PF_OK;
}

/* --regions: the contig's regions that lie in [s, e) (all of them without
 * opts.region) join the run's records with zero sums; H->brk is the contig's */
static int hm_regions_begin(hm_t *H, int32_t tid, const char *chrom, uint32_t s, uint32_t e) {
    const uint32_t *rs, *re;
    const char *const *rn;
    uint64_t n;
    int rc = pf_regions_contig(H->rlist, (uint32_t)tid, &rs, &re, &rn, &n);
    if (rc) return rc;
    free(H->ks); free(H->ke); free(H->kmax);
    H->ks = (uint32_t *)malloc(4ull * (n ? n : 1));
    H->ke = (uint32_t *)malloc(4ull * (n ? n : 1));
    H->kmax = (uint32_t *)malloc(4ull * (n ? n : 1));
    H->kn = 0;
    H->rec0 = H->nrec;
    if (!H->ks || !H->ke || !H->kmax) return PF_ERR_NOMEM;
    for (uint64_t i = 0; i < n; i++) {
        if (H->o->region && (rs[i] < s || re[i] > e)) { H->rst.n_outside++; continue; }
        if (H->nrec == H->mrec) {
            const size_t nm = H->mrec ? H->mrec * 2 : 256;
            pf_region_rec_t *p = (pf_region_rec_t *)realloc(H->rec, nm * sizeof *p);
            if (!p) return PF_ERR_NOMEM;
            H->rec = p;
            H->mrec = nm;
        }
        pf_region_rec_t *r = H->rec + H->nrec++;
        memset(r, 0, sizeof *r);
        r->chrom = chrom; r->name = rn[i]; r->start = rs[i]; r->end = re[i];
        uint32_t lo = 0, hi = H->n_brk;                      /* breaks <= start */
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (H->brk[mid] <= rs[i]) lo = mid + 1; else hi = mid;
        }
        if (lo < H->n_brk && H->brk[lo] < re[i]) { r->flags |= PF_REGION_SPLIT; H->rst.n_split++; }
        H->ks[H->kn] = rs[i];
        H->ke[H->kn] = re[i];
        H->kmax[H->kn] = H->kn && H->kmax[H->kn - 1] > re[i] ? H->kmax[H->kn - 1] : re[i];
        H->kn++;
    }
    return PF_OK;
}

/* --regions: the job's windows span [a, b); the contig's regions that can
 * hold a site of it -- a superset: start < b, and some region up to it ends
 * past a -- are summed over the job's sites and added to their records */
static int hm_regions_job(hm_t *H, const pf_pileup_t *pile, uint32_t n, uint32_t a, uint32_t b) {
    uint64_t lo = 0, hi = H->kn;
    while (lo < hi) {                                        /* starts < b */
        const uint64_t mid = lo + (hi - lo) / 2;
        if (H->ks[mid] < b) lo = mid + 1; else hi = mid;
    }
    const uint64_t i1 = lo;
    lo = 0; hi = i1;
    while (lo < hi) {                                        /* largest end so far <= a */
        const uint64_t mid = lo + (hi - lo) / 2;
        if (H->kmax[mid] <= a) lo = mid + 1; else hi = mid;
    }
    const uint64_t i0 = lo;
    if (i0 >= i1) return PF_OK;
    pf_regions_t *part = NULL;
    int rc = pf_region_sums(H->ctx, pile, 0, n, &H->dmr->cfg, H->ks + i0, H->ke + i0, i1 - i0, 0, &part);
    if (rc) return rc;
    for (uint64_t k = 0; k < part->n; k++) {
        pf_region_sum_t *d = &H->rec[H->rec0 + i0 + k].s;
        const pf_region_sum_t *x = part->r + k;
        d->n_cpg += x->n_cpg; d->n_sites += x->n_sites; d->n_pos += x->n_pos; d->n_neg += x->n_neg;
        for (int q = 0; q < 4; q++) d->sum[q] += x->sum[q];
        d->evidence += x->evidence;
    }
    H->rst.ms_kernels += part->ms_kernels;
    pf_regions_free(part);
    return PF_OK;
}

/* --tile: the tiles of the job's windows -- window [a, b) holds [a + j*T, min(a
 * + (j+1)*T, b)) -- as the ranges of one pf_batch_rankranges call on the batch
 * the pileup has just loaded; a tile with a participating read becomes a
 * record */
static int hm_tiles_job(hm_t *H, const char *chrom, pf_dbatch_t *db, uint32_t n, const uint32_t *ws, const uint32_t *we) {
    const uint32_t T = H->tiles->tile;
    uint64_t *off = (uint64_t *)malloc(8ull * ((size_t)n + 1));
    if (!off) return PF_ERR_NOMEM;
    off[0] = 0;
    for (uint32_t w = 0; w < n; w++) off[w + 1] = off[w] + ((uint64_t)(we[w] - ws[w]) + T - 1) / T;
    const uint64_t nr = off[n];
    uint32_t *rs = (uint32_t *)malloc(4ull * (nr ? nr : 1)), *re = (uint32_t *)malloc(4ull * (nr ? nr : 1));
    pf_rank_t *rk = NULL;
    int rc = rs && re ? PF_OK : PF_ERR_NOMEM;
    for (uint32_t w = 0; w < n && !rc; w++)
        for (uint64_t i = off[w]; i < off[w + 1]; i++) {
            const uint64_t a = (uint64_t)ws[w] + (i - off[w]) * T, b = a + T;
            rs[i] = (uint32_t)a;
            re[i] = b < we[w] ? (uint32_t)b : we[w];
        }
    if (!rc) rc = pf_batch_rankranges_loaded(H->ctx, db, NULL, 0, H->tiles->min_calls, off, rs, re, &rk);
    if (!rc && rk->n_windows != nr) rc = PF_ERR_INTERNAL;
    for (uint64_t i = 0; i < nr && !rc; i++) {
        const uint32_t *c = rk->n_reads + 2 * i, *sh = rk->n_short + 2 * i;
        if (!(c[0] + sh[0]) && !(c[1] + sh[1])) continue;      /* no participating read */
        if (H->nl == H->ml) {
            const size_t nm = H->ml ? H->ml * 2 : 1024;
            pf_rank_rec_t *p = (pf_rank_rec_t *)realloc(H->lrec, nm * sizeof *p);
            if (p) H->lrec = p;
            pf_rank_tile_rec_t *q = p ? (pf_rank_tile_rec_t *)realloc(H->ltrec, nm * sizeof *q) : NULL;
            if (q) H->ltrec = q;
            if (!p || !q) { rc = PF_ERR_NOMEM; break; }
            H->ml = nm;
        }
        pf_rank_rec_t *r = H->lrec + H->nl;
        pf_rank_tile_rec_t *t = H->ltrec + H->nl;
        H->nl++;
        memset(r, 0, sizeof *r);
        memset(t, 0, sizeof *t);
        r->chrom = chrom; r->start = rs[i]; r->end = re[i];
        for (int q = 0; q < 2; q++) { r->reads[q] = c[q]; r->n_short[q] = sh[q]; }
        for (int q = 0; q < 6; q++) r->cls[q] = rk->cls[6 * i + q];
        r->status = rk->status[i]; r->u2 = rk->u2[i]; r->ties = rk->ties[i];
        for (int q = 0; q < 4; q++) t->sum[q] = rk->sum[4 * i + q];
        uint32_t lo = 0, hi = H->n_brk;                      /* breaks <= start */
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (H->brk[mid] <= rs[i]) lo = mid + 1; else hi = mid;
        }
        if (lo < H->n_brk && H->brk[lo] < re[i]) { t->split = 1; H->lst.n_split++; }
    }
    if (!rc) H->lst.ms_kernels += rk->ms_kernels;
    pf_rank_free(rk);
    free(off);
    free(rs);
    free(re);
    return rc;
}

/* one job: the windows ws/we[0, n) of chrom */
static int hm_job(hm_t *H, const char *chrom, uint32_t n, const uint32_t *ws, const uint32_t *we) {
    pf_dbatch_t *db = NULL;
    pf_bam_dev_fetch_t *F = NULL;
    pf_bam_records_t *recs = NULL;
    pf_pileup_t *pile = NULL;
    int rc = hm_fetch(H, chrom, n, ws, we, &db, &F, &recs, &H->st.n_records);
    if (rc == PF_ERR_LIMIT)
        fprintf(stderr, "[E::pf_hapmeth_main] %s:%u-%u: a window exceeds a device limit (65,535 records per window); "
                "try a smaller --chunk-size\n", chrom, ws[0] + 1, we[n - 1]);
    if (!rc) rc = pf_batch_pileup(H->ctx, db, NULL, 0, &pile);
    if (!rc && H->tiles) rc = hm_tiles_job(H, chrom, db, n, ws, we);      /* nothing in between: the calls as they stand */
    if (!rc) rc = pf_write_hapmeth(H->path, chrom, pile, 0, n, 0);
    if (!rc) {
        H->st.n_sites += pile->n_sites;
        H->st.ms_kernels += pile->ms_kernels;
    }
    if (!rc && H->hmm) rc = hm_keep(H, pile);
    if (!rc && H->regions) rc = hm_regions_job(H, pile, n, ws[0], we[n - 1]);
    if (!rc && H->dmr && !H->hmm && !H->regions) {
        pf_dmr_t *part = NULL;
        rc = pf_dmr_regions(H->ctx, pile, 0, n, &H->dmr->cfg, H->brk, H->n_brk, &part);
        if (!rc) rc = pf_dmr_acc_add(H->acc, part);
        if (!rc) H->dst.ms_kernels += part->ms_kernels;
        pf_dmr_free(part);
    }
    pf_pileup_free(pile);
    if (db) pf_batch_free(db);
    if (F) pf_bam_dev_fetch_free(F);
    if (recs) pf_bam_records_free(recs);
    return rc;
}

static int cmp_u32(const void *a, const void *b) {
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

/* the breaks of chrom: each phase block's 0-based start and its end, sorted */
static int hm_breaks(hm_t *H, const char *chrom) {
    free(H->brk);
    H->brk = NULL;
    H->n_brk = 0;
    const pf_gaps_t *g = H->blocks;
    if (!g) return PF_OK;
    uint32_t c = 0;
    while (c < g->n_contigs && strcmp(g->names[c], chrom)) c++;
    if (c == g->n_contigs) return PF_OK;
    const uint64_t r0 = g->raw_off[c], nr = g->raw_off[c + 1] - r0;       /* nr gaps: nr + 1 blocks */
    if (nr > 0x3FFFFFFFull) return PF_ERR_LIMIT;
    H->brk = (uint32_t *)malloc(8ull * (nr + 1));
    if (!H->brk) return PF_ERR_NOMEM;
    for (uint64_t k = 0; k <= nr; k++) {
        const uint32_t bs = k ? g->raw_end[r0 + k - 1] : g->abs_start[c]; /* 1-based */
        const uint32_t be = k < nr ? g->raw_start[r0 + k] : g->abs_end[c];
        H->brk[H->n_brk++] = bs ? bs - 1u : 0u;
        H->brk[H->n_brk++] = be;
    }
    qsort(H->brk, H->n_brk, 4, cmp_u32);
    return PF_OK;
}

/* the second pass over a contig's final regions, for --dmr-perm, --assign and
 * --tag-check (pf_batch_tagcheck on the same batch, its lines appended to the
 * two tag-check files job by job):
 * the regions that pass max_p are the windows [start, end) of jobs of at most
 * jw windows, each fetched once as in the first pass; on that batch, under the
 * records' HP tags, pf_batch_permtest (run k's result lands in window k of
 * *out; malloc'ed arrays: pf_perm_free) and / or pf_batch_assign, whose lines
 * are appended to the assign file job by job (region order) */
static int hm_second(hm_t *H, const char *chrom, const pf_dmr_t *fin, pf_perm_t **out) {
    *out = NULL;
    const uint64_t n = fin->n_runs;
    if (n > 0xFFFFFFFFull) return PF_ERR_LIMIT;
    pf_perm_t *P = NULL;
    uint32_t *nr = NULL, *hits = NULL, *stat = NULL;
    uint64_t *sum = NULL;
    int rc = PF_OK;
    if (H->perm) {
        P = (pf_perm_t *)calloc(1, sizeof *P);
        if (!P) return PF_ERR_NOMEM;
        nr = (uint32_t *)calloc(2 * n + 1, 4); hits = (uint32_t *)calloc(n + 1, 4); stat = (uint32_t *)calloc(n + 1, 4);
        sum = (uint64_t *)calloc(4 * n + 1, 8);
        P->n_windows = (uint32_t)n; P->n_perm = H->perm->n_perm; P->seed = H->perm->seed;
        P->n_reads = nr; P->sum = sum; P->hits = hits; P->status = stat;
        if (!nr || !hits || !stat || !sum) rc = PF_ERR_NOMEM;
    }
    uint32_t *ws = (uint32_t *)malloc(4ull * H->jw), *we = (uint32_t *)malloc(4ull * H->jw);
    uint64_t *idx = (uint64_t *)malloc(8ull * H->jw);
    if (!ws || !we || !idx) rc = PF_ERR_NOMEM;
    uint32_t k = 0;
    for (uint64_t i = 0; i <= n && !rc; i++) {
        if (i < n) {
            const pf_dmr_run_t *r = fin->runs + i;
            double two = 1.0;
            if ((r->sum[0] | r->sum[1] | r->sum[2] | r->sum[3]) > (uint64_t)INT32_MAX) rc = PF_ERR_LIMIT;   /* as the writer */
            else (void)pf_fisher_exact((int)r->sum[0], (int)r->sum[1], (int)r->sum[2], (int)r->sum[3], NULL, NULL, &two);
            if (rc || two > H->dmr->max_p) continue;         /* no line: nothing to test */
            ws[k] = r->start; we[k] = r->end; idx[k] = i;
            k++;
        }
        if (k == 0 || (k < H->jw && i < n)) continue;
        pf_dbatch_t *db = NULL;
        pf_bam_dev_fetch_t *F = NULL;
        pf_bam_records_t *recs = NULL;
        pf_perm_t *part = NULL;
        pf_assign_t *as = NULL;
        pf_tagcheck_t *tc = NULL;
        uint64_t fetched = 0;
        rc = hm_fetch(H, chrom, k, ws, we, &db, &F, &recs, &fetched);
        if (H->perm) H->pst.n_records += fetched;
        if (H->assign) H->ast.n_records += fetched;
        if (H->tagcheck) H->tst.n_records += fetched;
        if (H->rank) H->kst.n_records += fetched;
        if (rc == PF_ERR_LIMIT)
            fprintf(stderr, "[E::pf_hapmeth_main] %s:%u-%u: a region exceeds a device limit (65,535 records per window)\n",
                    chrom, ws[0] + 1, we[k - 1]);
        if (!rc && H->perm) {
            rc = pf_batch_permtest(H->ctx, db, NULL, 0, H->perm->n_perm, H->perm->seed, &part);
            if (!rc && part->n_windows != k) rc = PF_ERR_INTERNAL;
            for (uint32_t j = 0; j < k && !rc; j++) {
                nr[2 * idx[j]] = part->n_reads[2 * j];
                nr[2 * idx[j] + 1] = part->n_reads[2 * j + 1];
                for (int q = 0; q < 4; q++) sum[4 * idx[j] + q] = part->sum[4 * j + q];
                hits[idx[j]] = part->hits[j];
                stat[idx[j]] = part->status[j];
            }
            if (!rc) H->pst.ms_kernels += part->ms_kernels;
        }
        if (!rc && H->rank) {
            pf_rank_t *rk = NULL;
            rc = pf_batch_ranktest(H->ctx, db, NULL, 0, H->rank->min_calls, &rk);
            if (!rc && rk->n_windows != k) rc = PF_ERR_INTERNAL;
            if (!rc && H->nk + k > H->mk) {
                size_t nm = H->mk ? H->mk * 2 : 256;
                while (nm < H->nk + k) nm *= 2;
                pf_rank_rec_t *p = (pf_rank_rec_t *)realloc(H->krec, nm * sizeof *p);
                if (!p) rc = PF_ERR_NOMEM;
                else { H->krec = p; H->mk = nm; }
            }
            for (uint32_t j = 0; j < k && !rc; j++) {
                pf_rank_rec_t *r = H->krec + H->nk++;
                memset(r, 0, sizeof *r);
                r->chrom = chrom; r->start = ws[j]; r->end = we[j];
                for (int q = 0; q < 2; q++) { r->reads[q] = rk->n_reads[2 * j + q]; r->n_short[q] = rk->n_short[2 * j + q]; }
                for (int q = 0; q < 6; q++) r->cls[q] = rk->cls[6 * j + q];
                r->status = rk->status[j]; r->u2 = rk->u2[j]; r->ties = rk->ties[j];
            }
            if (!rc) H->kst.ms_kernels += rk->ms_kernels;
            if (!rc && H->exact) {                     /* the same batch, the same min_calls: no further fetch */
                pf_rank_exact_t *xr = NULL;
                rc = pf_batch_rankexact(H->ctx, db, NULL, 0, H->rank->min_calls, H->exact->max_reads, &xr);
                if (!rc && xr->n_windows != k) rc = PF_ERR_INTERNAL;
                if (!rc && H->nk > H->mx) {
                    pf_rank_exact_rec_t *p = (pf_rank_exact_rec_t *)realloc(H->xrec, H->mk * sizeof *p);
                    if (!p) rc = PF_ERR_NOMEM;
                    else { H->xrec = p; H->mx = H->mk; }
                }
                for (uint32_t j = 0; j < k && !rc; j++) {
                    pf_rank_exact_rec_t *x = H->xrec + (H->nk - k + j);
                    if (xr->u2[j] != rk->u2[j] || xr->n_reads[2 * j] != rk->n_reads[2 * j] ||
                        xr->n_reads[2 * j + 1] != rk->n_reads[2 * j + 1])
                        rc = PF_ERR_INTERNAL;          /* the two kernels count the same reads */
                    x->two = xr->two[j]; x->total = xr->total[j]; x->status = xr->status[j];
                    if (x->status == 2) H->xst.n_over++;
                }
                if (!rc) H->xst.ms_kernels += xr->ms_kernels;
                pf_rank_exact_free(xr);
            }
            pf_rank_free(rk);
        }
        if (!rc && H->assign) {
            pf_assign_cfg_t ac;
            ac.min_cov = H->dmr->cfg.min_cov; ac.min_calls = H->assign->min_calls; ac.min_llr_q16 = H->assign->min_llr_q16;
            rc = pf_batch_assign(H->ctx, db, NULL, 0, &ac, &as);
            if (!rc && as->n_windows != k) rc = PF_ERR_INTERNAL;
            uint32_t *rec_of = NULL;
            if (!rc) {
                rec_of = (uint32_t *)malloc(4ull * as->n_reads + 4);
                rc = rec_of ? pf_batch_read_recs(db, rec_of, as->n_reads) : PF_ERR_NOMEM;
            }
            uint64_t lines = 0;
            if (!rc)
                rc = pf_write_assign(H->apath, chrom, as, ws, we, rec_of, recs ? recs->qname_off : F->qname_off,
                                     recs ? recs->qname : F->qname, 0, &lines);
            if (!rc) {
                H->ast.n_lines += lines;
                for (uint32_t j = 0; j < k; j++) {
                    H->ast.n_h1 += as->win_n[3 * j + 1];
                    H->ast.n_h2 += as->win_n[3 * j + 2];
                }
                H->ast.ms_kernels += as->ms_kernels;
            }
            free(rec_of);
        }
        if (!rc && H->tagcheck) {
            /* the rule being checked: --assign's thresholds, or its defaults */
            pf_assign_cfg_t ac;
            ac.min_cov = H->dmr->cfg.min_cov;
            ac.min_calls = H->rule ? H->rule->min_calls : 2u;
            ac.min_llr_q16 = H->rule ? H->rule->min_llr_q16 : 3 * 65536;
            rc = pf_batch_tagcheck(H->ctx, db, NULL, 0, &ac, &tc);
            if (!rc && tc->n_windows != k) rc = PF_ERR_INTERNAL;
            uint32_t *rec_of = NULL;
            if (!rc) {
                rec_of = (uint32_t *)malloc(4ull * tc->n_reads + 4);
                rc = rec_of ? pf_batch_read_recs(db, rec_of, tc->n_reads) : PF_ERR_NOMEM;
            }
            uint64_t lines = 0, regions = 0;
            if (!rc)
                rc = pf_write_tagcheck(H->tpath, chrom, tc, ws, we, rec_of, recs ? recs->qname_off : F->qname_off,
                                       recs ? recs->qname : F->qname, 0, &lines);
            if (!rc) rc = pf_write_tagcheck_regions(H->trpath, chrom, tc, ws, we, 0, &regions);
            if (!rc) {
                H->tst.n_lines += lines;
                H->tst.n_regions += regions;
                for (uint32_t j = 0; j < k; j++)
                    for (int h = 0; h < 2; h++) {
                        const uint32_t *c = tc->win_n + 8ull * j + 4 * h;
                        H->tst.n_ok[h] += c[2];
                        H->tst.n_flip[h] += c[3];
                        H->tst.n_undecided[h] += c[1] - c[2] - c[3];
                    }
                H->tst.ms_kernels += tc->ms_kernels;
            }
            free(rec_of);
        }
        pf_tagcheck_free(tc);
        pf_assign_free(as);
        pf_perm_free(part);
        if (db) pf_batch_free(db);
        if (F) pf_bam_dev_fetch_free(F);
        if (recs) pf_bam_records_free(recs);
        k = 0;
    }
    free(ws);
    free(we);
    free(idx);
    if (rc) pf_perm_free(P); else *out = P;
    return rc;
}

/* the contig's regions are complete: close the carry, (test, assign,) append */
static int hm_flush(hm_t *H, const char *chrom) {
    pf_dmr_t *fin = NULL;
    pf_perm_t *P = NULL;
    uint64_t lines = 0, dots = 0;
    int rc = H->hmm ? hm_model(H, &fin) : pf_dmr_acc_flush(H->acc, &fin);
    if (!rc && (H->perm || H->assign || H->tagcheck || H->rank)) rc = hm_second(H, chrom, fin, &P);
    if (!rc) rc = write_dmr(H->dpath, chrom, fin, P, H->dmr->max_p, 0, &lines, &dots);
    if (!rc) {
        H->dst.n_regions += lines;
        H->dst.n_informative += fin->n_informative;
        if (P) {
            H->pst.n_tested += lines - dots;
            H->pst.n_untested += dots;
        }
    }
    pf_perm_free(P);
    pf_dmr_free(fin);
    pf_dmr_acc_free(H->acc);
    H->acc = NULL;
    return rc;
}

/* --regions: the contig's sums are complete; its eligible regions go through
 * the second pass as the windows [start, end) */
static int hm_regions_flush(hm_t *H, const char *chrom) {
    if (!H->perm && !H->assign && !H->tagcheck && !H->rank) return PF_OK;
    pf_region_rec_t *rec = H->rec + H->rec0;
    const uint64_t n = H->kn;
    pf_dmr_t fin;
    memset(&fin, 0, sizeof fin);
    pf_dmr_run_t *runs = (pf_dmr_run_t *)calloc(n ? n : 1, sizeof *runs);
    uint64_t *of = (uint64_t *)malloc(8ull * (n ? n : 1));
    if (!runs || !of) { free(runs); free(of); return PF_ERR_NOMEM; }
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) {
        const pf_region_rec_t *r = rec + i;
        if ((r->flags & PF_REGION_SPLIT) || r->s.n_sites < H->dmr->cfg.min_sites || r->start >= r->end ||
            r->end - r->start > PF_REGION_TEST_MAX_SPAN ||
            (r->s.sum[0] | r->s.sum[1] | r->s.sum[2] | r->s.sum[3]) > (uint64_t)INT32_MAX)
            continue;
        double two = 1.0;
        (void)pf_fisher_exact((int)r->s.sum[0], (int)r->s.sum[1], (int)r->s.sum[2], (int)r->s.sum[3], NULL, NULL, &two);
        if (two > H->dmr->max_p) continue;
        runs[k].start = r->start; runs[k].end = r->end; runs[k].n_sites = r->s.n_sites; runs[k].sign = 1;
        for (int q = 0; q < 4; q++) runs[k].sum[q] = r->s.sum[q];
        of[k++] = i;
    }
    fin.n_runs = k;
    fin.runs = runs;
    pf_perm_t *P = NULL;
    int rc = hm_second(H, chrom, &fin, &P);                  /* takes every run: each passes max_p */
    for (uint64_t j = 0; j < k && !rc; j++) {
        pf_region_rec_t *r = rec + of[j];
        r->flags |= PF_REGION_ELIGIBLE;
        if (P) {
            r->reads[0] = P->n_reads[2 * j]; r->reads[1] = P->n_reads[2 * j + 1];
            r->hits = P->hits[j]; r->status = P->status[j];
        }
    }
    pf_perm_free(P);
    free(runs);
    free(of);
    return rc;
}

/* [s, e) of contig tid in windows of `chunk` bases, jobs of at most jw windows */
static int hm_span(hm_t *H, int32_t tid, uint32_t s, uint32_t e, uint32_t chunk, uint32_t jw, uint32_t *ws, uint32_t *we) {
    const char *chrom = pf_bam_target_name(H->bam, tid);
    uint32_t n = 0;
    int rc = PF_OK;
    if (H->dmr) {
        rc = hm_breaks(H, chrom);
        if (rc) return rc;
        H->hn = 0;
        if (H->regions) {
            rc = hm_regions_begin(H, tid, chrom, s, e);
            if (rc) return rc;
        } else if (!H->hmm) {
            H->acc = pf_dmr_acc_new(&H->dmr->cfg, H->brk, H->n_brk);
            if (!H->acc) return PF_ERR_NOMEM;
        }
    }
    if (H->tiles) {
        if (!H->dmr) rc = hm_breaks(H, chrom);               /* with dmr they are built above: one GTF, one array */
        if (rc) return rc;
        H->lst.n_tiles += ((uint64_t)(e - s) + H->tiles->tile - 1) / H->tiles->tile;   /* e >= s */
    }
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
    if (!rc && H->dmr) rc = H->regions ? hm_regions_flush(H, chrom) : hm_flush(H, chrom);
    return rc;
}

int pf_hapmeth_main(const pf_hapmeth_opts_t *o, pf_hapmeth_stats_t *stats) {
    return pf_hapmeth_run_perm(o, NULL, NULL, stats, NULL, NULL);
}

int pf_hapmeth_run(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, pf_hapmeth_stats_t *stats,
                   pf_hapmeth_dmr_stats_t *dstats) {
    return pf_hapmeth_run_perm(o, dmr, NULL, stats, dstats, NULL);
}

int pf_hapmeth_run_perm(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_perm_t *perm,
                        pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats, pf_hapmeth_perm_stats_t *pstats) {
    return pf_hapmeth_run_assign(o, dmr, perm, NULL, stats, dstats, pstats, NULL);
}

int pf_hapmeth_run_assign(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_perm_t *perm,
                          const pf_hapmeth_assign_t *assign, pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats,
                          pf_hapmeth_perm_stats_t *pstats, pf_hapmeth_assign_stats_t *astats) {
    return pf_hapmeth_run_tagcheck(o, dmr, perm, assign, NULL, stats, dstats, pstats, astats, NULL);
}

int pf_hapmeth_run_tagcheck(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_perm_t *perm,
                            const pf_hapmeth_assign_t *assign, const pf_hapmeth_tagcheck_t *tagcheck,
                            pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats, pf_hapmeth_perm_stats_t *pstats,
                            pf_hapmeth_assign_stats_t *astats, pf_hapmeth_tagcheck_stats_t *tstats) {
    return pf_hapmeth_run_hmm(o, dmr, NULL, perm, assign, tagcheck, stats, dstats, NULL, pstats, astats, tstats);
}

int pf_hapmeth_run_hmm(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                       const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                       const pf_hapmeth_tagcheck_t *tagcheck, pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats,
                       pf_hapmeth_hmm_stats_t *hstats, pf_hapmeth_perm_stats_t *pstats, pf_hapmeth_assign_stats_t *astats,
                       pf_hapmeth_tagcheck_stats_t *tstats) {
    return pf_hapmeth_run_regions(o, dmr, hmm, perm, assign, tagcheck, NULL, stats, dstats, hstats, pstats, astats, tstats,
                                  NULL);
}

int pf_hapmeth_run_regions(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                           const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                           const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                           pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats, pf_hapmeth_hmm_stats_t *hstats,
                           pf_hapmeth_perm_stats_t *pstats, pf_hapmeth_assign_stats_t *astats,
                           pf_hapmeth_tagcheck_stats_t *tstats, pf_hapmeth_regions_stats_t *rstats) {
    return pf_hapmeth_run_rank(o, dmr, hmm, perm, assign, tagcheck, regions, NULL, stats, dstats, hstats, pstats, astats,
                               tstats, rstats, NULL);
}

int pf_hapmeth_run_rank(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                        const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                        const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                        const pf_hapmeth_rank_t *rank, pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats,
                        pf_hapmeth_hmm_stats_t *hstats, pf_hapmeth_perm_stats_t *pstats, pf_hapmeth_assign_stats_t *astats,
                        pf_hapmeth_tagcheck_stats_t *tstats, pf_hapmeth_regions_stats_t *rstats,
                        pf_hapmeth_rank_stats_t *kstats) {
    return pf_hapmeth_run_rank_exact(o, dmr, hmm, perm, assign, tagcheck, regions, rank, NULL, stats, dstats, hstats, pstats,
                                     astats, tstats, rstats, kstats, NULL);
}

int pf_hapmeth_run_rank_exact(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                              const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                              const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                              const pf_hapmeth_rank_t *rank, const pf_hapmeth_rank_exact_t *exact, pf_hapmeth_stats_t *stats,
                              pf_hapmeth_dmr_stats_t *dstats, pf_hapmeth_hmm_stats_t *hstats, pf_hapmeth_perm_stats_t *pstats,
                              pf_hapmeth_assign_stats_t *astats, pf_hapmeth_tagcheck_stats_t *tstats,
                              pf_hapmeth_regions_stats_t *rstats, pf_hapmeth_rank_stats_t *kstats,
                              pf_hapmeth_rank_exact_stats_t *xstats) {
    return pf_hapmeth_run_tiles(o, dmr, hmm, perm, assign, tagcheck, regions, rank, exact, NULL, stats, dstats, hstats, pstats,
                                astats, tstats, rstats, kstats, xstats, NULL);
}

int pf_hapmeth_run_tiles(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                         const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                         const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                         const pf_hapmeth_rank_t *rank, const pf_hapmeth_rank_exact_t *exact, const pf_hapmeth_tiles_t *tiles,
                         pf_hapmeth_stats_t *stats, pf_hapmeth_dmr_stats_t *dstats, pf_hapmeth_hmm_stats_t *hstats,
                         pf_hapmeth_perm_stats_t *pstats, pf_hapmeth_assign_stats_t *astats,
                         pf_hapmeth_tagcheck_stats_t *tstats, pf_hapmeth_regions_stats_t *rstats,
                         pf_hapmeth_rank_stats_t *kstats, pf_hapmeth_rank_exact_stats_t *xstats,
                         pf_hapmeth_tiles_stats_t *lstats) {
    if (lstats) memset(lstats, 0, sizeof *lstats);
    if (xstats) memset(xstats, 0, sizeof *xstats);
    if (kstats) memset(kstats, 0, sizeof *kstats);
    if (rstats) memset(rstats, 0, sizeof *rstats);
    if (hstats) memset(hstats, 0, sizeof *hstats);
    if (tstats) memset(tstats, 0, sizeof *tstats);
    const pf_hapmeth_assign_t *rule = assign;
    if (tagcheck && (tagcheck->flags & PF_HAPMETH_TAGCHECK_RULE_ONLY)) assign = NULL;
    if (stats) memset(stats, 0, sizeof *stats);
    if (dstats) memset(dstats, 0, sizeof *dstats);
    if (pstats) memset(pstats, 0, sizeof *pstats);
    if (astats) memset(astats, 0, sizeof *astats);
    if (!o || !o->bam_path || !o->out_prefix || !o->out_prefix[0]) return PF_ERR_ARG;
    if (dmr && (dmr->cfg.min_delta_pct > 100u || !(dmr->max_p >= 0.0))) return PF_ERR_ARG;
    if (perm && (!dmr || perm->n_perm < 1u || perm->n_perm > PF_PERM_MAX_PERM)) return PF_ERR_ARG;
    if (assign && !dmr) return PF_ERR_ARG;
    if (tagcheck && !dmr) return PF_ERR_ARG;
    if (hmm && (!dmr || hmm->cfg.site_cost_q16 < 0 || hmm->cfg.site_cost_q16 > 64 * 65536 || hmm->cfg.switch_q16 < 0 ||
                hmm->cfg.switch_q16 > 64 * 65536))
        return PF_ERR_ARG;
    if (regions && (!dmr || hmm || !regions->bed_path)) return PF_ERR_ARG;
    if (rank && (!dmr || rank->min_calls < 1u || rank->min_calls > 65535u)) return PF_ERR_ARG;
    if (exact && (!rank || exact->max_reads < 2u || exact->max_reads > PF_RANK_EXACT_MAX_READS)) return PF_ERR_ARG;
    const uint32_t chunk = o->chunk_size ? o->chunk_size : 100000u;
    if (tiles && (tiles->min_calls < 1u || tiles->min_calls > 65535u)) return PF_ERR_ARG;
    if (tiles && (tiles->tile < 100u || tiles->tile > chunk || chunk % tiles->tile)) {
        fprintf(stderr, "[E::pf_hapmeth_main] --tile %u: a tile is 100 bases to the chunk size, and the chunk size (%u) must "
                "be a multiple of it, so that a tile lies in one fetch window\n", tiles->tile, chunk);
        return PF_ERR_ARG;
    }
    hm_t H;
    memset(&H, 0, sizeof H);
    H.tiles = tiles;
    H.rank = rank;
    H.exact = exact;
    H.regions = regions;
    H.o = o;
    H.dmr = dmr;
    H.perm = perm;
    H.assign = assign;
    H.tagcheck = tagcheck;
    H.rule = rule;
    H.hmm = hmm;
    H.lc = o->load;
    /* the batch's phasing parameters are not used by the pileup: the reference's defaults */
    H.cfg.k = 3; H.cfg.k_span = 5000; H.cfg.cov_for_selection = 6; H.cfg.n_cand = 15; H.cfg.hard_cov = 15;
    const uint32_t jw = o->job_windows ? o->job_windows : 1024u;
    H.jw = jw;
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
    int made = 0, dmade = 0, amade = 0, tmade = 0, trmade = 0;
    if (!rc && regions) {
        const int32_t nt = pf_bam_n_targets(H.bam);
        const char **names = (const char **)malloc(sizeof(char *) * (size_t)(nt > 0 ? nt : 1));
        if (!names) rc = PF_ERR_NOMEM;
        for (int32_t t = 0; t < nt && !rc; t++) names[t] = pf_bam_target_name(H.bam, t);
        if (!rc) {
            rc = pf_regions_load(regions->bed_path, (uint32_t)(nt > 0 ? nt : 0), names, &H.rlist);
            if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot read the regions of %s\n", regions->bed_path);
        }
        free(names);
        if (!rc) {
            H.rst.n_unknown_contig = pf_regions_unknown(H.rlist);
            for (int32_t t = 0; t < nt; t++) {               /* the contigs the run does not visit */
                const uint32_t *a, *b;
                const char *const *c;
                uint64_t n = 0;
                if ((t < tid0 || t >= tid1) && !pf_regions_contig(H.rlist, (uint32_t)t, &a, &b, &c, &n)) H.rst.n_outside += n;
            }
        }
    }
    if (!rc && dmr && dmr->blocks_path) {
        rc = pf_interval_gaps(dmr->blocks_path, PF_INTERVALS_GTF, 0, &H.blocks);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot read the phase blocks of %s\n", dmr->blocks_path);
    }
    if (!rc && tiles && tiles->blocks_path && !dmr) {
        rc = pf_interval_gaps(tiles->blocks_path, PF_INTERVALS_GTF, 0, &H.blocks);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot read the phase blocks of %s\n", tiles->blocks_path);
    }
    if (!rc) {
        rc = pf_ctx_create(o->device, &H.ctx);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] no usable GPU (device %d): %s\n", o->device, pf_strerror(rc));
    }
    if (!rc) {
        const size_t l = strlen(o->out_prefix) + 40;
        H.path = (char *)malloc(l);
        H.dpath = (char *)malloc(l);
        H.apath = (char *)malloc(l);
        H.tpath = (char *)malloc(l);
        H.trpath = (char *)malloc(l);
        H.rpath = (char *)malloc(l);
        H.kpath = (char *)malloc(l);
        H.lpath = (char *)malloc(l);
        ws = (uint32_t *)malloc(4ull * jw);
        we = (uint32_t *)malloc(4ull * jw);
        if (!H.path || !H.dpath || !H.apath || !H.tpath || !H.trpath || !H.rpath || !H.kpath || !H.lpath || !ws || !we)
            rc = PF_ERR_NOMEM;
        else {
            snprintf(H.path, l, "%s.hapmeth.bed", o->out_prefix);
            snprintf(H.dpath, l, "%s.hapmeth.dmr.bed", o->out_prefix);
            snprintf(H.apath, l, "%s.hapmeth.assign.tsv", o->out_prefix);
            snprintf(H.tpath, l, "%s.hapmeth.tagcheck.tsv", o->out_prefix);
            snprintf(H.trpath, l, "%s.hapmeth.tagcheck.regions.tsv", o->out_prefix);
            snprintf(H.rpath, l, "%s.hapmeth.regions.bed", o->out_prefix);
            snprintf(H.kpath, l, "%s.hapmeth.rank.tsv", o->out_prefix);
            snprintf(H.lpath, l, "%s.hapmeth.tiles.tsv", o->out_prefix);
        }
    }
    if (!rc) {
        rc = pf_write_hapmeth(H.path, NULL, NULL, 0, 0, 1);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.path);
        else made = 1;
    }
    if (!rc && dmr && !regions) {
        pf_perm_t none;                                  /* with --dmr-perm the header names its columns */
        memset(&none, 0, sizeof none);
        rc = write_dmr(H.dpath, NULL, NULL, perm ? &none : NULL, 1.0, 1, NULL, NULL);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.dpath);
        else dmade = 1;
    }
    if (!rc && assign) {
        rc = pf_write_assign(H.apath, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1, NULL);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.apath);
        else amade = 1;
    }
    if (!rc && tagcheck) {
        rc = pf_write_tagcheck(H.tpath, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1, NULL);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.tpath);
        else tmade = 1;
    }
    if (!rc && tagcheck) {
        rc = pf_write_tagcheck_regions(H.trpath, NULL, NULL, NULL, NULL, 1, NULL);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.trpath);
        else trmade = 1;
    }
    for (int32_t t = tid0; t < tid1 && !rc; t++) {
        if (!o->region) { s = 0; e = pf_bam_target_len(H.bam, t); }
        rc = hm_span(&H, t, s, e, chunk, jw, ws, we);
    }
    int rmade = 0;
    if (!rc && regions) {                              /* at the end: perm_q needs every region */
        uint64_t tested = 0;
        rmade = 1;
        rc = pf_write_regions(H.rpath, H.rec, H.nrec, perm != NULL, perm ? perm->n_perm : 0, &tested);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.rpath);
        H.rst.n_regions = H.nrec;
        if (perm) {
            H.rst.n_tested = H.pst.n_tested = tested;
            H.rst.n_untested = H.pst.n_untested = H.nrec - tested;
        }
    }
    int kmade = 0;
    if (!rc && rank) {                                 /* at the end: rank_q needs every region */
        uint64_t tested = 0;
        kmade = 1;
        if (exact) {
            uint64_t nx = 0;
            rc = pf_write_rank_exact(H.kpath, H.krec, H.xrec, H.nk, regions != NULL, &tested, &nx);
            H.xst.n_exact = nx;
        } else rc = pf_write_rank(H.kpath, H.krec, H.nk, regions != NULL, &tested);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.kpath);
        H.kst.n_tested = tested;
        H.kst.n_untested = H.nk - tested;
    }
    int lmade = 0;
    if (!rc && tiles) {                                /* at the end: rank_q needs every tile */
        uint64_t tested = 0;
        lmade = 1;
        rc = pf_write_rank_tiles(H.lpath, H.lrec, H.ltrec, H.nl, &tested);
        if (rc) fprintf(stderr, "[E::pf_hapmeth_main] cannot write %s\n", H.lpath);
        H.lst.n_written = H.nl;
        H.lst.n_tested = tested;
    }
    if (rc && lmade) (void)unlink(H.lpath);
    if (rc && kmade) (void)unlink(H.kpath);
    if (rc && rmade) (void)unlink(H.rpath);
    if (rc && made) (void)unlink(H.path);              /* no truncated output behind a failure */
    if (rc && dmade) (void)unlink(H.dpath);
    if (rc && amade) (void)unlink(H.apath);
    if (rc && tmade) (void)unlink(H.tpath);
    if (rc && trmade) (void)unlink(H.trpath);
    if (!rc && o->verbose)
        fprintf(stderr, "[M::pf_hapmeth_main] %llu windows (%llu without reads in the index, skipped), %llu records, "
                "%llu sites, pileup kernels %.3f ms\n", (unsigned long long)H.st.n_windows,
                (unsigned long long)H.st.n_skipped, (unsigned long long)H.st.n_records,
                (unsigned long long)H.st.n_sites, H.st.ms_kernels);
    if (!rc && o->verbose && regions)
        fprintf(stderr, "[M::pf_hapmeth_main] given regions: %llu written (%llu split by a phase block), %llu on contigs "
                "the BAM does not have, %llu outside the range, region kernels %.3f ms\n",
                (unsigned long long)H.rst.n_regions, (unsigned long long)H.rst.n_split,
                (unsigned long long)H.rst.n_unknown_contig, (unsigned long long)H.rst.n_outside, H.rst.ms_kernels);
    if (!rc && o->verbose && dmr && !regions)
        fprintf(stderr, "[M::pf_hapmeth_main] %llu informative sites, %llu regions, region kernels %.3f ms\n",
                (unsigned long long)H.dst.n_informative, (unsigned long long)H.dst.n_regions, H.dst.ms_kernels);
    if (!rc && o->verbose && hmm)
        fprintf(stderr, "[M::pf_hapmeth_main] hidden Markov model: %llu chains, %llu regions, model kernels %.3f ms\n",
                (unsigned long long)H.hst.n_chains, (unsigned long long)H.dst.n_regions, H.hst.ms_kernels);
    if (!rc && o->verbose && perm)
        fprintf(stderr, "[M::pf_hapmeth_main] %llu regions tested (%u permutations, seed %u), %llu without a test, "
                "%llu records fetched again, permutation kernels %.3f ms\n", (unsigned long long)H.pst.n_tested,
                perm->n_perm, perm->seed, (unsigned long long)H.pst.n_untested, (unsigned long long)H.pst.n_records,
                H.pst.ms_kernels);
    if (!rc && o->verbose && rank)
        fprintf(stderr, "[M::pf_hapmeth_main] rank test: %llu regions tested (at least %u calls a read), %llu without a test, "
                "%llu records fetched for it, rank kernels %.3f ms\n", (unsigned long long)H.kst.n_tested, rank->min_calls,
                (unsigned long long)H.kst.n_untested, (unsigned long long)H.kst.n_records, H.kst.ms_kernels);
    if (!rc && o->verbose && exact)
        fprintf(stderr, "[M::pf_hapmeth_main] exact rank test: %llu regions with an exact p-value (at most %u reads), %llu over "
                "the limit, exact kernels %.3f ms\n", (unsigned long long)H.xst.n_exact, exact->max_reads,
                (unsigned long long)H.xst.n_over, H.xst.ms_kernels);
    if (!rc && o->verbose && tiles)
        fprintf(stderr, "[M::pf_hapmeth_main] tiles of %u bases: %llu planned, %llu with a read written, %llu tested (at least "
                "%u calls a read), %llu split by a phase block, range kernels %.3f ms\n", tiles->tile,
                (unsigned long long)H.lst.n_tiles, (unsigned long long)H.lst.n_written, (unsigned long long)H.lst.n_tested,
                tiles->min_calls, (unsigned long long)H.lst.n_split, H.lst.ms_kernels);
    if (!rc && o->verbose && assign)
        fprintf(stderr, "[M::pf_hapmeth_main] %llu candidate reads scored, %llu assigned (%llu h1 / %llu h2), "
                "%llu records fetched for it, assign kernels %.3f ms\n", (unsigned long long)H.ast.n_lines,
                (unsigned long long)(H.ast.n_h1 + H.ast.n_h2), (unsigned long long)H.ast.n_h1,
                (unsigned long long)H.ast.n_h2, (unsigned long long)H.ast.n_records, H.ast.ms_kernels);
    if (!rc && o->verbose && tagcheck) {
        const uint64_t ok = H.tst.n_ok[0] + H.tst.n_ok[1], flip = H.tst.n_flip[0] + H.tst.n_flip[1];
        char conc[16] = "n/a";                         /* no decision at all: no figure, not a measured zero */
        if (ok + flip) snprintf(conc, sizeof conc, "%.4f", (double)ok / (double)(ok + flip));
        fprintf(stderr, "[M::pf_hapmeth_main] tag check: %llu tagged reads scored, %llu ok (%llu h1 / %llu h2), %llu flip "
                "(%llu h1 / %llu h2), %llu undecided, concordance %s, %llu records fetched for it, tag-check kernels %.3f ms\n",
                (unsigned long long)H.tst.n_lines, (unsigned long long)ok, (unsigned long long)H.tst.n_ok[0],
                (unsigned long long)H.tst.n_ok[1], (unsigned long long)flip, (unsigned long long)H.tst.n_flip[0],
                (unsigned long long)H.tst.n_flip[1], (unsigned long long)(H.tst.n_undecided[0] + H.tst.n_undecided[1]),
                conc, (unsigned long long)H.tst.n_records, H.tst.ms_kernels);
    }
    if (stats) *stats = H.st;
    if (dstats) *dstats = H.dst;
    if (pstats) *pstats = H.pst;
    if (astats) *astats = H.ast;
    if (tstats) *tstats = H.tst;
    if (hstats) *hstats = H.hst;
    if (rstats) *rstats = H.rst;
    if (kstats) *kstats = H.kst;
    if (xstats) *xstats = H.xst;
    if (lstats) *lstats = H.lst;
    free(ws);
    free(we);
    free(H.path);
    free(H.dpath);
    free(H.apath);
    free(H.tpath);
    free(H.trpath);
    free(H.brk);
    free(H.hpos);
    free(H.hcnt);
    free(H.rpath);
    free(H.kpath);
    free(H.krec);
    free(H.xrec);
    free(H.lpath);
    free(H.lrec);
    free(H.ltrec);
    free(H.rec);
    free(H.ks);
    free(H.ke);
    free(H.kmax);
    pf_region_list_free(H.rlist);
    pf_dmr_acc_free(H.acc);
    pf_gaps_free(H.blocks);
    if (H.ctx) pf_ctx_destroy(H.ctx);
    pf_bam_close(H.bam);
    return rc;
}
