/*
 * pomfret-amd -- command-line drop-in for `pomfret methphase` and `pomfret
 * report` (reference: main.c, cli.c parse_cli / sancheck_cliopt, and
 * blockjoin.c main_blockjoin 4643 / main_methreport 4901), running the
 * per-window hot path on the MI355X through libpomfret_amd.so.
 *
 *   pomfret-amd methphase -o out --vcf phased.vcf.gz [-c 60] [-u] [-t N] [--write-bam] [--gpus G] reads.bam
 *   pomfret-amd report    -o out --vcf phased.vcf.gz [-c C] [--chunk-size S --chunk-stride D] reads.bam
 *   pomfret-amd varhaptag -o out.bam in.vcf in.bam
 *   pomfret-amd hapmeth   -o out [-r chrom[:beg-end]] [--chunk-size N] [-q mapq] [-L minlen] [--host-fetch]
 *                         [--dmr [--dmr-min-cov N] [--dmr-delta PCT] [--dmr-gap N] [--dmr-min-sites N] [--dmr-max-p P]
 *                         [--dmr-blocks blocks.gtf] [--dmr-perm N [--dmr-seed S]]
 *                         [--dmr-hmm [--dmr-hmm-site-cost BITS] [--dmr-hmm-switch BITS]]
 *                         [--regions regions.bed  (instead of --dmr: the regions are given)]
 *                         [--dmr-rank [--dmr-rank-min-calls N] [--dmr-rank-exact [--dmr-rank-exact-max N]]]
 *                         [--assign] [--tag-check] [--assign-min-llr BITS] [--assign-min-calls N]]
 *                         [--tile T [--tile-min-calls N]  (with or without --dmr; --dmr-blocks applies)] tagged.bam
 *
 * Options and defaults follow the reference's cliopt_t (cli.c:47-75) and
 * cliopt_haptag_t (cli.c:332-343); the -c arithmetic (cov/10, cov/4), the
 * order-dependent -n override and varhaptag's --write-bam (which there turns
 * the BAM output OFF, cli.c:416) are kept.  Added: --gpus G (GPUs driven by
 * this process; default all visible), --host-fetch (records inflated and
 * decoded on the host instead of the device fetch), --job-windows W (windows per device
 * job), and --mask-bed FILE / --mask-variants (reference positions no
 * methylation site may lie on: a BED's intervals, the phased variants of
 * --vcf; methphase and report), and --ref FILE (a reference FASTA, plain or
 * gz'd: MD is synthesised on the device for the -u pre-pass and on the host
 * for the rescue, so the BAM needs no MD:Z tags; methphase, report and
 * varhaptag).  Phase blocks come from --tsv, else --gtf, else --vcf (main_blockjoin
 * 4661-4666); with -u the VCF still supplies the variants and the contigs to
 * pre-haplotag.  -U writes {prefix}.mp.input_haptag.tsv (4494-4517).  --dbg's
 * {prefix}.mp.dbg.read2tag (2223-2248) lists a khash in bucket order, which
 * no other implementation reproduces: it is not written (a warning says so).
 * Added subcommand: hapmeth writes {prefix}.hapmeth.bed, the methylation of
 * every CpG per haplotype of a haplotagged BAM (the HP tags of methphase
 * --write-bam, varhaptag or any other haplotagger) with the allele-specific
 * methylation p-value (pf_hapmeth_main; no reference counterpart).  hapmeth
 * --tile T is the genome-wide scan: {prefix}.hapmeth.tiles.tsv, every T-base
 * tile with a read under the read-level rank-sum test, with q-values over the
 * run (pf_hapmeth_run_tiles).
 */
#include <getopt.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>

#include "../../include/pomfret_amd.h"

static double now_s(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static void help_main(void) {
    fprintf(stderr, "Usage: pomfret-amd <subcommand> [options]\n");
    fprintf(stderr, "Subcommands:\n");
    fprintf(stderr, "  methphase  Given aligned reads with methylation calls in bam\n");
    fprintf(stderr, "             and exiting phase blocks, try to use methylation to\n");
    fprintf(stderr, "             phase the unphased regions (on the GPU).\n");
    fprintf(stderr, "  varhaptag  Haplotag reads from phased variants (on the GPU).\n");
    fprintf(stderr, "  hapmeth    Given haplotagged reads with methylation calls in bam, write\n");
    fprintf(stderr, "             the methylation of every CpG per haplotype and where the\n");
    fprintf(stderr, "             two haplotypes differ (on the GPU).\n");
    fprintf(stderr, "  report     Given aligned reads in bam and a phased vcf, sample\n");
    fprintf(stderr, "             intervals within phase blocks, pretend they are phase gaps\n");
    fprintf(stderr, "             and report whether meth-phasing would generate correct \n");
    fprintf(stderr, "             phase block joining decisions.\n");
}

static void help_methphase(const char *prefix) {
    fprintf(stderr, "Usage: pomfret-amd methphase -o out_prefix --vcf phased.vcf[.gz] [...] reads.bam 2>log\n");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "  bam    [pos] Aligned reads. Must be sorted and has index. If reads are not\n");
    fprintf(stderr, "               haplotagged, supply -u and provide vcf (via --vcf).\n");
    fprintf(stderr, "  -h,--help [   ] Display this message.\n");
    fprintf(stderr, "  -c     [opt] Read coverage (total, not per-haplotap). Will infer if not supplied.\n");
    fprintf(stderr, "  -o     [opt] Name prefix of output files. [%s]\n", prefix);
    fprintf(stderr, "  --vcf  [opt] Input, sorted vcf file containing phased variants. Plain or gz'd.\n");
    fprintf(stderr, "  --gtf  [opt] Phase blocks as a GTF (e.g. whatshap stats --block-list). Overrides --vcf's.\n");
    fprintf(stderr, "  --tsv  [opt] Phase blocks as a 3-column tsv (chrom, start, end). Overrides --gtf and --vcf.\n");
    fprintf(stderr, "  -U,--write-input-tagging [opt] With -u, write {prefix}.mp.input_haptag.tsv.\n");
    fprintf(stderr, "  -u,--bam-is-untagged [opt] If present, will haplotag reads \n"
                    "               with phased variants in vcf first (on the GPU).\n");
    fprintf(stderr, "  -t     [opt] Host threads fetching reads, per GPU. [1]\n");
    fprintf(stderr, "  --output-tsv [opt] Also write {prefix}.mp.tsv.\n");
    fprintf(stderr, "  --write-bam  [opt] Also write {prefix}.mp.bam (+ .bai) with the new HP tags.\n");
    fprintf(stderr, "  -T,--bam-threads [opt] Compression threads of the output BAM. [-t]\n");
    fprintf(stderr, "  --gpus [opt] GPUs to use. [all visible]\n");
    fprintf(stderr, "  --host-fetch [opt] Inflate and decode BAM records (and the coverage pass) on the host instead of the GPU.\n");
    fprintf(stderr, "  --mask-bed FILE [opt] BED (chrom, start, end; 0-based half-open; plain or gz'd) of reference\n"
                    "               positions that are never used as methylation sites (methphase, report).\n");
    fprintf(stderr, "  --mask-variants [opt] Also mask every phased variant of --vcf (its position and length):\n"
                    "               a CpG a heterozygous variant creates or destroys is no site.\n");
    fprintf(stderr, "  --ref FILE [opt] Reference FASTA (plain or gz'd).  With it the bam needs no MD tags: -u and the\n"
                    "               VCF writer's rescue compute MD from CIGAR, SEQ and the reference (also varhaptag).\n");
}

enum { O_LO = 301, O_HI, O_GTF = 304, O_VCF = 306, O_MAPQ, O_TSV, O_WBAM, O_OTSV, O_BAMT, O_UNTAG, O_WIT,
       O_CSIZE, O_CSTRIDE, O_HELP = 400, O_DBG, O_GPUS = 500, O_JOBW, O_HFETCH, O_MBED, O_MVAR, O_REF,
       O_DMR = 600, O_DMR_COV, O_DMR_DELTA, O_DMR_GAP, O_DMR_SITES, O_DMR_MAXP, O_DMR_BLOCKS, O_DMR_PERM, O_DMR_SEED,
       O_ASSIGN, O_ASSIGN_LLR, O_ASSIGN_CALLS, O_TAGCHECK, O_DMR_HMM, O_DMR_HMM_SITE, O_DMR_HMM_SWITCH, O_REGIONS,
       O_DMR_RANK, O_DMR_RANK_CALLS, O_DMR_RANK_EXACT, O_DMR_RANK_EXACT_MAX, O_TILE, O_TILE_CALLS };

static const struct option longopts[] = {
    {"lo", required_argument, 0, O_LO},          {"hi", required_argument, 0, O_HI},
    {"gtf", required_argument, 0, O_GTF},        {"vcf", required_argument, 0, O_VCF},
    {"mapq", required_argument, 0, O_MAPQ},      {"tsv", required_argument, 0, O_TSV},
    {"write-bam", no_argument, 0, O_WBAM},       {"output-tsv", no_argument, 0, O_OTSV},
    {"bam-threads", required_argument, 0, O_BAMT}, {"bam-is-untagged", no_argument, 0, O_UNTAG},
    {"write-input-tagging", no_argument, 0, O_WIT},
    {"chunk-size", required_argument, 0, O_CSIZE}, {"chunk-stride", required_argument, 0, O_CSTRIDE},
    {"help", no_argument, 0, O_HELP},            {"dbg", no_argument, 0, O_DBG},
    {"gpus", required_argument, 0, O_GPUS},      {"job-windows", required_argument, 0, O_JOBW},
    {"host-fetch", no_argument, 0, O_HFETCH},
    {"mask-bed", required_argument, 0, O_MBED},  {"mask-variants", no_argument, 0, O_MVAR},
    {"ref", required_argument, 0, O_REF},
    {"dmr", no_argument, 0, O_DMR},              {"dmr-min-cov", required_argument, 0, O_DMR_COV},
    {"dmr-delta", required_argument, 0, O_DMR_DELTA}, {"dmr-gap", required_argument, 0, O_DMR_GAP},
    {"dmr-min-sites", required_argument, 0, O_DMR_SITES}, {"dmr-max-p", required_argument, 0, O_DMR_MAXP},
    {"dmr-blocks", required_argument, 0, O_DMR_BLOCKS},
    {"dmr-perm", required_argument, 0, O_DMR_PERM}, {"dmr-seed", required_argument, 0, O_DMR_SEED},
    {"assign", no_argument, 0, O_ASSIGN},        {"assign-min-llr", required_argument, 0, O_ASSIGN_LLR},
    {"assign-min-calls", required_argument, 0, O_ASSIGN_CALLS}, {"tag-check", no_argument, 0, O_TAGCHECK},
    {"dmr-hmm", no_argument, 0, O_DMR_HMM},      {"dmr-hmm-site-cost", required_argument, 0, O_DMR_HMM_SITE},
    {"dmr-hmm-switch", required_argument, 0, O_DMR_HMM_SWITCH},
    {"regions", required_argument, 0, O_REGIONS},
    {"dmr-rank", no_argument, 0, O_DMR_RANK},    {"dmr-rank-min-calls", required_argument, 0, O_DMR_RANK_CALLS},
    {"dmr-rank-exact", no_argument, 0, O_DMR_RANK_EXACT},
    {"dmr-rank-exact-max", required_argument, 0, O_DMR_RANK_EXACT_MAX},
    {"tile", required_argument, 0, O_TILE},      {"tile-min-calls", required_argument, 0, O_TILE_CALLS},
    {0, 0, 0, 0}};

typedef struct {
    int help, threads, lo, hi, readlen, mapq, k, k_span, cov, cov_sel, n_cand, untagged, out_tsv, out_bam;
    int chunk_size, chunk_stride, gpus, job_windows, verbose, host_fetch, write_input_tagging, dbg, bam_threads;
    int mask_variants;
    char *prefix, *vcf, *gtf, *tsv, *bam, *mask_bed, *ref;
} cli_t;

static int parse(int argc, char **argv, cli_t *c) {
    memset(c, 0, sizeof *c);                          /* init_cliopt_t, cli.c:47-75 */
    c->threads = 1; c->lo = 100; c->hi = 156; c->readlen = 15000; c->mapq = 10; c->k = 3; c->k_span = 5000;
    c->cov_sel = -1; c->n_cand = 15; c->chunk_size = 50000; c->chunk_stride = 1000000;
    c->prefix = "pomfret";
    int o;
    optind = 1;
    while ((o = getopt_long(argc, argv, "vhuUo:k:L:l:c:n:t:T:", longopts, NULL)) >= 0) {
        switch (o) {
        case 'v': c->verbose++; break;
        case 'h': case O_HELP: c->help = 1; break;
        case 't': c->threads = atoi(optarg); break;
        case 'o': c->prefix = optarg; break;
        case 'k': c->k = atoi(optarg); break;
        case 'l': c->k_span = atoi(optarg); break;
        case 'L': c->readlen = atoi(optarg); break;
        case 'c': c->cov = atoi(optarg); c->cov_sel = c->cov / 10; c->n_cand = c->cov / 4; break;
        case 'n': c->n_cand = atoi(optarg); break;
        case O_LO: c->lo = atoi(optarg); break;
        case O_HI: c->hi = atoi(optarg); break;
        case O_GTF: c->gtf = optarg; break;
        case O_VCF: c->vcf = optarg; break;
        case O_MAPQ: c->mapq = atoi(optarg); break;
        case O_TSV: c->tsv = optarg; break;
        case O_WBAM: c->out_bam = 1; break;
        case O_OTSV: c->out_tsv = 1; break;
        case 'T': case O_BAMT: c->bam_threads = atoi(optarg); break;
        case 'u': case O_UNTAG: c->untagged = 1; break;
        case 'U': case O_WIT: c->write_input_tagging = 1; break;
        case O_CSIZE: c->chunk_size = atoi(optarg); break;
        case O_CSTRIDE: c->chunk_stride = atoi(optarg); break;
        case O_DBG: c->dbg = 1; break;
        case O_GPUS: c->gpus = atoi(optarg); break;
        case O_JOBW: c->job_windows = atoi(optarg); break;
        case O_HFETCH: c->host_fetch = 1; break;
        case O_MBED: c->mask_bed = optarg; break;
        case O_MVAR: c->mask_variants = 1; break;
        case O_REF: c->ref = optarg; break;
        default:
            fprintf(stderr, "[E::parse_cli] unknown or incomplete option \"%s\"\n", argv[optind - 1]);
            return 1;
        }
    }
    for (int i = optind; i < argc; i++) {
        if (c->bam) { fprintf(stderr, "[E::parse_cli] multiple bam input is not supported.\n"); return 1; }
        c->bam = argv[i];
    }
    return 0;
}

static int sancheck(cli_t *c) {                       /* sancheck_cliopt, cli.c:111-222 */
    if (c->threads <= 0) c->threads = 1;
    if (c->lo < 0 || c->lo > 127) { fprintf(stderr, "[E::sancheck_cliopt] bad --lo (%d)\n", c->lo); return 1; }
    if (c->hi > 255 || c->hi <= 127) { fprintf(stderr, "[E::sancheck_cliopt] bad --hi (%d)\n", c->hi); return 1; }
    if (c->readlen < 0) c->readlen = 0;
    if (c->mapq < 0) c->mapq = 0;
    if (c->k <= 0) c->k = 1;
    if (c->k_span <= 0) c->k_span = 1;
    if (c->n_cand <= 0) c->n_cand = 1;
    if (!c->gtf && !c->tsv && !c->vcf) {
        fprintf(stderr, "[E::sancheck_cliopt] gtf, tsv and vcf cannot all be absent\n");
        return 1;
    }
    if (c->untagged && !c->vcf) {
        fprintf(stderr, "[E::sancheck_cliopt] input bam was flagged unhaplotagged, but vcf is missing.\n");
        return 1;
    }
    if (c->mask_variants && !c->vcf) {
        fprintf(stderr, "[E::sancheck_cliopt] --mask-variants needs the phased variants of --vcf.\n");
        return 1;
    }
    if (c->mask_bed) {
        FILE *fp = fopen(c->mask_bed, "rb");
        if (!fp) { fprintf(stderr, "[E::sancheck_cliopt] cannot read --mask-bed %s\n", c->mask_bed); return 1; }
        fclose(fp);
    }
    if (c->ref) {
        FILE *fp = fopen(c->ref, "rb");
        if (!fp) { fprintf(stderr, "[E::sancheck_cliopt] cannot read --ref %s\n", c->ref); return 1; }
        fclose(fp);
    }
    if (!c->bam) { fprintf(stderr, "[E::sancheck_cliopt] missing bam file\n"); return 1; }
    size_t l = c->prefix ? strlen(c->prefix) : 0;
    while (l > 0 && c->prefix[l - 1] == '/') c->prefix[--l] = 0;
    if (l == 0) { fprintf(stderr, "[E::sancheck_cliopt] no output prefix given\n"); return 1; }
    if (c->chunk_size <= 0 || c->chunk_stride <= 0) {
        fprintf(stderr, "[E::sancheck_cliopt] invalid chunk size or stride\n");
        return 1;
    }
    if ((c->gtf ? 1 : 0) + (c->tsv ? 1 : 0) + (c->vcf ? 1 : 0) > 1)
        fprintf(stderr, "[M::sancheck_cliopt] multiple phase block files. Will not resolve conflict, only total "
                        "override (order is always: tsv > gtf > vcf)\n");
    if (c->dbg)
        fprintf(stderr, "[W::pomfret-amd] --dbg: {prefix}.mp.dbg.read2tag (a hash table dump in bucket order) is "
                        "not written\n");
    return 0;
}

/* varhaptag: parse_cli_varhaptag (cli.c:386-446): -o out.bam, -t, -v,
 * --write-bam (disables the BAM), positional in.vcf then in.bam */
static int varhaptag(int argc, char **argv) {
    const char *out = "pomfret_varhaptag", *vcf = NULL, *bam = NULL, *ref = NULL;
    int threads = 1, verbose = 0, write_bam = 1, gpus = 0, o;
    optind = 1;
    while ((o = getopt_long(argc, argv, "ho:t:r:v", longopts, NULL)) >= 0) {
        switch (o) {
        case 'h': case O_HELP:
            fprintf(stderr, "Usage: pomfret-amd varhaptag [-t threads] [--ref ref.fa] -o out.bam in.vcf in.bam 2>log\n");
            return 1;
        case 'o': out = optarg; break;
        case 't': threads = atoi(optarg); break;
        case 'v': verbose = 1; break;
        case 'r': break;
        case O_WBAM: write_bam = 0; break;
        case O_GPUS: gpus = atoi(optarg); break;
        case O_REF: ref = optarg; break;
        default:
            fprintf(stderr, "[E::parse_cli_varhaptag] unknown or incomplete option \"%s\"\n", argv[optind - 1]);
            return 1;
        }
    }
    for (int i = optind; i < argc; i++) {
        if (!vcf) vcf = argv[i];
        else if (!bam) bam = argv[i];
        else { fprintf(stderr, "[E::parse_cli_varhaptag] too many positional arguments\n"); return 1; }
    }
    if (!vcf || !bam) { fprintf(stderr, "[E::sancheck_cliopt_varhaptag] need a vcf and a bam\n"); return 1; }
    if (threads < 1) threads = 1;
    if (ref) {
        FILE *fp = fopen(ref, "rb");
        if (!fp) { fprintf(stderr, "[E::sancheck_cliopt_varhaptag] cannot read --ref %s\n", ref); return 1; }
        fclose(fp);
    }
    pf_methphase_opts_t op;
    memset(&op, 0, sizeof op);
    op.mode = PF_MODE_VARHAPTAG;
    op.bam_path = bam;
    op.vcf_path = vcf;
    op.out_prefix = out;
    op.write_bam = write_bam;
    op.threads = threads;
    op.n_devices = gpus;
    op.verbose = verbose;
    op.ref_path = ref;
    pf_mp_plan_t *p = NULL;
    const int rc = pf_methphase_main(&op, &p);
    if (rc) {
        fprintf(stderr, "[E::main] varhaptag failed: %s (%d)\n", pf_strerror(rc), rc);
        return 1;
    }
    pf_mp_free(p);
    return 0;
}

static void help_hapmeth(void) {
    fprintf(stderr, "Usage: pomfret-amd hapmeth -o out_prefix [...] tagged.bam 2>log\n");
    fprintf(stderr, "Writes {out_prefix}.hapmeth.bed: per CpG (0-based position of its C, strands combined) the meth and\n"
                    "unmeth calls of haplotype 1, haplotype 2 and the other reads, and the two-sided Fisher p-value of\n"
                    "haplotype 1 against haplotype 2 (allele-specific methylation).\n");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "  bam    [pos] Aligned, sorted, indexed reads with HP tags (methphase --write-bam, varhaptag, ...).\n");
    fprintf(stderr, "  -o     [opt] Name prefix of the output file. [pomfret]\n");
    fprintf(stderr, "  -r     [opt] Region chrom or chrom:beg-end (1-based, inclusive). [every contig]\n");
    fprintf(stderr, "  --chunk-size [opt] Bases per window, the fetch unit. [100000]\n");
    fprintf(stderr, "  -q,--mapq [opt] Minimum mapping quality. [10]\n");
    fprintf(stderr, "  -L     [opt] Minimum read length. [0]  Reads shorter than 2 bases and reads whose de tag fails\n"
                    "               the loader's divergence filter are dropped whatever -L says.\n");
    fprintf(stderr, "  --lo, --hi [opt] ML below lo is unmethylated, from hi methylated, between them no call. [100, 156]\n");
    fprintf(stderr, "  -t     [opt] Host threads of --host-fetch. [1]\n");
    fprintf(stderr, "  --host-fetch [opt] Inflate and decode BAM records on the host instead of the GPU.\n");
    fprintf(stderr, "  --gpus [opt] The GPU to use (the first of the list). [0]\n");
    fprintf(stderr, "  --job-windows [opt] Windows per device job. [1024]\n");
    fprintf(stderr, "  -v     [opt] Print the run's counts and the pileup kernels' time.\n");
    fprintf(stderr, "  --dmr  [opt] Also write {out_prefix}.hapmeth.dmr.bed: the regions where one haplotype is methylated\n"
                    "               and the other is not (runs of CpGs of one direction), with the pooled counts, the\n"
                    "               difference of the pooled methylation levels and pooled_p, the two-sided Fisher test\n"
                    "               of the pooled counts.  pooled_p is a ranking score, not a calibrated p-value: one\n"
                    "               read contributes to many CpGs, so the pooled counts are not independent.\n");
    fprintf(stderr, "  --dmr-min-cov [opt] Calls per haplotype a CpG needs to take part. [5]\n");
    fprintf(stderr, "  --dmr-delta [opt] Least difference of the two haplotypes' methylation at a CpG, in percent. [40]\n");
    fprintf(stderr, "  --dmr-gap [opt] Largest distance between neighbouring CpGs of one region, in bases. [500]\n");
    fprintf(stderr, "  --dmr-min-sites [opt] CpGs a region needs. [5]\n");
    fprintf(stderr, "  --dmr-max-p [opt] Drop regions whose pooled_p (a ranking score, see --dmr) is above this. [1]\n");
    fprintf(stderr, "  --dmr-blocks FILE [opt] Phase blocks as a GTF (methphase's {prefix}.mp.gtf): no region crosses a\n"
                    "               block's start or end, since HP tags are comparable only inside one block.\n");
    fprintf(stderr, "  --dmr-perm N [opt] Test every region with N permutations of its reads' haplotype labels and add\n"
                    "               the columns reads_h1, reads_h2 and perm_p = (hits + 1) / (N + 1): a p-value that\n"
                    "               holds although one read contributes to many CpGs (\".\" where a region has reads of\n"
                    "               one haplotype only, or more than 4096).  N in 1 .. 1000000. [0: off]\n");
    fprintf(stderr, "  --dmr-seed S [opt] Seed of the permutations. [1]\n");
    fprintf(stderr, "  --dmr-rank [opt] Needs --dmr or --regions.  Also write {out_prefix}.hapmeth.rank.tsv: every region of the\n"
                    "               second pass (those --dmr-perm tests) under a read-level Mann-Whitney rank-sum test.  Each\n"
                    "               read counts once, with its own methylation fraction inside the region: reads_h1, reads_h2,\n"
                    "               short_h1, short_h2 (reads below --dmr-rank-min-calls, left out), the fully methylated,\n"
                    "               fully unmethylated and mixed reads of each haplotype, auc = U / (reads_h1 * reads_h2) (the\n"
                    "               chance that a haplotype-1 read is more methylated than a haplotype-2 read; 1 or 0: an\n"
                    "               on/off switch), z, rank_p and, with --regions, rank_q (Benjamini-Hochberg over the run's\n"
                    "               tested regions; \".\" with --dmr, whose regions are selected on the data).  rank_p is the\n"
                    "               two-sided normal approximation with tie and continuity correction: it has no floor and\n"
                    "               needs no permutations, but it is asymptotic, so approximate below about eight reads per\n"
                    "               haplotype; --dmr-rank-exact adds the exact small-sample p-value.  rank_p underflows to 0\n"
                    "               near z > 38, which is why z has its own column.  \".\" in the four where a haplotype has no\n"
                    "               counted read, or a region more than 4096.\n");
    fprintf(stderr, "  --dmr-rank-min-calls N [opt] Needs --dmr-rank.  Calls inside the region a read needs to count, 1 .. 65535;\n"
                    "               a choice, not a measured optimum. [3]\n");
    fprintf(stderr, "  --dmr-rank-exact [opt] Needs --dmr-rank.  Three more columns in {out_prefix}.hapmeth.rank.tsv: exact_p, the\n"
                    "               exact two-sided p-value of the same test, counted over every way to deal the region's\n"
                    "               counted reads to the two haplotypes, ties included (all integers; for two separated groups\n"
                    "               of 10 reads it is 1.08e-5 where rank_p gives 1.83e-4); best_p, exact_p where there is one,\n"
                    "               else rank_p; best_q, Benjamini-Hochberg over best_p with --regions, \".\" with --dmr.\n"
                    "               exact_p is \".\" where a haplotype has no counted read or the region has more counted\n"
                    "               reads than --dmr-rank-exact-max.  The first 17 columns do not change.\n");
    fprintf(stderr, "  --dmr-rank-exact-max N [opt] Needs --dmr-rank-exact.  The most counted reads of a region that is counted\n"
                    "               exactly, 2 .. 64 (the counts of 68 reads pass 64 bits). [64]\n");
    fprintf(stderr, "  --tile T [opt] The genome-wide scan: also write {out_prefix}.hapmeth.tiles.tsv, every tile of T bases of\n"
                    "               each contig (or of -r's range, counted from its start) that holds a tagged read's call,\n"
                    "               under --dmr-rank's read-level rank-sum test, in the first pass: no region file and no\n"
                    "               second fetch.  The columns are --dmr-rank's 17, then h1_meth, h1_unmeth, h2_meth, h2_unmeth\n"
                    "               (the counted reads' calls), delta and block (split: a --dmr-blocks phase block ends inside;\n"
                    "               such a tile is counted, not tested).  rank_q is Benjamini-Hochberg over the run's tested\n"
                    "               tiles: the tiles are fixed in advance, so the correction holds.  T is 100 .. --chunk-size,\n"
                    "               and --chunk-size must be a multiple of T.  Needs no --dmr and goes with every other\n"
                    "               option; the records stay in memory until the end, about 120 bytes a tile with a read\n"
                    "               (a human genome at T = 1000: about 3 million).\n");
    fprintf(stderr, "  --tile-min-calls N [opt] Needs --tile.  Calls inside the tile a read needs to count, 1 .. 65535. [3]\n");
    fprintf(stderr, "  --dmr-hmm [opt] Needs --dmr.  Find the regions with a three-state hidden Markov model (none, h1>h2,\n"
                    "               h1<h2) over each contig's CpGs instead of the per-CpG threshold: every CpG adds its\n"
                    "               evidence for one direction (log2 likelihood ratio of two methylation levels against\n"
                    "               one), so a single noisy CpG does not cut a region in two.  --dmr-delta then applies to\n"
                    "               a region's pooled difference, not to each CpG; --dmr-min-cov, --dmr-gap, --dmr-min-sites,\n"
                    "               --dmr-blocks and the file's columns are as without it.\n");
    fprintf(stderr, "  --dmr-hmm-site-cost BITS [opt] Needs --dmr-hmm.  What every CpG of a region pays, a decimal in\n"
                    "               [0, 64]: the evidence a CpG must bring to extend a region; lower lets regions creep\n"
                    "               into flat stretches.  A choice made on simulated data, not measured on real samples. [2]\n");
    fprintf(stderr, "  --dmr-hmm-switch BITS [opt] Needs --dmr-hmm.  What opening and what closing a region pays, a decimal\n"
                    "               in [0, 64]: higher asks for more evidence per region and bridges longer weak stretches.\n"
                    "               A choice made on simulated data as well. [8]\n");
    fprintf(stderr, "  --regions FILE [opt] Instead of --dmr: the regions are given, not found.  FILE is a BED (chrom start end\n"
                    "               [name], 0-based half-open, plain or gzipped; regions may overlap, nest and repeat).  Writes\n"
                    "               {out_prefix}.hapmeth.regions.bed, one line per region whether the haplotypes differ in it\n"
                    "               or not: chrom, start, end, name, n_cpg, n_sites (CpGs with --dmr-min-cov calls on both\n"
                    "               haplotypes), n_h1gt and n_h2gt (of those, with a --dmr-delta difference either way), dir,\n"
                    "               the pooled counts, delta, pooled_p, llr_bits (the summed per-CpG evidence of two levels\n"
                    "               against one, signed) and block (split: a --dmr-blocks phase block ends inside; such a\n"
                    "               region is never tested).  Excludes --dmr, --dmr-hmm* and --dmr-gap and stands in for\n"
                    "               --dmr wherever another option needs it.  --dmr-perm, --assign and --tag-check run on the\n"
                    "               regions that are not split, have --dmr-min-sites CpGs, pass --dmr-max-p and are at most\n"
                    "               1,000,000 bases long; --dmr-perm adds reads_h1, reads_h2, perm_p and perm_q, the\n"
                    "               Benjamini-Hochberg q-value over the tested regions of the run.  With -r, regions not\n"
                    "               wholly inside the range are dropped.\n");
    fprintf(stderr, "  --assign [opt] Needs --dmr.  Also write {out_prefix}.hapmeth.assign.tsv: every untagged read with a call\n"
                    "               at a member CpG of a region (those that pass --dmr-max-p), scored against the region's\n"
                    "               tagged reads: qname, chrom, start, end (the region), n_calls (the read's calls used),\n"
                    "               llr (log2 odds of haplotype 1 against 2, Laplace-smoothed per CpG) and hp: 1, 2 or \".\"\n"
                    "               (not assigned).  One line per region and read; no BAM is rewritten.\n");
    fprintf(stderr, "  --assign-min-llr BITS [opt] Least |llr| for a tag, a decimal in (0, 64].  The default asks for\n"
                    "               odds of 8:1; it is a choice, not a measured optimum. [3]\n");
    fprintf(stderr, "  --assign-min-calls N [opt] Least n_calls for a tag, 1 .. 65535; a choice as well. [2]\n");
    fprintf(stderr, "  --tag-check [opt] Needs --dmr.  How far an --assign tag can be trusted on this sample: every tagged read\n"
                    "               of a region is scored as --assign would score it, against the region's tagged reads with\n"
                    "               its own calls taken out (leave-one-out), under --assign-min-llr / --assign-min-calls (given\n"
                    "               with --assign or --tag-check).  Writes {out_prefix}.hapmeth.tagcheck.tsv: qname, chrom,\n"
                    "               start, end, hp (the read's tag), n_calls, llr and verdict: ok (its own tag back), flip\n"
                    "               (the other one: a mis-tag or switch-error candidate) or \".\" (undecided); and\n"
                    "               {out_prefix}.hapmeth.tagcheck.regions.tsv: per region the reads, scored, ok and flip\n"
                    "               counts of each haplotype.  -v prints the concordance ok / (ok + flip).\n");
}

/* hapmeth: one device, the jobs one after another (pf_hapmeth_main) */
static int hapmeth(int argc, char **argv) {
    pf_hapmeth_opts_t op;
    memset(&op, 0, sizeof op);
    op.out_prefix = "pomfret";
    op.load.min_mapq = 10; op.load.min_len = 0; op.load.qual_lo = 100; op.load.qual_hi = 156;
    op.threads = 1;
    pf_hapmeth_dmr_t dm;
    memset(&dm, 0, sizeof dm);
    dm.cfg.min_cov = 5; dm.cfg.min_delta_pct = 40; dm.cfg.max_gap = 500; dm.cfg.min_sites = 5;
    dm.max_p = 1.0;
    pf_hapmeth_perm_t pm;
    pm.n_perm = 0; pm.seed = 1;
    pf_hapmeth_assign_t am;
    memset(&am, 0, sizeof am);
    int o, csize = 100000, jobw = 0, dmr = 0, dmr_opt = 0, assign = 0, assign_opt = 0, tagcheck = 0, hmm = 0, hmm_opt = 0;
    int gap_opt = 0, rank = 0, rank_opt = 0, exact = 0, exact_opt = 0;
    long xmax = 64;
    long rcalls = 3, tile = 0, tcalls = 3;
    int tile_opt = 0, blocks_opt = 0;
    pf_hapmeth_regions_t rg;
    rg.bed_path = NULL;
    double hsite = 2.0, hswitch = 8.0;
    long dcov = 5, ddelta = 40, dgap = 500, dsites = 5, dperm = 0, dseed = 1, acalls = 2;
    double allr = 3.0;
    char *end;
    if (argc == 1) { help_hapmeth(); return 1; }
    optind = 1;
    while ((o = getopt_long(argc, argv, "vho:r:q:L:t:", longopts, NULL)) >= 0) {
        switch (o) {
        case 'h': case O_HELP: help_hapmeth(); return 1;
        case 'v': op.verbose++; break;
        case 'o': op.out_prefix = optarg; break;
        case 'r': op.region = optarg; break;
        case 'q': case O_MAPQ: op.load.min_mapq = atoi(optarg); break;
        case 'L': op.load.min_len = atoi(optarg); break;
        case 't': op.threads = atoi(optarg); break;
        case O_LO: op.load.qual_lo = atoi(optarg); break;
        case O_HI: op.load.qual_hi = atoi(optarg); break;
        case O_CSIZE: csize = atoi(optarg); break;
        case O_GPUS: op.device = atoi(optarg); break;
        case O_JOBW: jobw = atoi(optarg); break;
        case O_HFETCH: op.host_fetch = 1; break;
        case O_DMR: dmr = 1; break;
        case O_DMR_COV: dmr_opt = 1; dcov = strtol(optarg, &end, 10); if (*end || !*optarg) dcov = -1; break;
        case O_DMR_DELTA: dmr_opt = 1; ddelta = strtol(optarg, &end, 10); if (*end || !*optarg) ddelta = -1; break;
        case O_DMR_GAP: dmr_opt = gap_opt = 1; dgap = strtol(optarg, &end, 10); if (*end || !*optarg) dgap = -1; break;
        case O_DMR_SITES: dmr_opt = 1; dsites = strtol(optarg, &end, 10); if (*end || !*optarg) dsites = -1; break;
        case O_DMR_MAXP: dmr_opt = 1; dm.max_p = strtod(optarg, &end); if (*end || !*optarg) dm.max_p = -1.0; break;
        case O_DMR_BLOCKS: blocks_opt = 1; dm.blocks_path = optarg; break;
        case O_TILE: tile = strtol(optarg, &end, 10); if (*end || !*optarg || tile < 1) tile = -1; break;
        case O_TILE_CALLS: tile_opt = 1; tcalls = strtol(optarg, &end, 10); if (*end || !*optarg) tcalls = -1; break;
        case O_DMR_PERM: dmr_opt = 1; dperm = strtol(optarg, &end, 10); if (*end || !*optarg) dperm = -1; break;
        case O_DMR_SEED: dmr_opt = 1; dseed = strtol(optarg, &end, 10); if (*end || !*optarg) dseed = -1; break;
        case O_ASSIGN: assign = 1; break;
        case O_TAGCHECK: tagcheck = 1; break;
        case O_DMR_HMM: hmm = 1; break;
        case O_REGIONS: rg.bed_path = optarg; break;
        case O_DMR_RANK: rank = 1; break;
        case O_DMR_RANK_EXACT: exact = 1; break;
        case O_DMR_RANK_EXACT_MAX: exact_opt = 1; xmax = strtol(optarg, &end, 10); if (*end || !*optarg) xmax = -1; break;
        case O_DMR_RANK_CALLS: rank_opt = 1; rcalls = strtol(optarg, &end, 10); if (*end || !*optarg) rcalls = -1; break;
        case O_DMR_HMM_SITE: hmm_opt = 1; hsite = strtod(optarg, &end); if (*end || !*optarg) hsite = -1.0; break;
        case O_DMR_HMM_SWITCH: hmm_opt = 1; hswitch = strtod(optarg, &end); if (*end || !*optarg) hswitch = -1.0; break;
        case O_ASSIGN_LLR: assign_opt = 1; allr = strtod(optarg, &end); if (*end || !*optarg) allr = -1.0; break;
        case O_ASSIGN_CALLS: assign_opt = 1; acalls = strtol(optarg, &end, 10); if (*end || !*optarg) acalls = -1; break;
        default:
            fprintf(stderr, "[E::parse_cli_hapmeth] unknown or incomplete option \"%s\"\n", argv[optind - 1]);
            return 1;
        }
    }
    for (int i = optind; i < argc; i++) {
        if (op.bam_path) { fprintf(stderr, "[E::parse_cli_hapmeth] multiple bam input is not supported.\n"); return 1; }
        op.bam_path = argv[i];
    }
    if (!op.bam_path) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] missing bam file\n"); return 1; }
    if (op.load.qual_lo < 0 || op.load.qual_lo > 127) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --lo (%d)\n", op.load.qual_lo); return 1; }
    if (op.load.qual_hi > 255 || op.load.qual_hi <= 127) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --hi (%d)\n", op.load.qual_hi); return 1; }
    if (csize <= 0) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] invalid chunk size\n"); return 1; }
    if (!op.out_prefix[0]) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] no output prefix given\n"); return 1; }
    if (rg.bed_path && (dmr || hmm || hmm_opt || gap_opt)) {
        fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --regions gives the regions: it excludes --dmr, --dmr-hmm* and --dmr-gap\n");
        return 1;
    }
    const int have = dmr || rg.bed_path != NULL;       /* a source of regions */
    if (blocks_opt && !tile) dmr_opt = 1;              /* --dmr-blocks also goes with --tile alone */
    if (dmr_opt && !have) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-* options need --dmr or --regions\n"); return 1; }
    if (tile_opt && !tile) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --tile-min-calls needs --tile\n"); return 1; }
    if (tile && (tile < 100 || tile > csize || csize % tile)) {
        fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --tile: 100 .. --chunk-size (%d), and --chunk-size must be a multiple "
                "of it\n", csize);
        return 1;
    }
    if (tcalls < 1 || tcalls > 65535) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --tile-min-calls (1 .. 65535)\n"); return 1; }
    if (dcov < 1 || dcov > 65535) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-min-cov (1 .. 65535)\n"); return 1; }
    if (ddelta < 1 || ddelta > 100) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-delta (1 .. 100)\n"); return 1; }
    if (dgap < 1 || dgap > 0x7FFFFFFFl) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-gap\n"); return 1; }
    if (dsites < 1 || dsites > 0x7FFFFFFFl) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-min-sites\n"); return 1; }
    if (!(dm.max_p >= 0.0 && dm.max_p <= 1.0)) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-max-p (0 .. 1)\n"); return 1; }
    if (dperm < 0 || dperm > 1000000) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-perm (0 .. 1000000)\n"); return 1; }
    if (dseed < 0 || dseed > 0xFFFFFFFFl) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-seed (0 .. 4294967295)\n"); return 1; }
    if (assign_opt && !assign && !tagcheck) {
        fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --assign-* options need --assign or --tag-check\n");
        return 1;
    }
    if (assign && !have) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --assign needs --dmr or --regions\n"); return 1; }
    if (tagcheck && !have) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --tag-check needs --dmr or --regions\n"); return 1; }
    if (rank && !have) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-rank needs --dmr or --regions\n"); return 1; }
    if (rank_opt && !rank) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-rank-min-calls needs --dmr-rank\n"); return 1; }
    if (exact && !rank) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-rank-exact needs --dmr-rank\n"); return 1; }
    if (exact_opt && !exact) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-rank-exact-max needs --dmr-rank-exact\n"); return 1; }
    if (xmax < 2 || xmax > 64) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-rank-exact-max (2 .. 64)\n"); return 1; }
    if (rcalls < 1 || rcalls > 65535) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-rank-min-calls (1 .. 65535)\n"); return 1; }
    if (hmm_opt && !hmm) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-hmm-* options need --dmr-hmm\n"); return 1; }
    if (hmm && !dmr) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] --dmr-hmm needs --dmr\n"); return 1; }
    if (!(hsite >= 0.0 && hsite <= 64.0)) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-hmm-site-cost (0 .. 64)\n"); return 1; }
    if (!(hswitch >= 0.0 && hswitch <= 64.0)) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --dmr-hmm-switch (0 .. 64)\n"); return 1; }
    if (!(allr > 0.0 && allr <= 64.0)) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --assign-min-llr (above 0, at most 64)\n"); return 1; }
    if (acalls < 1 || acalls > 65535) { fprintf(stderr, "[E::sancheck_cliopt_hapmeth] bad --assign-min-calls (1 .. 65535)\n"); return 1; }
    am.min_llr_q16 = (int64_t)llround(allr * 65536.0); am.min_calls = (uint32_t)acalls;
    pm.n_perm = (uint32_t)dperm; pm.seed = (uint32_t)dseed;
    dm.cfg.min_cov = (uint32_t)dcov; dm.cfg.min_delta_pct = (uint32_t)ddelta;
    dm.cfg.max_gap = (uint32_t)dgap; dm.cfg.min_sites = (uint32_t)dsites;
    if (op.load.min_mapq < 0) op.load.min_mapq = 0;
    if (op.load.min_len < 0) op.load.min_len = 0;
    if (op.threads < 1) op.threads = 1;
    if (op.device < 0) op.device = 0;
    op.chunk_size = (uint32_t)csize;
    op.job_windows = jobw > 0 ? (uint32_t)jobw : 0;
    pf_hapmeth_stats_t st;
    pf_hapmeth_dmr_stats_t dst;
    pf_hapmeth_perm_stats_t pst;
    pf_hapmeth_assign_stats_t ast;
    pf_hapmeth_tagcheck_t tm;
    memset(&tm, 0, sizeof tm);
    if (!assign) tm.flags = PF_HAPMETH_TAGCHECK_RULE_ONLY;
    pf_hapmeth_tagcheck_stats_t tst;
    /* --tag-check checks the rule the two --assign-* options set, with --assign or without */
    pf_hapmeth_hmm_t hm;
    hm.cfg.site_cost_q16 = (int32_t)llround(hsite * 65536.0); hm.cfg.switch_q16 = (int32_t)llround(hswitch * 65536.0);
    pf_hapmeth_hmm_stats_t hst;
    pf_hapmeth_regions_stats_t rst;
    pf_hapmeth_rank_t km;
    km.min_calls = (uint32_t)rcalls;
    pf_hapmeth_rank_stats_t kst;
    pf_hapmeth_rank_exact_t xm;
    xm.max_reads = (uint32_t)xmax;
    pf_hapmeth_rank_exact_stats_t xst;
    pf_hapmeth_tiles_t lm;
    lm.tile = (uint32_t)tile; lm.min_calls = (uint32_t)tcalls; lm.blocks_path = dm.blocks_path;
    pf_hapmeth_tiles_stats_t lst;
    const int rc = pf_hapmeth_run_tiles(&op, have ? &dm : NULL, hmm ? &hm : NULL, pm.n_perm ? &pm : NULL,
                                        assign || tagcheck ? &am : NULL, tagcheck ? &tm : NULL, rg.bed_path ? &rg : NULL,
                                        rank ? &km : NULL, exact ? &xm : NULL, tile ? &lm : NULL, &st, &dst, &hst, &pst, &ast,
                                        &tst, &rst, &kst, &xst, &lst);
    if (rc) {
        fprintf(stderr, "[E::main] hapmeth failed: %s (%d)\n", pf_strerror(rc), rc);
        return 1;
    }
    fprintf(stderr, "[M::main] %llu sites written to %s.hapmeth.bed\n", (unsigned long long)st.n_sites, op.out_prefix);
    if (dmr)
        fprintf(stderr, "[M::main] %llu regions written to %s.hapmeth.dmr.bed\n", (unsigned long long)dst.n_regions,
                op.out_prefix);
    if (rg.bed_path)
        fprintf(stderr, "[M::main] %llu regions written to %s.hapmeth.regions.bed\n", (unsigned long long)rst.n_regions,
                op.out_prefix);
    if (pm.n_perm)
        fprintf(stderr, "[M::main] %llu of them with a permutation p-value\n", (unsigned long long)pst.n_tested);
    if (rank)
        fprintf(stderr, "[M::main] %llu regions written to %s.hapmeth.rank.tsv, %llu of them with a rank-sum p-value\n",
                (unsigned long long)(kst.n_tested + kst.n_untested), op.out_prefix, (unsigned long long)kst.n_tested);
    if (exact)
        fprintf(stderr, "[M::main] %llu of them with an exact p-value, %llu with more than %u counted reads\n",
                (unsigned long long)xst.n_exact, (unsigned long long)xst.n_over, xm.max_reads);
    if (tile)
        fprintf(stderr, "[M::main] %llu tiles written to %s.hapmeth.tiles.tsv, %llu of them with a rank-sum p-value\n",
                (unsigned long long)lst.n_written, op.out_prefix, (unsigned long long)lst.n_tested);
    if (assign)
        fprintf(stderr, "[M::main] %llu scored reads written to %s.hapmeth.assign.tsv, %llu of them with a tag\n",
                (unsigned long long)ast.n_lines, op.out_prefix, (unsigned long long)(ast.n_h1 + ast.n_h2));
    if (tagcheck)
        fprintf(stderr, "[M::main] %llu tagged reads checked in %s.hapmeth.tagcheck.tsv, %llu regions in "
                "%s.hapmeth.tagcheck.regions.tsv\n", (unsigned long long)tst.n_lines, op.out_prefix,
                (unsigned long long)tst.n_regions, op.out_prefix);
    return 0;
}

int main(int argc, char **argv) {
    fprintf(stderr, "[M::main] pomfret-amd (MI355X) ABI %d\n[M::main] CMD: ", pf_abi_version());
    for (int i = 0; i < argc; i++) fprintf(stderr, "%s ", argv[i]);
    fprintf(stderr, "\n");
    const double T = now_s();
    if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help") || !strcmp(argv[1], "help")) {
        help_main();
        return 1;
    }
    if (!strcmp(argv[1], "varhaptag")) return varhaptag(argc - 1, argv + 1);
    if (!strcmp(argv[1], "hapmeth")) return hapmeth(argc - 1, argv + 1);
    const int report = !strcmp(argv[1], "report");
    if (!report && strcmp(argv[1], "methphase")) {
        fprintf(stderr, "[E::main] unknown subcommand: %s\n", argv[1]);
        return 1;
    }
    cli_t c;
    if (argc == 2) { help_methphase("pomfret"); return 1; }
    if (parse(argc - 1, argv + 1, &c)) return 1;
    if (c.help) { help_methphase(c.prefix); return 1; }
    if (sancheck(&c)) return 1;
    if (report && !c.vcf) { fprintf(stderr, "[E::main] missing input: phasd vcf file.\n"); return 1; }

    pf_methphase_opts_t o;
    memset(&o, 0, sizeof o);
    o.mode = report ? PF_MODE_REPORT : PF_MODE_METHPHASE;
    o.bam_path = c.bam;
    o.vcf_path = c.vcf;
    o.out_prefix = c.prefix;
    o.cov_for_selection = c.cov_sel;
    o.n_cand = c.n_cand;
    o.cov = c.cov;
    o.k = c.k;
    o.k_span = c.k_span;
    o.load.min_mapq = c.mapq;
    o.load.min_len = c.readlen;
    o.load.qual_lo = c.lo;
    o.load.qual_hi = c.hi;
    o.untagged = c.untagged;
    o.write_tsv = c.out_tsv;
    o.write_bam = c.out_bam;
    o.chunk_size = c.chunk_size;
    o.chunk_stride = c.chunk_stride;
    o.threads = c.threads;
    o.bam_threads = c.bam_threads;                  /* -T; else -t (cli.c:261-264) */
    o.n_devices = c.gpus;
    o.job_windows = c.job_windows > 0 ? (uint32_t)c.job_windows : 0;
    o.host_fetch = c.host_fetch;
    o.verbose = c.verbose;
    if (!report && (c.tsv || c.gtf)) {         /* tsv > gtf > vcf (4661-4666) */
        o.interval_path = c.tsv ? c.tsv : c.gtf;
        o.interval_format = c.tsv ? PF_INTERVALS_TSV : PF_INTERVALS_GTF;
    }
    o.write_input_tagging = c.write_input_tagging;
    o.mask_path = c.mask_bed;
    o.mask_variants = c.mask_variants;
    o.ref_path = c.ref;
    pf_mp_plan_t *p = NULL;
    const int rc = pf_methphase_main(&o, &p);
    if (rc) {
        fprintf(stderr, "[E::main] %s failed: %s (%d)\n", argv[1], pf_strerror(rc), rc);
        return 1;
    }
    const int8_t *dec;
    uint32_t n, n_limit;
    pf_mp_decisions(p, &dec, &n, &n_limit);
    uint32_t joined = 0;
    for (uint32_t i = 0; i < n; i++) joined += dec[i] >= 0;
    fprintf(stderr, "[M::main] %u of %u windows joined; %u read tags; done, used %.1fs\n", joined, n,
            (unsigned)pf_tags_size(pf_mp_qname_hp(p)), now_s() - T);
    if (c.verbose) {
        pf_mp_stats_t st;
        if (pf_mp_stats(p, &st) == PF_OK)
            fprintf(stderr, "[M::main] phases: plan %.3fs (coverage pass %.3fs), -u pre-pass %.3fs, windows %.3fs, "
                    "writers %.3fs; device inflate %.1f ms (-u) + %.1f ms (windows)\n", st.s_plan, st.s_estimate,
                    st.s_haptag, st.s_windows, st.s_finish, st.fetch_ms[1][1], st.fetch_ms[0][1]);
    }
    pf_mp_free(p);
    return 0;
}
