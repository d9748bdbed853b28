/*
 * pomfret_amd.h -- C ABI of the MI355X (gfx950) implementation of Pomfret's
 * per-window methylation-phasing hot path.
 *
 * Plain C, plain pointers and sizes; no HIP or torch types cross this
 * boundary.  The library (libpomfret_amd.so) owns its device buffers; callers
 * own every host buffer they pass in.  No entry point calls exit(): errors are
 * returned as negative PF_ERR_* codes ("no evidence" is decision = -1, not an
 * error), matching the reference's split between fatal exits and -1 decisions
 * (reference blockjoin.c:1059, 1150, 4266-4270, 4313-4320).
 *
 * Reference interfaces replaced (all line numbers: /root/reference/<file>):
 *
 *   pf_methphase_windows / pf_methphase_run
 *       replaces the per-window call haplotag_region_given_bam()
 *       (blockjoin.c:4217-4335) as driven by the kt_for worker
 *       blockjoin_one_chrom_callback() (blockjoin.c:4350-4426, dispatched at
 *       blockjoin.c:4560) and by the serial report loop (blockjoin.c:5054-5077).
 *       One call processes a whole batch of windows (gaps) from any number of
 *       contigs; decisions land in caller-owned arrays exactly where the
 *       reference writes ranges->decisions.a[i] (blockjoin.c:4406), and the
 *       per-read tags the worker stores for joined windows (blockjoin.c:4408-4423)
 *       are returned per read.
 *
 *   pf_haptag_reads
 *       replaces parse_variants_for_one_read() + haptag_one_read_with_variants()
 *       (blockjoin.c:1545-1840) as driven by pre_haplotagging_read_in_one_ref()
 *       (blockjoin.c:1841-1898), the --bam-is-untagged (-u) pre-pass.
 *
 *   pf_fisher_exact
 *       the two-sided Fisher exact test the reference borrows from htslib
 *       (kt_fisher_exact, called at blockjoin.c:3926).
 *
 * Input layout ("SoA"): what the reference's BAM window loader
 * (load_reads_given_interval, blockjoin.c:1043-1173) keeps per read after its
 * filters, flattened:
 *   - windows in any order; each window owns a contiguous run of reads;
 *   - reads of a window in BAM order (the order sam_itr_next returns them);
 *   - each read owns a contiguous run of 5mC calls in the order
 *     get_mod_poss_on_ref() produces them (blockjoin.c:605-792).
 */
#ifndef POMFRET_AMD_H
#define POMFRET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 1

/* error codes */
#define PF_OK               0
#define PF_ERR_ARG         -1   /* bad argument / inconsistent batch */
#define PF_ERR_HIP         -2   /* HIP runtime error (no device, launch failure) */
#define PF_ERR_NOMEM       -3   /* device or host allocation failed */
#define PF_ERR_UNSUPPORTED -4   /* configuration outside what this build implements */
#define PF_ERR_LIMIT       -5   /* input exceeds a documented hard limit */
#define PF_ERR_INTERNAL    -6

/* Methmer / tagging configuration.  Mirrors mmr_config_t (blockjoin.h:7-16)
 * plus the per-contig n_candidates_per_iter (blockjoin.c:4357-4390). */
typedef struct pf_cfg {
    int32_t k;                  /* methmer length, cli -k (default 3, cli.c:67)            */
    int32_t k_span;             /* methmer base-span limit, cli -l (default 5000)          */
    int32_t cov_for_selection;  /* site min meth AND unmeth calls (blockjoin.c:3270-3271)  */
    int32_t cov_for_runtime;    /* min hap0+hap1 methmer count to use a site (3669-3691)   */
    int32_t n_cand;             /* candidates scored per greedy iteration (4039-4045)      */
    int32_t hard_cov;           /* left-side per-haplotype read minimum, 15 (1161)         */
    int32_t flags;              /* PF_FLAG_*                                               */
    int32_t reserved;
} pf_cfg_t;

#define PF_FLAG_NONE 0

/* One batch of windows.  A "window" is one call of haplotag_region_given_bam:
 * the gap [win_start, win_end] (blockjoin.c:4397-4398) and the reads that
 * load_reads_given_interval fetched for [s-READBACK, e+READBACK] and kept. */
typedef struct pf_window_batch {
    uint32_t n_windows;
    uint32_t n_reads;
    uint64_t n_calls;
    const uint32_t *win_start;     /* [n_windows] gap start s (ranges->starts.a[i])         */
    const uint32_t *win_end;       /* [n_windows] gap end e   (ranges->ends.a[i])           */
    const uint32_t *win_read_off;  /* [n_windows+1] reads of window w: [off[w], off[w+1])   */
    const int32_t  *win_cov_sel;   /* [n_windows] or NULL -> cfg.cov_for_selection          */
    const int32_t  *win_cov_rt;    /* [n_windows] or NULL -> cfg.cov_for_runtime            */
    const int32_t  *win_n_cand;    /* [n_windows] or NULL -> cfg.n_cand                     */
    const uint32_t *read_start;    /* [n_reads] core.pos, 0-based (blockjoin.c:1124)        */
    const uint32_t *read_end;      /* [n_reads] bam_endpos, exclusive (blockjoin.c:1125)    */
    const uint8_t  *read_hp;       /* [n_reads] HP-1, 254 if untagged (910-923, 1114-1122)  */
    const uint64_t *read_call_off; /* [n_reads+1] calls of read r: [off[r], off[r+1])      */
    const uint32_t *call_pos;      /* [n_calls] reference position of the CpG's C           */
    const uint8_t  *call_cat;      /* [n_calls] 0 meth (q>=hi), 1 unmeth (q<lo), 2 nocall   */
} pf_window_batch_t;

/* Per-window results.  Every pointer except decision may be NULL. */
typedef struct pf_window_out {
    int8_t   *decision;      /* [n_windows] 0 cis, 1 trans, -1 no join (4313-4320)       */
    uint8_t  *read_hp;       /* [n_reads] rs->a[j].hp when the window returns; these are
                                the tags the worker stores when decision>=0 (4408-4423)   */
    int32_t  *dir_table;     /* [n_windows*2*4] 2x2 table buf[raw][new] per direction:
                                index (w*2+dir)*4 + raw*2 + new; dir 0 = forward
                                (left->right, scored on right strict reads), dir 1 =
                                backward (scored on left strict reads) (3881-3893)       */
    int32_t  *dir_join;      /* [n_windows*2] haplotag_region2 return: 0,1,-1 (4088)     */
    int32_t  *dir_which_way; /* [n_windows*2] evaluate_separation1 join_dir (-9 on fail) */
    double   *dir_fisher_p;  /* [n_windows*2] two-sided p (1.0 when not reached)          */
    float    *dir_score;     /* [n_windows*2] evaluate_separation1 return value           */
    uint32_t *win_n_sites;   /* [n_windows] methmer sites (ms->n); 0 => window skipped     */
    uint32_t *win_n_reads;   /* [n_windows] rs->n after the left-coverage check (1161)    */
} pf_window_out_t;

/* ------------------------------------------------------------------ */
/* Record-level input: the BAM records each window's region query returned,
 * decoded on the host (BGZF inflate and record split; htslib's part in the
 * reference) and kept as raw fields.  The read filters and the 5mC
 * extraction of load_reads_given_interval / fill_read_meth_record_from_bam_line
 * / get_mod_poss_on_ref (blockjoin.c:1043-1173, 794-908, 605-792) run on the
 * device (kernel K0), so the window batch above never exists on the host. */

/* Loader parameters: mmr_config_t's lo/hi/readlen_threshold/min_mapq
 * (blockjoin.h:7-16; cli defaults lo 100, hi 156, -L 15000, -q 10). */
typedef struct pf_load_cfg {
    int32_t min_mapq;     /* reads with core.qual < min_mapq are dropped (1082)        */
    int32_t min_len;      /* reads with l_qseq < min_len (or < 2) are dropped (1083)   */
    int32_t qual_lo;      /* ML < lo -> unmeth (1); passed as uint8_t (799, 876-878)   */
    int32_t qual_hi;      /* ML >= hi -> meth (0); otherwise no-call (2)               */
} pf_load_cfg_t;

typedef struct pf_aln_batch {
    uint32_t n_windows;
    uint32_t n_recs;
    const uint32_t *win_start;     /* [n_windows] gap start s                             */
    const uint32_t *win_end;       /* [n_windows] gap end e                               */
    const uint32_t *win_rec_off;   /* [n_windows+1] records of window w in BAM order      */
    const int32_t  *win_cov_sel;   /* [n_windows] or NULL -> cfg.cov_for_selection        */
    const int32_t  *win_cov_rt;    /* [n_windows] or NULL -> cfg.cov_for_runtime          */
    const int32_t  *win_n_cand;    /* [n_windows] or NULL -> cfg.n_cand                   */
    const uint16_t *flag;          /* [n_recs] core.flag                                  */
    const uint8_t  *mapq;          /* [n_recs] core.qual                                  */
    const uint32_t *pos;           /* [n_recs] core.pos (0-based)                         */
    const uint32_t *l_qseq;        /* [n_recs] core.l_qseq                                */
    const float    *de;            /* [n_recs] de:f value, -1 when absent (1079-1080)      */
    const uint8_t  *hp;            /* [n_recs] get_hp_from_aln (910-923) or the -u table  */
    const uint64_t *cigar_off;     /* [n_recs+1] into cigar                               */
    const uint32_t *cigar;         /* BAM encoding len<<4|op                              */
    const uint64_t *seq_off;       /* [n_recs+1] byte offsets into seq                    */
    const uint8_t  *seq;           /* BAM 4-bit packed SEQ                                */
    const uint64_t *mm_off;        /* [n_recs+1] MM:Z (or Mm:Z) text, no terminator       */
    const char     *mm;
    const uint64_t *ml_off;        /* [n_recs+1] ML:B:C values; empty = tag absent        */
    const uint8_t  *ml;
} pf_aln_batch_t;

/* ------------------------------------------------------------------ */
/* -u pre-pass: known phased variants of one contig and reads to tag.  */

/* variant ops as in blockjoin.c:28-31 */
#define PF_VAR_M 0
#define PF_VAR_X 1
#define PF_VAR_I 2
#define PF_VAR_D 3

typedef struct pf_known_vars {
    uint32_t n;
    const uint32_t *pos;       /* [n] 0-based, as insert_variant_from_vcf_line stores it (1432-1543) */
    const uint32_t *len;       /* [n] op length                                               */
    const uint8_t  *op;        /* [n] PF_VAR_X / PF_VAR_I / PF_VAR_D                          */
    const uint8_t  *haptag;    /* [n] haplotype carrying REF (GT[0])                          */
    const uint64_t *char_off;  /* [n+1] allele chars (seq_nt4 codes 0..4) of variant i        */
    const uint8_t  *chars;
} pf_known_vars_t;

/* Reads of ONE contig in BAM order, primary mapped only (flag filter of
 * blockjoin.c:1869-1870 already applied by the caller). */
typedef struct pf_read_aln_batch {
    uint32_t n_reads;
    const uint32_t *start;      /* [n] core.pos                                  */
    const uint32_t *end;        /* [n] bam_endpos                                */
    const uint64_t *cigar_off;  /* [n+1] into cigar                              */
    const uint32_t *cigar;      /* BAM encoding: len<<4 | op                     */
    const uint64_t *seq_off;    /* [n+1] byte offsets into seq (4-bit packed)    */
    const uint32_t *seq_len;    /* [n] l_qseq                                    */
    const uint8_t  *seq;        /* BAM 4-bit packed SEQ                          */
    const uint64_t *md_off;     /* [n+1] into md (no terminator needed)          */
    const char     *md;         /* MD:Z strings, concatenated                    */
} pf_read_aln_batch_t;

/* ------------------------------------------------------------------ */

typedef struct pf_ctx pf_ctx_t;        /* one device, one HIP stream          */
typedef struct pf_dbatch pf_dbatch_t;  /* a window batch resident in HBM      */

int  pf_abi_version(void);
int  pf_device_count(void);
const char *pf_strerror(int code);

/* Context bound to one device (one process per GPU). */
int  pf_ctx_create(int device, pf_ctx_t **out);
void pf_ctx_destroy(pf_ctx_t *ctx);

/* Upload a batch to HBM.  Validates it (offsets monotone, sizes, limits) and
 * keeps a device copy plus the few host-side arrays the decision epilogue
 * needs.  The caller's host arrays may be freed afterwards. */
int  pf_batch_upload(pf_ctx_t *ctx, const pf_cfg_t *cfg,
                     const pf_window_batch_t *batch, pf_dbatch_t **out);
void pf_batch_free(pf_dbatch_t *db);
uint32_t pf_batch_n_windows(const pf_dbatch_t *db);
/* Reads of the batch (record level: the kept records of the last finished
 * run -- K0 sizes the batch on the device -- bounded by the record count). */
uint32_t pf_batch_n_reads(const pf_dbatch_t *db);
/* Calls of the batch (record level: of the last finished run, 0 before). */
uint64_t pf_batch_n_calls(const pf_dbatch_t *db);

/* Run the hot path on a resident batch: all kernels, then the 2x2 tables and
 * tags come back to the host, where the Fisher test and the join decision
 * are applied.  Synchronous. */
int  pf_methphase_run(pf_ctx_t *ctx, pf_dbatch_t *db, pf_window_out_t *out);

/* Split, pipelined form of pf_methphase_run: pf_methphase_launch enqueues a
 * run and returns; pf_methphase_finish waits for the oldest unfinished run
 * and does its host epilogue (Fisher tests, decisions, tags).  Up to two runs
 * of a batch may be in flight, so the epilogue of one overlaps the kernels of
 * the next; a third launch before a finish returns PF_ERR_ARG. */
int  pf_methphase_launch(pf_ctx_t *ctx, pf_dbatch_t *db);
int  pf_methphase_finish(pf_ctx_t *ctx, pf_dbatch_t *db, pf_window_out_t *out);

/* Upload record-level input (pf_aln_batch_t).  The records stay resident in
 * HBM and every run of the batch starts with kernel K0, which applies the
 * loader's filters and extracts each kept read's 5mC calls on the device;
 * this call runs K0 once to size the batch.  The batch's reads are the kept
 * records in record order; pf_batch_read_recs maps them back. */
int  pf_batch_upload_aln(pf_ctx_t *ctx, const pf_cfg_t *cfg, const pf_load_cfg_t *lcfg,
                         const pf_aln_batch_t *aln, pf_dbatch_t **out);
/* rec_of_read[i] = record index of read i (n >= pf_batch_n_reads). */
int  pf_batch_read_recs(const pf_dbatch_t *db, uint32_t *rec_of_read, uint32_t n);
/* Parity/debug for K0: runs it and copies every read's calls sorted by
 * (pos, cat) as the methmer kernels consume them (call_off [R+1]), and the
 * first and last call of each read in get_mod_poss_on_ref's order.  Returns
 * the number of calls or < 0. */
int64_t pf_batch_debug_calls(pf_dbatch_t *db, uint64_t *call_off, uint32_t *pos, uint8_t *cat,
                             uint32_t *first, uint32_t *last, uint64_t cap);
/* Parity/debug for K0: runs it and copies every read's reference start and
 * end (bam_endpos) as K0 wrote them (n >= pf_batch_n_reads). */
int  pf_batch_debug_spans(pf_dbatch_t *db, uint32_t *start, uint32_t *end, uint32_t n);

/* K0 counters since upload (count pass + every run), out[0..7]: records
 * walked by the sequential path, records whose calls needed a sort, records
 * in implicit-canonical mode, records whose MM/ML could not be decoded,
 * emission chunks with a duplicate position.  n >= 8. */
/* test hook: a record-level batch's record arrays copied back (sizes[5] =
 * records, CIGAR ops, SEQ bytes (16-byte aligned slices), MM bytes, ML bytes;
 * flag == NULL fills sizes only) */
int  pf_batch_debug_recs(pf_dbatch_t *db, uint64_t *sizes, uint16_t *flag, uint8_t *mapq, uint32_t *pos,
                         uint32_t *l_qseq, float *de, uint8_t *hp, uint64_t *cigar_off, uint32_t *cigar,
                         uint64_t *seq_off, uint8_t *seq, uint64_t *mm_off, uint8_t *mm, uint64_t *ml_off,
                         uint8_t *ml);
int  pf_batch_load_counters(pf_dbatch_t *db, uint64_t *out, int n);

/* One-shot convenience: upload + run + free on `device`. */
int  pf_methphase_windows(int device, const pf_cfg_t *cfg,
                          const pf_window_batch_t *batch, pf_window_out_t *out);

/* Average device time (ms) of each kernel of the last run, measured with HIP
 * events on the library's stream.  names/ms arrays of length *n. */
int  pf_last_kernel_times(pf_ctx_t *ctx, const char **names, float *ms, int *n);

/* Per-(window,direction) counters of the last run, out[(w*2+dir)*8 + j]:
 * j=0 methmer lookups (in-range methmers of every scored candidate),
 * j=1 methmer insertions (reference reads + tagged reads), j=2 greedy
 * iterations that scored >= 1 candidate, j=3 reads visited by the candidate
 * scans, j=4 methmers of all reads, j=5 strict reference reads in the 2x2
 * table, j=6 reads, j=7 sites.  n >= 16*n_windows.  These feed the
 * algorithmic-byte model of DESIGN.md. */
int  pf_batch_stats(pf_dbatch_t *db, uint64_t *out, uint64_t n);
/* The greedy loop's slot-list source per (window, direction) of the last
 * run, out[w*2+dir]: 1 slot lists in LDS, 2 the candidate cache in LDS, 3
 * slot lists in HBM (the slim loop), 4 the general body (fallback kernel),
 * 5 the one-wave kernel (pf_k3_wave), 6 the candidate cache with the count
 * table in HBM (a problem a few KB past the main kernel's budget), 0 no
 * greedy run (no sites).  n >= 2*n_windows.  Tests assert which variant
 * PF_K3_CACHE / PF_K3_GCNT forced. */
int  pf_batch_k3_paths(pf_dbatch_t *db, uint8_t *out, uint64_t n);
/* K12's sites path per window of the last run, out[w]: 1 or 2 the fast
 * path (seen-twice bitmaps and rank counters) over one or two 512 kb
 * segments, 3 the dense path (per-chunk histograms in HBM: spans past 1 Mb,
 * or more repeated positions than a segment's counters), 0 no K12 sites pass
 * (no calls, or the left-coverage check of blockjoin.c:1161).  n >= n_windows.
 * Tests assert which path the wide headline windows took. */
int  pf_batch_k12_paths(pf_dbatch_t *db, uint8_t *out, uint64_t n);
/* The items (chunks of PF_K12C_READS reads of one window) K12 handed to
 * pf_k12_chunks in the last run; 0 when every window's methmer phase ran in
 * K12 itself.  Tests assert that PF_K12C_MINR forced the chunk route. */
int  pf_batch_k12_chunk_items(pf_dbatch_t *db, uint32_t *out);

/* Masked reference positions (the masked_poss set of get_methmer_sites_and_ranges,
 * blockjoin.c:3202-3205, 3277-3283): a position that qualifies as a
 * methylation site by its call counts and is in the mask is no site.  Nothing
 * else changes: the calls stay in their reads, the window's position range,
 * the reads' first and last calls, K12's path and the left-coverage check are
 * those of the unmasked run, so a masked run equals the unmasked run of the
 * batch whose calls at masked positions are no-calls (call_cat 2).
 * pos[0..n): strictly ascending 0-based positions of the batch's coordinate
 * space (a site's position is its call_pos value, the CpG's C), each below
 * 2^29 (PF_ERR_LIMIT).  win_rng NULL: every window sees the whole array;
 * else [2*n_windows] with window w seeing pos[win_rng[2w], win_rng[2w+1])
 * (begin <= end <= n, else PF_ERR_ARG).  n == 0 clears the mask.  Serves
 * window-level and record-level batches; copies to the device and
 * synchronises the context's stream; the mask stays in force for every later
 * run of the batch until replaced, and a refused call leaves the previous
 * mask in force. */
int  pf_batch_set_mask(pf_dbatch_t *db, const uint32_t *pos, uint64_t n, const uint32_t *win_rng);
/* out[w]: the qualifying positions the mask removed from window w in the last
 * finished run (the reference's n_filtered); zeros with no mask.  win_n_sites
 * counts the sites after masking.  n >= n_windows. */
int  pf_batch_masked_sites(pf_dbatch_t *db, uint32_t *out, uint64_t n);
/* The greedy launch this batch was given: out[0] the main kernel's dynamic
 * LDS per problem, out[1] its persistent workgroups (problems at once on the
 * device), out[2] pf_k3_heavy's dynamic LDS, out[3] its problems.  n >= 4. */
int  pf_batch_k3_budget(const pf_dbatch_t *db, uint32_t *out, uint64_t n);

/* The greedy problems (w<<1 | dir) this batch runs in pf_k3_heavy, the second
 * greedy kernel on the context's second stream: windows with at least 2,000
 * reads (1,100 when the batch's 90th-percentile window has <= 400 reads);
 * every other problem, heaviest first, runs in the main kernel.
 * PF_K3_HEAVY_X=x takes x times the median instead, PF_K3_HEAVY=n forces the
 * n heaviest problems.  Returns their count (<= cap copied). */
int  pf_batch_heavy(const pf_dbatch_t *db, uint32_t *probs, uint32_t cap);

/* Parity/debug: run K1 only and copy window w's sites (ms->sites_real_poss,
 * sites_starts, mmr_lens of direction dir); returns S or <0. */
int  pf_batch_debug_sites(pf_dbatch_t *db, uint32_t w, int dir, uint32_t *real,
                          uint32_t *starts, uint8_t *lens, uint32_t cap);
/* Parity/debug: run K1+K2 and copy every read's methmers of direction dir
 * (read_t.mmr_n, mmr_start_i, mmr keys back to back); returns #keys or <0. */
int64_t pf_batch_debug_methmers(pf_dbatch_t *db, int dir, uint32_t *mmr_n,
                                uint32_t *mmr_start, uint32_t *keys, uint64_t cap);

/* Per-haplotype CpG methylation pileup of a batch's calls (pf_pileup.hip; no
 * reference counterpart).  For window w every call entry of its reads with
 * win_start[w] <= pos < win_end[w] and cat 0 (meth) or 1 (unmeth) adds one to
 * cnt[pos][h][cat]; h = 0 / 1 for read_hp 0 / 1 and 2 for every other tag (254
 * untagged, HP >= 3).  No-calls (cat 2) count nowhere; a read with two entries
 * at one position counts twice; a read of two windows counts in each, inside
 * that window's range; K12's left-coverage check does not apply.  A position
 * with a non-zero counter is a site.  The result is an exactly sized CSR owned
 * by the library (pf_pileup_free), the same for any tile size. */
typedef struct pf_pileup {
    uint32_t n_windows;
    uint64_t n_sites;
    const uint64_t *win_off;   /* [n_windows+1]                                  */
    const uint32_t *pos;       /* [n_sites] ascending inside a window            */
    const uint32_t *cnt;       /* [n_sites*6] index h*2+cat; h 0,1,2=other; cat 0 meth,1 unmeth */
    float ms_kernels;          /* event-timed: the pileup kernels only           */
} pf_pileup_t;
/* Record-level batches run their load stage (K0, scan, pack) first.  read_hp
 * NULL: the batch's own tags; else [n_hp] tags in read order that replace them
 * for this call only (e.g. pf_window_out_t.read_hp of a run), n_hp equal to
 * pf_batch_n_reads after the load (PF_ERR_ARG otherwise).  PF_ERR_ARG while a
 * launched run is unfinished.  The batch is left as it was.  Counts are exact
 * up to 65,535 per counter; a count past that (duplicate entries only: a
 * window holds at most 65,535 reads) returns PF_ERR_LIMIT.  PF_PILE_TILE=<n>
 * in the environment (tests) sets the LDS tile to n positions, a power of two
 * in [64, 8192]; the default is 4,096. */
int  pf_batch_pileup(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, pf_pileup_t **out);
void pf_pileup_free(pf_pileup_t *p);

/* Allele-specific methylated regions of a pileup (pf_dmr.hip; no reference
 * counterpart): a segmented scan over the sites of windows [w0, w1), all in
 * integers.  With m1,u1,m2,u2 = cnt[0..3] of a site, n1 = m1+u1, n2 = m2+u2:
 *   informative  n1 >= min_cov && n2 >= min_cov; every other site is
 *                transparent (it neither joins nor breaks anything; the
 *                "other" class cnt[4..5] is ignored);
 *   sign         d = (m1*n2 - m2*n1) * 100, t = min_delta_pct * n1 * n2 in 64
 *                bits: +1 if d >= t, else -1 if -d >= t, else 0;
 *   join         two consecutive informative sites a < b are joined iff they
 *                have the same non-zero sign, b - a <= max_gap and no break x
 *                lies in a < x <= b (breaks: a sorted array given per call;
 *                HP tags are comparable only inside one phase block);
 *   run          a maximal chain of joined sites; a sign-0 site forms no run
 *                and ends any run. */
typedef struct pf_dmr_cfg {
    uint32_t min_cov;          /* default 5                                      */
    uint32_t min_delta_pct;    /* default 40; at most 100                        */
    uint32_t max_gap;          /* default 500                                    */
    uint32_t min_sites;        /* default 5                                      */
} pf_dmr_cfg_t;

#define PF_DMR_OPEN_LEFT  1u   /* the run's first member is the range's first informative site */
#define PF_DMR_OPEN_RIGHT 2u   /* the run's last member is the range's last informative site   */
typedef struct pf_dmr_run {
    uint32_t start;            /* first member's position                        */
    uint32_t end;              /* last member's position + 1                     */
    uint32_t n_sites;          /* members                                        */
    int32_t  sign;             /* +1: haplotype 1 more methylated, -1: less      */
    uint64_t sum[4];           /* the members' m1, u1, m2, u2 summed             */
    uint32_t open;             /* PF_DMR_OPEN_* bits                             */
    uint32_t reserved;
} pf_dmr_run_t;

typedef struct pf_dmr {
    uint64_t n_runs;
    const pf_dmr_run_t *runs;  /* [n_runs] ascending                             */
    uint64_t n_informative;    /* informative sites of the range                 */
    float ms_kernels;          /* event-timed: the region kernels only           */
    float ms_upload;           /* host clock: the range's pos, cnt and the breaks to the device */
} pf_dmr_t;

/* The runs of the sites of windows [w0, w1) of pile with n_sites >= min_sites
 * or open != 0 (open runs come back unfiltered so that ranges can be stitched,
 * pf_dmr_acc_*).  Positions must be strictly ascending over the whole range
 * (disjoint consecutive windows; overlapping methphase windows are not):
 * PF_ERR_ARG otherwise, and for unsorted breaks or min_delta_pct > 100.  A
 * count above 65,535 returns PF_ERR_LIMIT.  Runs on ctx's stream; the result
 * is exactly sized and owned by the library (pf_dmr_free), the same for any
 * block size.  An empty range, no site and no informative site are valid,
 * empty results.  PF_DMR_BLOCK=<n> in the environment (tests) sets the sites
 * per workgroup, a power of two in [64, 1024]; the default is 1,024; any other
 * value returns PF_ERR_ARG.  pf_dmr_regions_block takes the block as an
 * argument instead (0: the environment's or the default). */
int  pf_dmr_regions(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                    const uint32_t *breaks, uint32_t n_breaks, pf_dmr_t **out);
int  pf_dmr_regions_block(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                          const uint32_t *breaks, uint32_t n_breaks, uint32_t block, pf_dmr_t **out);
void pf_dmr_free(pf_dmr_t *d);

/* Stitching (host only): the results of consecutive ranges of one contig, in
 * ascending position order, give the runs of the whole -- independent of how
 * the contig was cut.  A part's open-left run joins the carried open-right run
 * under the join rule above; a part with n_informative == 0 leaves the carry
 * open; a part whose first informative site is in no open-left run closes it;
 * min_sites is applied when a run closes.  pf_dmr_acc_flush closes the carry,
 * returns every closed run so far (open = 0; pf_dmr_free) and leaves the
 * accumulator empty for the next contig's parts under the same cfg and breaks. */
typedef struct pf_dmr_acc pf_dmr_acc_t;
pf_dmr_acc_t *pf_dmr_acc_new(const pf_dmr_cfg_t *cfg, const uint32_t *breaks, uint32_t n_breaks);
int  pf_dmr_acc_add(pf_dmr_acc_t *acc, const pf_dmr_t *part);
int  pf_dmr_acc_flush(pf_dmr_acc_t *acc, pf_dmr_t **final);
void pf_dmr_acc_free(pf_dmr_acc_t *acc);

/* Allele-specific regions by a hidden Markov model (pf_dmr_hmm.hip; no
 * reference counterpart): where pf_dmr_regions asks every CpG of a run to pass
 * a fixed difference, this sums per-site evidence along the contig and makes a
 * region pay to open and to close, so one noisy CpG does not cut a region in
 * two.  Input as pf_dmr_regions: the position-sorted sites of windows [w0, w1)
 * of a pileup, pf_dmr_cfg_t and sorted breaks.  All in integers; L is
 * pf_ilog2_q16; scores are int64 in Q16 bits.
 *   informative  n1 >= min_cov && n2 >= min_cov; every other site is
 *                transparent, as in pf_dmr_regions;
 *   chain        a maximal sequence of consecutive informative sites a < b
 *                with b - a <= max_gap and no break x in a < x <= b
 *                (pf_dmr_regions' join rule without the sign); chains are
 *                independent of one another;
 *   evidence     of an informative site, with m = m1+m2, u = u1+u2, n = n1+n2:
 *                sep  = m1*(L(m1+1)-L(n1+2)) + u1*(L(u1+1)-L(n1+2))
 *                     + m2*(L(m2+1)-L(n2+2)) + u2*(L(u2+1)-L(n2+2)),
 *                pool = m*(L(m+1)-L(n+2)) + u*(L(u+1)-L(n+2)),
 *                g = min(max(sep - pool, 0), 2^28): the Laplace-smoothed
 *                log-likelihood ratio, in bits, of "two levels" against "one
 *                level"; d = m1*n2 - m2*n1; e = g if d > 0, -g if d < 0, else
 *                0 (pf_dmr_hmm_evidence).  With the clamp, and the two costs at
 *                most 2^22 each, every path sum stays below 2^60 in magnitude
 *                for any range below 2^31 sites;
 *   states       0 none, 1 h1>h2, 2 h1<h2; emission em[0] = 0,
 *                em[1] = e - site_cost_q16, em[2] = -e - site_cost_q16;
 *   Viterbi      per chain: V_0[s] = em_0[s]; for i >= 1
 *                cand(r,s) = V_{i-1}[r] - (r != s ? switch_q16 : 0),
 *                best[s] = max_r cand(r,s), V_i[s] = em_i[s] + best[s],
 *                bp_i[s] = s if cand(s,s) == best[s], else the smallest r that
 *                attains it.  The last site's state is the smallest s that
 *                attains max V_last; x_{i-1} = bp_i[x_i].  Both ends of a chain
 *                are free;
 *   run          a maximal stretch of consecutive sites of one chain in one
 *                non-zero state: start, end, n_sites (all members, the weak
 *                ones included), sign (+1 for state 1, -1 for state 2), sum[4]
 *                over the members, open = 0;
 *   kept         a run with n_sites >= min_sites and, with M1,U1,M2,U2 = sum[],
 *                N1 = M1+U1, N2 = M2+U2,
 *                sign*(M1*N2 - M2*N1)*100 >= min_delta_pct*N1*N2 in 128 bits:
 *                under the model min_delta_pct is a property of the region's
 *                pooled levels, not of each CpG.
 * There is no stitching: the call takes everything the caller regards as a
 * whole, and the chains at the range's ends are closed there.  The device
 * result is the sequential one bit for bit, for any block: the forward pass is
 * a scan of 3x3 max-plus matrices, the backtrace a reverse scan of composed
 * maps {0,1,2} -> {0,1,2}, both exact and associative.  The two defaults are
 * choices made on simulated data, not measured on real samples. */
typedef struct pf_dmr_hmm_cfg {
    int32_t site_cost_q16;     /* what a site pays to be in state 1 or 2; default 2 bits (131,072); [0, 64*65536] */
    int32_t switch_q16;        /* what a change of state pays; default 8 bits (524,288); [0, 64*65536]            */
} pf_dmr_hmm_cfg_t;

#define PF_DMR_HMM_SITES 1u    /* flags: also return state[] and evidence[] */
typedef struct pf_dmr_hmm {
    uint64_t n_runs;
    const pf_dmr_run_t *runs;  /* [n_runs] ascending, the kept runs, open = 0    */
    uint64_t n_informative;    /* informative sites of the range                 */
    uint64_t n_chains;         /* chains of the range                            */
    uint64_t n_sites;          /* sites of the range                             */
    const uint8_t *state;      /* [n_sites] 0, 1, 2; 255 a transparent site; NULL without PF_DMR_HMM_SITES */
    const int64_t *evidence;   /* [n_sites] e; 0 at a transparent site; NULL without PF_DMR_HMM_SITES      */
    float ms_kernels;          /* event-timed: the model's and the run kernels   */
    float ms_upload;           /* host clock: the range's pos, cnt and the breaks to the device */
} pf_dmr_hmm_t;

/* The kept runs of the sites of windows [w0, w1) of pile.  Errors as
 * pf_dmr_regions (positions not ascending, unsorted breaks, min_delta_pct >
 * 100: PF_ERR_ARG; a count above 65,535: PF_ERR_LIMIT), and PF_ERR_ARG for a
 * cost outside [0, 64*65536].  block as in pf_dmr_regions_block: 0 is
 * PF_DMR_BLOCK of the environment or 1,024; a power of two in [64, 1024].  An
 * empty range and a range without an informative site are valid, empty
 * results.  Runs on ctx's stream; the result is owned by the library
 * (pf_dmr_hmm_free). */
int  pf_dmr_hmm_regions(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                        const pf_dmr_hmm_cfg_t *hcfg, const uint32_t *breaks, uint32_t n_breaks, uint32_t block,
                        uint32_t flags, pf_dmr_hmm_t **out);
void pf_dmr_hmm_free(pf_dmr_hmm_t *h);
/* e of a site on the host (the code the kernels compile); each count at most
 * 65,535, 0 for anything larger. */
int64_t pf_dmr_hmm_evidence(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2);

/* Given regions (pf_regions.hip; no reference counterpart): what the two
 * haplotypes look like inside regions the caller names, whether or not either
 * region call above would have found them.  Input as pf_dmr_regions: the
 * position-sorted sites of windows [w0, w1) of a pileup and pf_dmr_cfg_t, of
 * which min_cov and min_delta_pct are used and max_gap and min_sites are not.
 * A region is half-open [start, end); regions may come in any order and may
 * overlap, nest and repeat, every region is summed on its own, and none of that
 * changes the cost: the kernels make the prefix sums of the range once and a
 * region is the difference of two rows.  The informative rule and the sign are
 * pf_dmr_regions', the evidence is pf_dmr_hmm_regions' e.
 * Additivity: every field is a sum over sites, so the records of one region
 * over two disjoint site ranges add field by field to its record over their
 * union.  That is all the stitching there is: a caller that cuts a contig into
 * ranges adds the parts. */
typedef struct pf_region_sum {
    uint32_t n_cpg;            /* sites of the range with start <= pos < end                 */
    uint32_t n_sites;          /* of those, informative (pf_dmr_cfg_t.min_cov on both haps)  */
    uint32_t n_pos;            /* informative sites with sign +1 (pf_dmr_regions' sign rule) */
    uint32_t n_neg;            /* ... with sign -1                                           */
    uint64_t sum[4];           /* informative sites' m1, u1, m2, u2                          */
    int64_t  evidence;         /* sum of e (pf_dmr_hmm_evidence) over informative sites, Q16 */
} pf_region_sum_t;
typedef struct pf_regions {
    uint64_t n;
    const pf_region_sum_t *r;  /* [n], in the caller's region order                          */
    uint64_t n_informative;    /* informative sites of the range                             */
    float ms_kernels;          /* event-timed: the four kernels                              */
    float ms_upload;           /* host clock: the range's pos and cnt and the regions to the device */
} pf_regions_t;
/* Errors as pf_dmr_regions: positions not strictly ascending over the range or
 * min_delta_pct > 100: PF_ERR_ARG; a count above 65,535: PF_ERR_LIMIT.  A
 * region with start > end: PF_ERR_ARG; start == end is an empty region, all
 * zero.  n_regions >= 2^31: PF_ERR_LIMIT.  n_regions == 0, an empty range and a
 * range without sites are valid results.  block: sites per workgroup, a power
 * of two in [64, 1024]; 0 is PF_REG_BLOCK of the environment or 1,024; any
 * other value PF_ERR_ARG.  The records are the same for any block.  Scratch on
 * the device: 64 bytes per site of the range while the call runs.  Runs on
 * ctx's stream; the result is owned by the library (pf_regions_free). */
int  pf_region_sums(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                    const uint32_t *reg_start, const uint32_t *reg_end, uint64_t n_regions, uint32_t block,
                    pf_regions_t **out);
void pf_regions_free(pf_regions_t *r);

/* Read-label permutation test of windows (pf_perm.hip; no reference
 * counterpart): for each window [ws, we) of a batch, how often a random
 * relabelling of its reads separates the two pooled methylation fractions at
 * least as far as the reads' own tags do.  The read is the exchangeable unit,
 * so the p-value (hits + 1) / (n_perm + 1) holds under the correlation of one
 * read's calls, which the pooled Fisher test of pf_write_dmr ignores.  All in
 * integers; windows may overlap, every window is tested on its own.
 *   participating  the window's reads with tag 0 or 1 and at least one call
 *                  entry with ws <= pos < we and cat 0 or 1, in the batch's
 *                  read order, numbered i = 0 .. n-1;
 *   counts         m_i / u_i the read's meth / unmeth entries in range (a
 *                  duplicate entry counts twice, cat 2 nowhere); n1 the
 *                  participating reads tagged 0, M = sum m_i, N = sum (m_i + u_i);
 *   statistic      for a labelling L with M0, N0 the sums over the reads
 *                  labelled 0: A(L) = |M0*N - M*N0|, D(L) = N0*(N - N0); A/D is
 *                  the absolute difference of the two pooled fractions.  A0,
 *                  D0 are those of the true tags;
 *   keys           uint32 arithmetic with wrap-around;
 *                  mix(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15;
 *                          x *= 0x846ca68b; x ^= x>>16;
 *                  base = mix(seed ^ mix(ws ^ mix(we))): the salt is the
 *                  window's coordinates, not its index, so a region's result
 *                  does not depend on the batch it lands in;
 *                  key(b, i) = mix(mix(base + b) ^ i);
 *   permutation b  (0 <= b < n_perm) rank(i) = the number of j with
 *                  (key(b,j), j) < (key(b,i), i) lexicographically; read i is
 *                  labelled 0 iff rank(i) < n1; b is a hit iff D_b > 0 and
 *                  A_b*D0 >= A0*D_b, compared as 128-bit values;
 *   status         0 tested; 1 nothing to test (n1 == 0, n1 == n or D0 == 0),
 *                  hits 0; 2 n > PF_PERM_MAX_READS, hits 0 (no error). */
#define PF_PERM_MAX_READS 4096u
#define PF_PERM_MAX_PERM  1000000u
typedef struct pf_perm {
    uint32_t n_windows;
    uint32_t n_perm;
    uint32_t seed;
    const uint32_t *n_reads;   /* [n_windows*2] participating reads tagged 0, tagged 1 */
    const uint64_t *sum;       /* [n_windows*4] their m1, u1, m2, u2 in range    */
    const uint32_t *hits;      /* [n_windows]                                    */
    const uint32_t *status;    /* [n_windows] 0, 1, 2 as above                   */
    float ms_kernels;          /* event-timed: the kernels only                  */
} pf_perm_t;
/* Batches and tags as in pf_batch_pileup: calls-level and record-level batches
 * (the latter run their load stage first); read_hp NULL uses the batch's own
 * tags, else [n_hp] tags replace them for this call only; PF_ERR_ARG while a
 * launched run is unfinished; the batch is left as it was.  n_perm outside
 * [1, PF_PERM_MAX_PERM] returns PF_ERR_ARG, N >= 2^31 in any window
 * PF_ERR_LIMIT.  The result is owned by the library (pf_perm_free) and depends
 * on neither launch geometry nor atomic order.  PF_PERM_THREADS=<64|256|1024>
 * in the environment (tests) sets the workgroup size; the default is 256; any
 * other value returns PF_ERR_ARG. */
int  pf_batch_permtest(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t n_perm,
                       uint32_t seed, pf_perm_t **out);
void pf_perm_free(pf_perm_t *p);

/* Read-level rank-sum test of windows (pf_rank.hip; no reference counterpart):
 * the Mann-Whitney U test between the two haplotypes' reads, each read
 * contributing its own methylation fraction inside the window.  The read is
 * the exchangeable unit, as in the permutation test; here the null
 * distribution has a closed form (pf_rank_p), so the p-value has no floor and
 * costs one pass, and AUC = U / (n1*n2) is a read-level effect size.  All in
 * integers; windows may overlap, every window is tested on its own.
 *   participating  as in pf_batch_permtest: tag 0 or 1, m_i / u_i the read's
 *                  cat 0 / cat 1 entries with ws <= pos < we (a duplicate entry
 *                  counts each time, cat 2 nowhere), n_i = m_i + u_i >= 1;
 *   counted        a participating read with n_i >= min_calls; n_short[h] the
 *                  participating reads tagged h below min_calls; n1 / n2 the
 *                  counted reads tagged 0 / 1;
 *   order          f_i > f_j iff m_i*n_j > m_j*n_i, equal iff the products are
 *                  equal, in unsigned 64-bit arithmetic (N = sum of n_i over the
 *                  participating reads is below 2^31, so products stay below
 *                  2^62); never floating point;
 *   statistic      over the pairs (i tagged 0, j tagged 1) of counted reads
 *                  G = #{f_i > f_j}, E = #{f_i == f_j}; u2 = 2G + E, twice
 *                  haplotype 1's U, in [0, 2*n1*n2];
 *   ties           T = sum of t^3 - t over the groups of equal fraction among
 *                  all counted reads = sum over i of e_i^2 - 1, e_i the counted
 *                  reads with f_j == f_i, i itself included;
 *   classes        per tag the counted reads with u_i == 0 (all-meth), with
 *                  m_i == 0 (all-unmeth) and with both above 0 (mixed); sum[4]
 *                  the counted reads' m1, u1, m2, u2;
 *   status         0 tested; 1 nothing to test (n1 == 0 or n2 == 0), u2 and T
 *                  0; 2 more than PF_RANK_MAX_READS counted reads, u2 and T 0
 *                  (no error). */
#define PF_RANK_MAX_READS 4096u
typedef struct pf_rank {
    uint32_t n_windows;
    uint32_t min_calls;
    const uint32_t *n_reads;   /* [n_windows*2] counted reads tagged 0, tagged 1  */
    const uint32_t *n_short;   /* [n_windows*2] participating reads below min_calls */
    const uint32_t *cls;       /* [n_windows*6] all-meth, all-unmeth, mixed of tag 0, then of tag 1 */
    const uint64_t *sum;       /* [n_windows*4] the counted reads' m1, u1, m2, u2 */
    const uint64_t *u2;        /* [n_windows] 2G + E                              */
    const uint64_t *ties;      /* [n_windows] T                                   */
    const uint32_t *status;    /* [n_windows] 0, 1, 2 as above                    */
    float ms_kernels;          /* event-timed: the kernel only                    */
} pf_rank_t;
/* Batches, tags, the refusal while a run is in flight and ownership
 * (pf_rank_free) exactly as in pf_batch_permtest; the batch is left as it was.
 * min_calls outside [1, 65535] returns PF_ERR_ARG, N >= 2^31 in any window
 * PF_ERR_LIMIT.  One workgroup per window; a window whose largest n_i is at
 * most 65,535 is compared with 32-bit products, any other with 64-bit ones.
 * The result depends on neither launch geometry, the product width nor atomic
 * order.  In the environment (tests): PF_RANK_THREADS=<64|256|1024> sets the
 * workgroup size (default 256); PF_RANK_WIDE=1 forces the 64-bit products for
 * every window, unset or 0 leaves the choice per window; any other value of
 * either returns PF_ERR_ARG. */
int  pf_batch_ranktest(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                       pf_rank_t **out);
void pf_rank_free(pf_rank_t *r);

/* The same test over position ranges inside the batch's windows (pf_rank.hip,
 * pf_rank_ranges): range i of window w (rng_off[w] <= i <
 * rng_off[w+1]) is tested over window w's reads by pf_batch_ranktest's
 * definition, word for word, with ws, we := rng_start[i], rng_end[i].
 * Participating and counted reads, order, statistic, ties, classes, sum,
 * status 0 / 1 / 2 and the N < 2^31 limit hold per range; a read takes part
 * in every range it has calls in.  The result's n_windows is the number of
 * ranges, every array holds one entry per range in range order, and
 * pf_rank_free frees it.  Ranges of one window may overlap and may be empty
 * (start == end: status 1 and zeros); a window may have no range.  rng_off is
 * [n_windows + 1] with rng_off[0] == 0, non-decreasing (it may be NULL for a
 * batch without windows); rng_start / rng_end hold rng_off[n_windows] entries.
 * PF_ERR_ARG: ws <= start <= end <= we violated for a range of window [ws,
 * we), rng_off not as above, more than 2^31 - 1 ranges, min_calls outside [1,
 * 65535]; PF_ERR_LIMIT: N >= 2^31 in a range, or ranges times the workgroup
 * size above 2^32 - 1 (one workgroup per range, one launch: 16.7 M ranges at
 * the default 256 threads, 67 M at 64).  Batches, the tag override, the
 * refusal while a run is in flight and ownership as in pf_batch_ranktest; the
 * batch is left as it was.  A workgroup keeps its counted reads in an LDS
 * array of min(4,096, the reads of the largest window that has a range),
 * rounded up to a power of two.  The result depends on neither the launch
 * geometry, the product width nor any atomic order.  In the environment
 * (tests): PF_RANK_THREADS and PF_RANK_WIDE as in pf_batch_ranktest;
 * PF_RANKR_LDS_FIXED=1 takes the 4,096-read array whatever the batch (unset or
 * 0: sized as above); any other value returns PF_ERR_ARG. */
int  pf_batch_rankranges(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                         const uint64_t *rng_off, const uint32_t *rng_start, const uint32_t *rng_end, pf_rank_t **out);

/* The rank test's two-sided p-value by the normal approximation with tie and
 * continuity correction (host only), in doubles in exactly this order:
 *   a = (double)n1 * (double)n2;  n = (double)n1 + (double)n2;
 *   auc = u2 / (2a);
 *   var = (a / 12) * ((n + 1) - T / (n * (n - 1)));
 *   var <= 0 (every read tied): z = 0, p = 1;
 *   else d = max(|u2 - a| / 2 - 0.5, 0);  z = d / sqrt(var);
 *        p = min(1, erfc(z / sqrt(2))).
 * It is scipy.stats.mannwhitneyu(alternative="two-sided", method="asymptotic",
 * use_continuity=True).  The test is asymptotic: approximate below about eight
 * reads per haplotype.  p underflows to 0 near z > 38; z does not.  PF_ERR_ARG
 * when n1 or n2 is 0 or u2 > 2*n1*n2.  auc, z and p may each be NULL. */
int  pf_rank_p(uint64_t u2, uint32_t n1, uint32_t n2, uint64_t ties, double *auc, double *z, double *p);

/* The rank test's exact null distribution for small windows (pf_rank.hip,
 * pf_rank_exact; no reference counterpart): conditional on the counted reads'
 * fractions, ties included, every assignment of n1 of the n = n1 + n2 counted
 * reads to haplotype 1 is equally likely.  Participating and counted reads,
 * the order of fractions and the N < 2^31 limit are pf_batch_ranktest's.  For
 * a subset A of the counted reads with |A| = n1
 *   u2(A) = 2 * #{(i in A, j not in A): f_i > f_j} + #{(i in A, j not in A): f_i == f_j},
 * A0 the reads tagged 0, u2(A0) = pf_rank_t.u2, and over all C(n, n1) subsets
 *   total  C(n, n1);
 *   le     #{A: u2(A) <= u2(A0)};   ge  #{A: u2(A) >= u2(A0)};
 *   two    #{A: |u2(A) - n1*n2| >= |u2(A0) - n1*n2|}, in signed 64-bit arithmetic;
 *   status 0 tested; 1 n1 == 0 or n2 == 0, every count 0; 2 n > max_reads,
 *          every count 0 (no error).
 * le / total and ge / total are the exact one-sided p-values, two / total the
 * two-sided one (pf_rank_exact_p).  Counted as subset sums: with r_i = 2 * #{j:
 * f_j < f_i} + #{j: f_j == f_i} (i included), u2(A) = sum of r_i over A - |A|^2,
 * so ways[c][s] += ways[c-1][s - r_i] per read, for the smaller class, le and
 * ge swapped where that is haplotype 2.  C(64, 32) < 2^63: every count and
 * intermediate fits 64 bits, which C(68, 34) does not; 64 is the limit.
 * n_reads, n_short and u2 are pf_batch_ranktest's for the same batch, tags and
 * min_calls, u2 also where status is 2. */
#define PF_RANK_EXACT_MAX_READS 64u
typedef struct pf_rank_exact {
    uint32_t n_windows;
    uint32_t min_calls;
    uint32_t max_reads;
    const uint32_t *n_reads;   /* [n_windows*2] counted reads tagged 0, tagged 1  */
    const uint32_t *n_short;   /* [n_windows*2] participating reads below min_calls */
    const uint32_t *status;    /* [n_windows] 0, 1, 2 as above                    */
    const uint64_t *u2;        /* [n_windows] pf_rank_t.u2                        */
    const uint64_t *total;     /* [n_windows] C(n, n1)                            */
    const uint64_t *le;        /* [n_windows]                                     */
    const uint64_t *ge;        /* [n_windows]                                     */
    const uint64_t *two;       /* [n_windows]                                     */
    float ms_kernels;          /* event-timed: the kernel only                    */
} pf_rank_exact_t;
/* Batches, tags, check order, return codes, the refusal while a run is in
 * flight and ownership (pf_rank_exact_free) exactly as in pf_batch_ranktest;
 * the batch is left as it was.  max_reads outside [2, PF_RANK_EXACT_MAX_READS]
 * returns PF_ERR_ARG.  At most 512 workgroups, each taking every 512th window;
 * a window's table lies in LDS where it has at most 8,113 cells of 8 bytes (up
 * to 36 counted reads, or a small class), else in the workgroup's slab in
 * device memory (358 KB at max_reads 64).  The result depends on no launch
 * geometry, no table placement and no atomic order.  In the environment
 * (tests): PF_RANKX_THREADS=<64|256|1024> sets the workgroup size (default
 * 1024), PF_RANKX_HBM=1 puts every window's table in its slab (unset or 0: per
 * window), PF_RANKX_GRID=<n>, 1 .. 65536, caps the workgroups; any other value
 * of the three returns PF_ERR_ARG. */
int  pf_batch_rankexact(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                        uint32_t max_reads, pf_rank_exact_t **out);
void pf_rank_exact_free(pf_rank_exact_t *r);

/* An exact p-value from its counts (host only): *p = (double)count /
 * (double)total.  PF_ERR_ARG when total == 0 or count > total. */
int  pf_rank_exact_p(uint64_t count, uint64_t total, double *p);

/* Tags for untagged reads from a window's allele-specific methylation
 * (pf_assign.hip; no reference counterpart): inside a window [ws, we) where
 * the two haplotypes' methylation differs, an untagged read's own calls say
 * which haplotype it came from.  The tagged reads give the per-site model, the
 * untagged read is never part of it.  All in integers; windows may overlap,
 * every window is scored on its own.  Out of scope: writing a retagged BAM;
 * merging one read's scores across regions or phase blocks (one row per
 * (window, read), the consumer decides); filtering regions by perm_p; more
 * than one device.  Leave-one-out scoring of the reads that carry a tag is
 * pf_batch_tagcheck's, below.
 *   model        for every position p of the window m1,u1,m2,u2 are the meth /
 *                unmeth entries of the window's reads tagged 0 and 1, exactly
 *                pf_batch_pileup's cnt[0..3]; n1 = m1+u1, n2 = m2+u2; p is
 *                informative iff n1 >= min_cov && n2 >= min_cov (pf_dmr_cfg_t's
 *                rule).  Tags other than 0 / 1 never enter the model;
 *   L(x), x >= 1 a Q16 fixed-point log2 defined by this algorithm, not by libm
 *                (pf_ilog2_q16): e = floor(log2 x); y = (uint64)x << (31 - e);
 *                f = 0; 16 times: y = (y*y) >> 31, f <<= 1, and if y >= 2^32
 *                then y >>= 1, f |= 1; L = (e << 16) | f.  Never above
 *                floor(65536*log2 x) and at most 1 below it;
 *   weights      of an informative site, Laplace-smoothed log-odds, int32:
 *                wM = L(m1+1) - L(n1+2) - L(m2+1) + L(n2+2) for a meth entry,
 *                wU = L(u1+1) - L(n1+2) - L(u2+1) + L(n2+2) for an unmeth one
 *                (counts reach 65,535, so arguments reach 131,072);
 *   candidates   the window's reads whose tag is exactly 254 (untagged), in
 *                the batch's read order; tags 0, 1 and HP >= 3 never;
 *   score        S (int64) the sum of wM / wU over the candidate's call entries
 *                with ws <= pos < we, cat 0 / 1, at an informative position;
 *                n_used the number of those entries.  A duplicate entry counts
 *                each time; cat 2 and non-informative positions count nowhere;
 *                an informative site whose weights are both 0 still counts in
 *                n_used;
 *   decision     new tag 0 iff n_used >= min_calls && S >= min_llr_q16 && S > 0;
 *                new tag 1 iff n_used >= min_calls && -S >= min_llr_q16 && S < 0;
 *                else the candidate stays 254. */
typedef struct pf_assign_cfg {
    uint32_t min_cov;          /* calls per haplotype a site needs (the --dmr one)   */
    uint32_t min_calls;        /* informative entries a candidate needs              */
    int64_t  min_llr_q16;      /* least |S|, Q16 bits: 3 bits (odds of 8:1) = 196608 */
} pf_assign_cfg_t;

typedef struct pf_assign {
    uint32_t n_windows;
    uint32_t n_reads;
    const uint32_t *win_read_off;  /* [n_windows+1] the batch's reads per window        */
    const uint32_t *n_used;    /* [n_reads] 0 for non-candidates                     */
    const int64_t  *llr;       /* [n_reads] S, Q16; 0 for non-candidates             */
    const uint8_t  *hp;        /* [n_reads] the new tag for candidates, the input tag
                                  for every other read: read_hp for pf_batch_pileup  */
    const uint32_t *win_n;     /* [n_windows*3] candidates with n_used >= 1, assigned
                                  0, assigned 1                                      */
    float ms_kernels;          /* event-timed: the assign kernels only (the site
                                  table's pileup kernels are not part of it)         */
} pf_assign_t;
/* Batches and tags as in pf_batch_permtest: calls-level and record-level
 * batches (the latter run their load stage first); read_hp NULL uses the
 * batch's own tags, else [n_hp] tags replace them for this call only (n_hp
 * equal to the batch's reads, PF_ERR_ARG otherwise); PF_ERR_ARG while a
 * launched run is unfinished; the batch is left as it was; no window is a
 * valid empty result.  A batch read belongs to exactly one window, so the
 * per-read arrays are dense.  The site table is pf_batch_pileup's, kept on the
 * device (its limits apply: a count past 65,535 returns PF_ERR_LIMIT).  The
 * result is owned by the library (pf_assign_free) and depends on neither
 * launch geometry nor atomic order: every sum is an integer sum.  min_llr_q16
 * below 1 acts as 1 (S > 0 / S < 0 is required anyway).  PF_ASSIGN_TILE=<n> in
 * the environment (tests) sets the sites per LDS tile, a power of two in
 * [64, 4096]; the default is 4,096; any other value returns PF_ERR_ARG. */
int  pf_batch_assign(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, const pf_assign_cfg_t *cfg,
                     pf_assign_t **out);
void pf_assign_free(pf_assign_t *a);
/* L(x) as defined above, on the host (the kernels compute the same); 0 for x == 0. */
uint32_t pf_ilog2_q16(uint32_t x);
/* The two weights of a site with the counts m1, u1, m2, u2 (host; the kernels
 * compute the same): w[0] = wM, w[1] = wU. */
void pf_assign_site_weights(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2, int32_t w[2]);

/* Leave-one-out check of read tags (pf_tagcheck.hip; no reference counterpart):
 * how far pf_batch_assign's rule can be trusted on this sample.  Every read
 * that carries a tag is scored against its window's model with the read's own
 * entries taken out, under exactly pf_batch_assign's rule: the share of reads
 * that get their own tag back is the accuracy estimate for an assigned tag at
 * the chosen thresholds, and a read that gets the other tag is a mis-tag or
 * switch-error candidate.  Scoring a tagged read against the model it helped to
 * build would be circular: where the haplotypes do not differ at all it still
 * agrees with itself.  All in integers; L is pf_ilog2_q16.  Out of scope:
 * removing all of a read's duplicate entries at a site (below); rewriting tags
 * or a BAM; merging a read's verdicts across regions; choosing thresholds;
 * more than one device.
 *   model        per window [ws, we) and position p the pileup's m1, u1, m2, u2
 *                under the call's tags, as in pf_batch_assign;
 *   scored reads the window's reads tagged exactly 0 or 1; h is the read's tag;
 *   leave one out  each entry of a scored read (position p, ws <= p < we,
 *                category c: 0 meth, 1 unmeth) is scored against the counts
 *                with that one entry removed: m_h or u_h at p is one less,
 *                giving m1', u1', m2', u2' and n1', n2'; the other haplotype's
 *                counts are untouched.  A duplicate entry of one read at one
 *                position removes one entry each time, not all of them: the
 *                read's other entry at p stays in the model.  That keeps the
 *                weight a function of (site, tag, category);
 *   usable       the entry is usable iff n1' >= min_cov && n2' >= min_cov;
 *   weight       of a usable meth entry L(m1'+1) - L(n1'+2) - L(m2'+1) + L(n2'+2),
 *                of an unmeth one the same in u.  Per site that is four weights,
 *                  tag 0: wM0 = L(m1) - L(n1+1) - L(m2+1) + L(n2+2),
 *                         wU0 = L(u1) - L(n1+1) - L(u2+1) + L(n2+2),
 *                  tag 1: wM1 = L(m1+1) - L(n1+2) - L(m2) + L(n2+1),
 *                         wU1 = L(u1+1) - L(n1+2) - L(u2) + L(n2+1),
 *                and two flags: tag 0 usable iff n1 - 1 >= min_cov && n2 >= min_cov
 *                (n1 >= 1), tag 1 iff n2 - 1 >= min_cov && n1 >= min_cov (n2 >= 1).
 *                L(0) is never evaluated: an in-range entry of category c on a
 *                read tagged h is itself counted, so that count is >= 1; where
 *                it is 0 no read can look the weight up and 0 stands for it.
 *                Arguments stay inside 1 .. 131,072 and |w| < 2^22;
 *   score        S (int64) the sum over the read's usable entries, n_used their
 *                number (cat 2 counts nowhere); positive favours tag 0;
 *   decision     d is pf_batch_assign's on (S, n_used) with min_calls and
 *                min_llr_q16: 0, 1 or none;
 *   verdict      0 ok: d == h; 1 flip: d == 1 - h; 2 undecided: n_used >= 1 and
 *                no decision; 255 not scored: tag not 0 / 1, or n_used == 0. */
#define PF_TAGCHECK_OK 0
#define PF_TAGCHECK_FLIP 1
#define PF_TAGCHECK_UNDECIDED 2
#define PF_TAGCHECK_NOT_SCORED 255
typedef struct pf_tagcheck {
    uint32_t n_windows;
    uint32_t n_reads;
    const uint32_t *win_read_off;  /* [n_windows+1] the batch's reads per window        */
    const uint32_t *n_used;    /* [n_reads] 0 for reads that are not scored          */
    const int64_t  *llr;       /* [n_reads] S, Q16; 0 for reads that are not scored  */
    const uint8_t  *verdict;   /* [n_reads] PF_TAGCHECK_*                            */
    const uint8_t  *hp;        /* [n_reads] the tags the call ran under: the batch's
                                  or read_hp (the writer's hp column)                */
    const uint32_t *win_n;     /* [n_windows*8] for tag 0, then tag 1: the window's
                                  reads with that tag, those with n_used >= 1, ok,
                                  flip                                               */
    float ms_kernels;          /* event-timed: the tag-check kernels only (the site
                                  table's pileup kernels are not part of it)         */
} pf_tagcheck_t;
/* Batches, tags, errors and ownership as in pf_batch_assign (read_hp NULL: the
 * batch's own tags; n_hp other than the batch's reads: PF_ERR_ARG; a count past
 * 65,535 in the pileup: PF_ERR_LIMIT; pf_tagcheck_free).  The result depends on
 * neither the tile, the workgroup size nor atomic order.  PF_TAGCHECK_TILE=<n>
 * in the environment (tests) sets the sites per LDS tile, a power of two in
 * [64, 2048]; the default is 2,048; any other value returns PF_ERR_ARG. */
int  pf_batch_tagcheck(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, const pf_assign_cfg_t *cfg,
                       pf_tagcheck_t **out);
void pf_tagcheck_free(pf_tagcheck_t *t);
/* The four weights of a site with the counts m1, u1, m2, u2 (host; the kernels
 * compute the same): w = wM0, wU0, wM1, wU1, usable[h] the flag of tag h; the
 * weights of a tag that is not usable, and of a category whose count is 0, are
 * 0.  A count above 65,535 is no pileup count and is taken as 65,535, as
 * pf_assign_site_weights does, so that L's arguments stay in range. */
void pf_tagcheck_site_weights(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2, uint32_t min_cov, int32_t w[4],
                              uint8_t usable[2]);

/* -u pre-pass: hp_out[r] in {0, 1, 254} for every read of one contig. */
int  pf_haptag_reads(pf_ctx_t *ctx, const pf_known_vars_t *known,
                     const pf_read_aln_batch_t *reads, uint8_t *hp_out);

/* Device self-test of what the kernels rely on for bit parity: the greedy
 * kernel's reciprocal-based division of 16-bit counts against the correctly
 * rounded fp32 division over all 2^32 operand pairs, and the DPP/permlane
 * wave scans and reductions against LDS references.  Writes the number of
 * mismatches (0 expected). */
int  pf_selftest(pf_ctx_t *ctx, uint64_t *mismatches);

/* Device BGZF inflate (the decompression of htslib's bgzf_read_block,
 * bgzf.c, which load_reads_given_interval reaches through sam_itr_next at
 * blockjoin.c:1076): every BGZF block of comp[0, comp_len) (whole blocks,
 * concatenated as in a BAM file) is inflated on the device, one wavefront per
 * block, and its CRC32 and ISIZE checked; the output (blocks back to back) is
 * copied to out.  block_status[i] (when given, i < status_cap) receives block
 * i's PF_INF_* code (pf_ingest.h; 0 = ok); kernel_ms the inflate kernel time.
 * PF_ERR_ARG for a malformed block table, an undersized out, or any block
 * that failed. */
int  pf_bgzf_inflate(pf_ctx_t *ctx, const uint8_t *comp, uint64_t comp_len, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_len, uint32_t *block_status, uint32_t status_cap, float *kernel_ms);

/* ------------------------------------------------------------------ */
/* Window definition (host side).                                      */

/* Phase-block gaps of a phased VCF, per contig in VCF order.  raw_* are the
 * gaps as insert_vcf_line collects them (blockjoin.c:1348-1430, driven by
 * load_intervals_from_file, :1977-2170): [last POS of a block, PS of the next
 * block]; gap_* are the windows the methphase worker receives after
 * merge_close_intervals(readback) (:2190-2220, called with READBACK at
 * :4520-4521); drop_* the phased intervals that merging swallowed.  Slices of
 * contig c: [x_off[c], x_off[c+1]). */
typedef struct pf_gaps {
    uint32_t n_contigs;
    char **names;
    uint32_t *abs_start, *abs_end;     /* ranges_t.abs_start / abs_end */
    uint64_t *raw_off, *gap_off, *drop_off;
    uint32_t *raw_start, *raw_end;
    uint32_t *gap_start, *gap_end;
    uint32_t *drop_start, *drop_end;
} pf_gaps_t;

/* Parse a (bgzipped or plain) VCF.  Lines starting with '#' are skipped, as
 * load_intervals_from_file does (:2023-2026).  Returns PF_OK, PF_ERR_ARG for
 * the reference's fatal input error (a POS below the previous one,
 * :1383-1387), PF_ERR_NOMEM, or -1 when the file cannot be read. */
int  pf_vcf_gaps(const char *vcf_path, int32_t readback, pf_gaps_t **out);
/* The same loader for any phase-block file main_blockjoin accepts
 * (blockjoin.c:4661-4666: --tsv, then --gtf, then --vcf): PF_INTERVALS_VCF
 * (PS blocks, as pf_vcf_gaps), PF_INTERVALS_GTF (block = GTF columns 4/5) or
 * PF_INTERVALS_TSV (columns 2/3 of "chrom start end"), through insert_gtf_line
 * (:1305-1345): a gap is [end of a block, start of the next block], the first
 * block of each contig sets its abs_start (prev_end resets per new contig,
 * :2098).  Plain or gzipped. */
#define PF_INTERVALS_VCF 0
#define PF_INTERVALS_GTF 1
#define PF_INTERVALS_TSV 2
int  pf_interval_gaps(const char *path, int32_t format, int32_t readback, pf_gaps_t **out);
void pf_gaps_free(pf_gaps_t *gaps);

/* `pomfret report` chunk windows of one contig (main_methreport,
 * blockjoin.c:4963-4991) from its raw gaps: writes up to cap windows
 * [win_start, win_end) and returns how many there are (or < 0). */
int64_t pf_report_windows(uint32_t abs_start, const uint32_t *gap_start, const uint32_t *gap_end,
                          uint64_t n_gaps, uint32_t chunk_size, uint32_t chunk_stride,
                          uint32_t *win_start, uint32_t *win_end, uint64_t cap);

/* ------------------------------------------------------------------ */
/* Output epilogue (host side): decisions -> phase blocks -> GTF/TSV/VCF. */

/* Per contig (slices [x_off[c], x_off[c+1])): the raw gaps after
 * lift_decisions fused the joined ones (rawunphasedblocks, blockjoin.c:
 * 2250-2310), one decision and one cumulative flip per raw gap
 * (decisions_onraw / flips_onraw, :2312-2324), and the new phase blocks
 * [blk_start, blk_end) of generate_new_phase_blocks(use_raw=1) (:2326-2362). */
typedef struct pf_blocks {
    uint32_t n_contigs;
    uint64_t *raw_off, *dec_off, *blk_off;
    uint32_t *raw_start, *raw_end;
    int32_t *dec_onraw, *flip;
    uint32_t *blk_start, *blk_end;
} pf_blocks_t;

/* decision[] holds one join decision (-1 none, 0 cis, 1 trans; the
 * pf_window_out_t.decision of each window) per merged gap of g, contig by
 * contig in g's order (the windows gap_*[gap_off[c] ...]).  Replaces the
 * three calls at blockjoin.c:4685-4687. */
int  pf_phase_blocks(const pf_gaps_t *g, const int8_t *decision, pf_blocks_t **out);
void pf_blocks_free(pf_blocks_t *b);

/* output_gtf (:2721-2756) / output_tsv (:2696-2719) to a file path. */
int  pf_write_gtf(const pf_gaps_t *g, const pf_blocks_t *b, const char *path);
int  pf_write_tsv(const pf_gaps_t *g, const pf_blocks_t *b, const char *path);

/* Phase of the REF allele at variant sites inside dropped intervals
 * (st->varphase_in_dropped of recover_variant_phase_in_dropped_intervals,
 * :2618-2694), per contig of g: 0-based positions ascending in
 * [off[c], off[c+1]), hap_of_ref 0, 1 or 254 (unphased). */
typedef struct pf_rescue {
    const uint64_t *off;
    const uint32_t *pos;
    const uint8_t *hap_of_ref;
} pf_rescue_t;

/* output_modify_vcf (:2918-2988) / alter_vcf_line (:2758-2916): rewrite
 * vcf_in (bgzipped or plain) into vcf_out (plain text) with the new PS and
 * flipped GTs.  rescue may be NULL (no rescued sites).  counts (optional):
 * {lines rewritten, lines unphased by the rescue, lines read}.  Returns
 * PF_OK, PF_ERR_ARG for a #CHROM header without 10 columns, PF_ERR_NOMEM,
 * or -1 on an I/O error. */
int  pf_write_vcf(const char *vcf_in, const pf_gaps_t *g, const pf_blocks_t *b, const pf_rescue_t *rescue,
                  const char *vcf_out, int64_t *counts);

/* ------------------------------------------------------------------ */
/* BAM ingest on the host: BGZF + BAM + BAI reader and  */
/* the region fetch of load_reads_given_interval, feeding pf_aln_batch_t. */

typedef struct pf_bam pf_bam_t;

/* Open a BAM and its BAI (bai_path NULL: bam_path + ".bai", then the path
 * with ".bam" replaced by ".bai").  bam_path NULL opens the index alone
 * (pf_bam_index_stats only).  Replaces hts_open + sam_index_load +
 * sam_hdr_read of init_and_open_bamfile_t (blockjoin.c:565-585).  Returns
 * PF_OK, PF_ERR_ARG (not a BAM / BAI, truncated), PF_ERR_NOMEM, or -1 when a
 * file cannot be opened. */
int  pf_bam_open(const char *bam_path, const char *bai_path, pf_bam_t **out);
void pf_bam_close(pf_bam_t *bam);
/* The host BGZF reader's block decoder: 1 = libdeflate (loaded at run time,
 * as htslib links it), 0 = zlib (libdeflate absent, or PF_HOST_ZLIB set in
 * the environment before the first block).  Diagnostics only. */
int  pf_host_inflater(void);
int32_t pf_bam_n_targets(const pf_bam_t *bam);
const char *pf_bam_target_name(const pf_bam_t *bam, int32_t tid);
uint32_t pf_bam_target_len(const pf_bam_t *bam, int32_t tid);
int32_t pf_bam_tid(const pf_bam_t *bam, const char *name);   /* -1 when absent */
/* The index's per-reference metadata pseudo-bin: mapped / unmapped counts
 * (hts_idx_get_stat); PF_ERR_ARG when tid has none. */
int  pf_bam_index_stats(const pf_bam_t *bam, int32_t tid, uint64_t *n_mapped, uint64_t *n_unmapped);
const char *pf_bam_path(const pf_bam_t *bam);
/* The index's count of unplaced records (the optional n_no_coor after the
 * references); -1 when the index does not have one. */
int64_t pf_bam_n_no_coor(const pf_bam_t *bam);
/* The BAI chunks [u, v) (virtual offsets) of region [beg, end) of tid, sorted
 * by u, as hts_itr_query collects them (bins overlapping the region, chunks
 * ending before the linear-index offset dropped).  Writes min(n, cap) pairs
 * u, v to uv; returns n or a negative PF_ERR. */
int64_t pf_bam_query_chunks(const pf_bam_t *bam, int32_t tid, int64_t beg, int64_t end, uint64_t *uv, uint64_t cap);

/* The records of a set of windows of one contig, in window order and BAM
 * order inside a window, as pf_aln_batch_t (owned by this struct) plus the
 * qnames (for the first-wins tag table, blockjoin.c:4408-4423). */
typedef struct pf_bam_records {
    pf_aln_batch_t aln;
    const uint64_t *qname_off;     /* [n_recs+1] into qname, no terminators */
    const char *qname;
    const int32_t *hp_tag;         /* [n_recs] raw HP value, INT32_MIN when absent */
    uint64_t n_truncated;          /* windows whose fetch stopped at a record
                                      htslib refuses (CIGAR/SEQ length mismatch) */
} pf_bam_records_t;

/* For window w the records sam_itr_querys(chrom:b-(e+readback)) yields,
 * b = s-readback clipped at 0, as load_reads_given_interval builds the
 * region (1053-1054); HP as get_hp_from_aln (910-923: absent or 0 -> 254,
 * else HP-1); de as bam_aux2f or -1; MM from MM:Z / Mm:Z, ML from ML:B:C /
 * Ml:B:C (a tag of another type makes the record's MM empty: htslib's
 * bam_parse_basemod fails and the read carries no calls); the CIGAR from a
 * CG:B:I tag when the record holds the kSmN placeholder.  win_start/win_end
 * are copied into aln.  n_threads > 1 fetches windows in parallel (one file
 * handle per thread).  Returns PF_OK, PF_ERR_ARG (unknown contig, corrupt
 * file), PF_ERR_NOMEM, or -1 on an I/O error. */
int  pf_bam_fetch_windows(pf_bam_t *bam, const char *chrom, uint32_t n_windows, const uint32_t *win_start,
                          const uint32_t *win_end, uint32_t readback, int n_threads, pf_bam_records_t **out);
void pf_bam_records_free(pf_bam_records_t *recs);

/* Device fetch: the same records as pf_bam_fetch_windows, but the host only
 * plans the fetch from the BAI and reads the compressed bytes of the blocks
 * the windows' index chunks touch; the device inflates them (pf_bgzf_inflate's
 * kernels), walks the record chain, decodes every record (rec_decode,
 * bam_tag2cigar, bam_endpos, the aux tags), runs each window's chunk walk
 * (sam_itr_next, with the overlap rule pos + rlen > beg and the stops at
 * another tid, pos >= end, a truncated record or EOF), and gathers the
 * returned records into a record-level batch (pf_batch_upload_aln's layout)
 * -- the record fields never cross PCIe.  Windows with more than
 * max_win_recs records (0 = no limit) are left empty.  *out is the batch
 * (pf_methphase_run etc.), *fetch the qnames and statistics (free with
 * pf_bam_dev_fetch_free). */
typedef struct pf_bam_dev_fetch {
    uint32_t n_windows;
    uint64_t n_recs;               /* records in the batch                               */
    const uint32_t *win_rec_off;   /* [n_windows+1] the batch's records per window       */
    const uint32_t *win_n_fetched; /* [n_windows] records the fetch returned (before the limit) */
    const uint64_t *qname_off;     /* [n_recs+1] into qname                              */
    const char *qname;
    const int32_t *hp_tag;         /* [n_recs] raw HP value, INT32_MIN when absent       */
    uint64_t n_truncated;          /* windows ended at a CIGAR/SEQ length mismatch       */
    uint64_t comp_bytes, inflated_bytes, n_blocks, n_chain_recs;
    double ms_read, ms_inflate, ms_chain, ms_decode, ms_select, ms_build, ms_total;
    uint32_t attempts;             /* plans tried (a record past the planned blocks widens the plan) */
    const uint8_t *read_hp;        /* pf_haptag_bam: [n_recs] each read's tag (NULL otherwise)  */
    uint32_t from_arena;           /* 1: the blocks came from a kept -u arena (nothing read or inflated) */
} pf_bam_dev_fetch_t;
/* replace a record-level batch's per-record HP values (the -u table's tags,
 * blockjoin.c:1114-1122); n must equal its record count */
int  pf_batch_set_hp(pf_dbatch_t *db, const uint8_t *hp, uint32_t n);
int  pf_batch_upload_bam(pf_ctx_t *ctx, const pf_cfg_t *cfg, const pf_load_cfg_t *lcfg, pf_bam_t *bam,
                         const char *chrom, uint32_t n_windows, const uint32_t *win_start, const uint32_t *win_end,
                         uint32_t readback, uint32_t max_win_recs, pf_dbatch_t **out, pf_bam_dev_fetch_t **fetch);
void pf_bam_dev_fetch_free(pf_bam_dev_fetch_t *fetch);
/* The -u pre-pass with the device fetch: the reads pf_bam_fetch_contig_reads
 * returns (the whole contig, primary mapped, MD:Z required unless a
 * reference is attached: PF_ERR_ARG otherwise) inflated, selected and gathered on the device and haptagged there
 * by K4 against `known` (pf_haptag_reads' semantics).  *fetch holds n_recs
 * reads in BAM order: read_hp, qnames. */
int  pf_haptag_bam(pf_ctx_t *ctx, const pf_known_vars_t *known, pf_bam_t *bam, const char *chrom,
                   pf_bam_dev_fetch_t **fetch);
/* the same with the contig's coverage estimate (estimate_read_coverage_dirtyfast,
 * 951-1040) from the same whole-contig fetch: every record is selected, the
 * primary mapped ones are haplotagged; *truncated is set when a truncated
 * record ended the pass (the serial estimate stops there).  Used by the driver
 * for `methphase -u` without -c: one pass over each contig instead of two. */
int  pf_haptag_bam_cov(pf_ctx_t *ctx, const pf_known_vars_t *known, pf_bam_t *bam, const char *chrom,
                       pf_bam_dev_fetch_t **fetch_out, int32_t *cov, int32_t *truncated);
/* Both with the contig's position pieces given: n_bounds strictly increasing
 * positions > 0 split [0, HTS_POS_MAX) into n_bounds + 1 pieces (a read is
 * taken in the piece its start falls in; the reads, tags and order are the
 * one-piece fetch's).  fetch_ends (optional, fetch_ends[k] >= bounds[k]):
 * piece k fetches the region [bounds[k-1], fetch_ends[k]) -- reaching past
 * its bound over the windows that start in it -- while its reads stay those
 * starting before bounds[k].  With the fetch cache on (a -u pre-pass that
 * keeps its arenas) every piece's arena is kept, and a later window fetch of
 * the contig is served by the piece whose fetch region holds all its
 * windows.  cov / truncated NULL: no coverage estimate.  The driver places
 * the bounds between its windows' fetch regions where it can
 * (pf_pipeline.c). */
int  pf_haptag_bam_pieces(pf_ctx_t *ctx, const pf_known_vars_t *known, pf_bam_t *bam, const char *chrom,
                          uint32_t n_bounds, const int64_t *bounds, const int64_t *fetch_ends,
                          pf_bam_dev_fetch_t **fetch_out, int32_t *cov, int32_t *truncated);
/* The pieces the -u pre-pass fetches a contig in by default: K =
 * ceil(compressed bytes of the contig's index chunks / piece_bytes) (0: the
 * PF_FETCH_PIECE_BYTES variable or 4 GiB), each *step bases long. */
uint64_t pf_bam_contig_pieces(pf_bam_t *bam, int32_t tid, uint64_t piece_bytes, int64_t *step);


/* The -u pre-pass reads of one contig (pre_haplotagging_read_in_one_ref,
 * 1841-1898: sam_itr_querys over the whole contig, flags 4/256/2048
 * skipped), in BAM order, as pf_haptag_reads takes them, plus qnames for
 * its first-wins table.  A primary mapped record without MD:Z returns
 * PF_ERR_ARG (the reference asserts, 1594-1595) unless a reference is attached
 * (pf_bam_set_ref: every record's MD is then synthesised, its tag ignored). */
typedef struct pf_bam_reads {
    pf_read_aln_batch_t reads;
    const uint64_t *qname_off;     /* [n_reads+1] */
    const char *qname;
    uint64_t n_truncated;          /* 1 when the fetch stopped at a record htslib refuses */
} pf_bam_reads_t;
int  pf_bam_fetch_contig_reads(pf_bam_t *bam, const char *chrom, pf_bam_reads_t **out);
void pf_bam_reads_free(pf_bam_reads_t *reads);

/* Per-contig read coverage estimate for runs without -c
 * (estimate_read_coverage_dirtyfast, 951-1040): covs[tid] for
 * tid < pf_bam_n_targets (n >= that).  A full sequential pass over the BAM. */
int  pf_bam_estimate_coverage(pf_bam_t *bam, int32_t *covs, int32_t n);
/* BGZF inflate threads of the handle's sequential passes (the coverage
 * estimate and pf_bam_fetch_contig_reads): the reference's -t N, which sets
 * pomfret_n_bam_threads for bgzf_mt on every BAM it opens (cli.c:261-264,
 * blockjoin.c:576-578).  n <= 1: single-threaded (the default). */
void pf_bam_set_threads(pf_bam_t *bam, int n);
/* The same estimate with the BAM's records inflated, chained and decoded on
 * ctx's device (the device fetch, pieces of <= piece_bytes compressed bytes
 * per call; 0 = 4 GiB), contig by contig through the index; identical covs
 * for a coordinate-sorted, indexed BAM (the only kind the pipeline opens).
 * Falls back to pf_bam_estimate_coverage when the index has no unplaced-read
 * count (the last contig's estimate depends on it). */
int  pf_bam_estimate_coverage_dev(pf_ctx_t *ctx, pf_bam_t *bam, int32_t *covs, int32_t n, uint64_t piece_bytes);
/* one contig of that pass (0 without records; *truncated: the pass would stop here) */
int  pf_bam_estimate_contig_dev(pf_ctx_t *ctx, pf_bam_t *bam, int32_t tid, int32_t *cov, int32_t *truncated);


/* ------------------------------------------------------------------ */
/* MD synthesis from a reference FASTA (DESIGN.md "MD synthesis"): for  */
/* BAMs whose records carry no MD:Z.                                     */

/* The FASTA, read once front to back (plain or gzipped; no .fai / BGZF
 * random access).  A name runs from '>' to the first whitespace; in the
 * sequence all whitespace is dropped, case folded, A C G T -> 1 2 4 8, U -> 8,
 * every other byte -> 15 (N).  PF_ERR_ARG for a duplicate name or sequence
 * before the first header, -1 when the file cannot be read. */
typedef struct pf_ref pf_ref_t;
int  pf_ref_open(const char *path, pf_ref_t **out);
uint32_t pf_ref_n(const pf_ref_t *ref);
const char *pf_ref_name(const pf_ref_t *ref, uint32_t i);
/* contig `name`: its packed nibbles, high nibble first as BAM SEQ is packed
 * ((len + 1) / 2 bytes, valid until pf_ref_free), and its length in bases;
 * PF_ERR_ARG when absent */
int  pf_ref_contig(const pf_ref_t *ref, const char *name, const uint8_t **nib, uint64_t *len);
void pf_ref_free(pf_ref_t *ref);

/* Attach a reference to a BAM handle (NULL detaches; the handle does not own
 * it).  PF_ERR_ARG when a BAM target is present in the FASTA with another
 * length; a target absent from the FASTA is an error only when a record on it
 * needs its MD.  With a reference attached pf_haptag_bam, _cov, _pieces,
 * pf_bam_fetch_contig_reads and pf_rescue_dropped, _mt, _multi synthesise the
 * MD of every record they would have read MD:Z from and ignore the tags. */
int  pf_bam_set_ref(pf_bam_t *bam, const pf_ref_t *ref);
/* target tid's nibbles in the attached reference: 1 and (*nib, *len), 0 when
 * no reference is attached, PF_ERR_ARG when the FASTA lacks the target */
int  pf_bam_ref_contig(const pf_bam_t *bam, int32_t tid, const uint8_t **nib, uint64_t *len);

/* The MD rule on the host: md_off[n_reads + 1] and the MD bytes of every read
 * of `reads` against the contig's nibbles (reads->md and md_off are ignored).
 * PF_ERR_ARG when an M/=/X/D op reaches past ref_len.  Free with pf_md_free. */
int  pf_md_synth_host(const pf_read_aln_batch_t *reads, const uint8_t *ref_nib, uint64_t ref_len, uint64_t **md_off,
                      uint8_t **md);
void pf_md_free(uint64_t *md_off, uint8_t *md);
/* The same bytes from the device kernels (pf_k4_mdlen, pf_k4_mdfill), copied
 * back: for tests and callers that want the tag.  ref_len < 2^32. */
int  pf_md_synth(pf_ctx_t *ctx, const pf_read_aln_batch_t *reads, const uint8_t *ref_nib, uint64_t ref_len,
                 uint64_t **md_off, uint8_t **md);
/* pf_haptag_reads on the synthesised MD, which never leaves the device */
int  pf_haptag_reads_ref(pf_ctx_t *ctx, const pf_known_vars_t *known, const pf_read_aln_batch_t *reads,
                         const uint8_t *ref_nib, uint64_t ref_len, uint8_t *hp_out);
/* measurement hook: the context's MD synthesis so far -- reference bytes
 * uploaded, reads synthesised, MD bytes written, and the two kernels' summed
 * times */
typedef struct pf_md_stats {
    uint64_t ref_upload_bytes, n_reads, md_bytes;
    double ms_len, ms_fill;
} pf_md_stats_t;
int  pf_ctx_md_stats(const pf_ctx_t *ctx, pf_md_stats_t *out);

/* qname -> tag table across the boundary (first entry of a qname wins). */
typedef struct pf_qname_tags {
    uint32_t n;
    const uint64_t *off;           /* [n+1] into names */
    const char *names;
    const uint8_t *hp;
} pf_qname_tags_t;

/* VCF-writer rescue map of one contig: recover_variant_phase_in_dropped_
 * intervals (2618-2694) / recover_variant_phase_in_one_interval (2475-2616).
 * For each dropped interval [s, e] in order: the known positions in
 * [s-1, e+1); the records of region "chrom:(s-1)-(e+1)" whose qname is in
 * `methphased` (st->qname2haptag) and whose raw tag (`raw` table when given
 * -- the -u table -- else the HP tag) is not unphased; their variant
 * positions (CIGAR I, MD mismatches and closed ^-runs) voted by methphased
 * tag 0/1 at each known position: more hap0 -> REF on hap1, more hap1 ->
 * REF on hap0, else 254.  A known position sorted last among the interval's
 * entries gets no vote (the loop stops at n-1).  Positions ascending, last
 * write wins.  PF_ERR_ARG for an MD-less selected record (the reference
 * asserts) unless a reference is attached (pf_bam_set_ref), or an invalid MD
 * character (it exits). */
typedef struct pf_rescue_map {
    uint32_t n;
    const uint32_t *pos;
    const uint8_t *hap_of_ref;
} pf_rescue_map_t;
int  pf_rescue_dropped(pf_bam_t *bam, const char *chrom, uint32_t n_drop, const uint32_t *drop_start,
                       const uint32_t *drop_end, const pf_known_vars_t *known, const pf_qname_tags_t *methphased,
                       const pf_qname_tags_t *raw, pf_rescue_map_t **out);
/* the same with the intervals spread over `threads` host threads (each with
 * its own file handle); the result is the serial pass's */
int  pf_rescue_dropped_mt(pf_bam_t *bam, const char *chrom, uint32_t n_drop, const uint32_t *drop_start,
                          const uint32_t *drop_end, const pf_known_vars_t *known, const pf_qname_tags_t *methphased,
                          const pf_qname_tags_t *raw, int threads, pf_rescue_map_t **out);
/* several contigs at once (the qname tables built once, every (contig,
 * interval) one work item); out[c] per contig, each the serial pass's */
int  pf_rescue_dropped_multi(pf_bam_t *bam, uint32_t n_contigs, const char *const *chroms, const uint32_t *n_drop,
                             const uint32_t *const *drop_start, const uint32_t *const *drop_end,
                             const pf_known_vars_t *const *known, const pf_qname_tags_t *methphased,
                             const pf_qname_tags_t *raw, int threads, pf_rescue_map_t **out);
void pf_rescue_map_free(pf_rescue_map_t *map);

/* -u known variants of one contig: insert_variant_from_vcf_line (1432-1543)
 * on every complete line whose CHROM equals `contig` (the variants the
 * reference collects for a contig before pre-haplotagging its reads,
 * 1937-1941, 2069-2080): GT "a|b" with a, b in {0,1}; SNP -> X at POS-1;
 * ref longer -> D at POS (len ref-alt, chars ref+1); alt longer -> I at
 * POS-1 (len alt-ref, chars alt+1); equal-length non-SNPs skipped; haptag =
 * GT[0].  Tokens split on runs of tabs as strtok_r does; '#' lines skipped
 * (:2023-2026).  Returns PF_OK, PF_ERR_NOMEM, or -1 when the file cannot be
 * read. */
typedef struct pf_known_table {
    pf_known_vars_t vars;
} pf_known_table_t;
int  pf_vcf_known_vars(const char *vcf_path, const char *contig, pf_known_table_t **out);
/* The tables recover_variant_phase_in_dropped_intervals builds for the run's
 * contigs (names: the phase-block file's contigs) in one pass over the VCF:
 * the var_storage branch of load_intervals_from_file (2150-2163), where a
 * line whose CHROM is not among `names` goes to the table the previous line
 * went to (skipped before the first match).  With the VCF's own contigs as
 * `names` (no --gtf / --tsv) out[c] equals pf_vcf_known_vars(names[c]).
 * out[0..n) are set on PF_OK (free each with pf_known_table_free). */
int  pf_vcf_known_vars_multi(const char *vcf_path, uint32_t n, const char *const *names, pf_known_table_t **out);
void pf_known_table_free(pf_known_table_t *t);

/* A host mask: per contig of `names` the sorted unique masked positions
 * (pf_batch_set_mask), the union of
 *   bed_path: lines `chrom start end` (tab or space separated, 0-based
 *     half-open, plain or gzipped, read like --tsv: a trailing line without
 *     its newline is dropped); '#' and empty lines skipped, contigs not in
 *     `names` ignored, start >= end empty; unsorted, overlapping and
 *     duplicate intervals allowed; a line with fewer than three columns or a
 *     non-numeric bound is PF_ERR_ARG;
 *   vcf_path: [pos, pos+len) of every variant of each contig's known-variant
 *     table (pf_vcf_known_vars_multi with the same names), the set
 *     main_methreport builds (blockjoin.c:5006-5029).
 * Either path may be NULL.  A position >= 2^29 is PF_ERR_LIMIT; a file that
 * cannot be read -1. */
typedef struct pf_mask pf_mask_t;
int  pf_mask_load(const char *bed_path, const char *vcf_path, uint32_t n_contigs, const char *const *names,
                  pf_mask_t **out);
/* contig c's positions (valid until pf_mask_free); *pos is NULL when *n is 0 */
int  pf_mask_contig(const pf_mask_t *mask, uint32_t c, const uint32_t **pos, uint64_t *n);
void pf_mask_free(pf_mask_t *mask);

/* ------------------------------------------------------------------ */
/* qname -> haplotag tables (the reference's htstri_t: st->qname2haptag,  */
/* st->qname2haptag_raw), first entry of a qname wins.                    */

typedef struct pf_tags pf_tags_t;
pf_tags_t *pf_tags_new(void);
void     pf_tags_free(pf_tags_t *t);
uint64_t pf_tags_size(const pf_tags_t *t);
/* Insert every (names[off[i]:off[i+1]], hp[i]) whose qname is absent, in
 * order (kh_put + "if (absent)", blockjoin.c:4412-4421).  Returns the number
 * inserted or < 0. */
int64_t  pf_tags_put_first(pf_tags_t *t, uint32_t n, const uint64_t *off, const char *names, const uint8_t *hp);
/* hp_out[i] = tag of qname i, or dflt when absent; returns how many were found. */
int64_t  pf_tags_get(const pf_tags_t *t, uint32_t n, const uint64_t *off, const char *names, uint8_t dflt,
                     uint8_t *hp_out);
/* The entries in insertion order (valid until the next insertion). */
int      pf_tags_view(const pf_tags_t *t, pf_qname_tags_t *out);

/* ------------------------------------------------------------------ */
/* Pipeline driver: `pomfret methphase` (main_blockjoin, blockjoin.c:    */
/* 4643-4736) and `pomfret report` (main_methreport, 4901-5089) from     */
/* files, on one or more GPUs.                                           */

#define PF_READBACK 50000          /* blockjoin.c READBACK, the fetch margin of 1053-1054 */
#define PF_MODE_METHPHASE 0
#define PF_MODE_REPORT    1
#define PF_MODE_VARHAPTAG 2        /* pf_methphase_main only: out_prefix is the output BAM path */
#define PF_JOB_WINDOWS 0           /* a run of consecutive windows of one contig */
#define PF_JOB_HAPTAG  1           /* the -u pre-pass of one contig (1841-1898) */

typedef struct pf_methphase_opts {
    int32_t mode;                  /* PF_MODE_*                                                */
    const char *bam_path;          /* positional bam (sorted, indexed)                         */
    const char *vcf_path;          /* --vcf                                                    */
    const char *out_prefix;        /* -o; NULL: nothing written                                */
    /* methphase: cliopt->cov_for_selection / n_candidates_per_iter as the
     * CLI leaves them (-c C sets C/10 and C/4, -n sets n_cand; <= 0: per
     * contig from the coverage estimate, 4357-4374); cov_for_runtime <= 0
     * means 2*cov_for_selection (4655).  report: cov is -c (<= 0: the
     * estimate), parameters cov/10+1, 2x, cov/4+1 (5045-5051). */
    int32_t cov_for_selection, cov_for_runtime, n_cand, cov;
    int32_t k, k_span;             /* -k, -l (<= 0: 3, 5000)                                   */
    pf_load_cfg_t load;            /* -q, -L, --lo, --hi                                       */
    int32_t untagged;              /* -u, --bam-is-untagged                                    */
    int32_t write_tsv;             /* --output-tsv: {prefix}.mp.tsv                            */
    int32_t write_bam;             /* --write-bam: {prefix}.mp.bam + .bai (varhaptag: the BAM) */
    int32_t chunk_size, chunk_stride;  /* report: --chunk-size, --chunk-stride                 */
    int32_t threads;               /* host threads fetching one job's windows (-t)             */
    int32_t n_devices;             /* GPUs to drive from this process (0: all visible)         */
    const int32_t *devices;        /* their ids (NULL: 0..n_devices-1)                         */
    pf_ctx_t *const *ctxs;         /* or caller-owned contexts, one per device thread          */
    int32_t n_ctxs;
    int32_t rank, world;           /* multi-process runs: this process runs the jobs the static
                                      LPT partition gives `rank` (world <= 1: all of them)      */
    uint32_t job_windows;          /* max windows per job (0: 1024)                            */
    int32_t verbose;               /* < 0: no progress messages                                */
    int32_t host_fetch;            /* 1: records fetched and decoded on the host (pf_bam_fetch_windows
                                      + pf_batch_upload_aln); 0: the device fetch (pf_batch_upload_bam) */
    /* --tsv / --gtf phase blocks (main_blockjoin 4661-4666: tsv, then gtf,
     * then vcf).  NULL or PF_INTERVALS_VCF: the VCF's PS blocks.  With -u the
     * VCF still names the contigs whose reads are pre-haplotagged (4446) and
     * the file replaces the intervals (4460-4465); without vcf_path (methphase
     * only, no -u) no VCF is written (4706). */
    const char *interval_path;
    int32_t interval_format;       /* PF_INTERVALS_GTF or PF_INTERVALS_TSV                     */
    int32_t write_input_tagging;   /* -U (with -u): {prefix}.mp.input_haptag.tsv (4494-4517)  */
    int32_t bam_threads;           /* -T / --bam-threads: --write-bam's BGZF compression threads
                                      (<= 0: `threads`, as -t sets threads_bam, cli.c:261-264)  */
    /* masked reference positions of the window jobs (methphase and report;
     * varhaptag ignores them): pf_mask_load(mask_path, mask_variants ?
     * vcf_path : NULL) over the windows' contigs, each job's batch given its
     * contig's positions (pf_batch_set_mask) */
    const char *mask_path;         /* --mask-bed: BED of positions no site may lie on (NULL: none) */
    int32_t mask_variants;         /* --mask-variants: also every phased variant's [pos, pos+len)
                                      of --vcf, the set main_methreport builds and leaves unused
                                      (blockjoin.c:5006-5029, 4250-4251); needs vcf_path         */
    const char *ref_path;          /* --ref: reference FASTA (plain or gzipped; NULL: none).  Every
                                      BAM handle of the run gets it attached (pf_bam_set_ref): the -u
                                      pre-pass and the rescue synthesise MD and need no MD:Z tags */
} pf_methphase_opts_t;

typedef struct pf_mp_plan pf_mp_plan_t;

/* Whole run in this process: plan, (-u) pre-pass jobs on the devices, window
 * jobs on the devices (one host thread per GPU; the next job's BAM fetch
 * overlaps the current job's kernels), merge and outputs:
 * {prefix}.mp.gtf, .mp.vcf (and .mp.tsv, .mp.bam + .mp.bam.bai), or
 * {prefix}.report.tsv plus the running totals on stdout, or (varhaptag) the
 * -u pre-pass alone with {out}.varhaptag.tsv and the retagged {out} + .bai.  On success *out holds the finished plan
 * (decisions, tables, blocks) until pf_mp_free. */
int  pf_methphase_main(const pf_methphase_opts_t *o, pf_mp_plan_t **out);

/* The same run split into steps, for one process per GPU: every rank builds
 * the same plan (deterministic), runs its jobs, exports their results; the
 * writer rank imports every rank's results and finishes. */
int  pf_mp_plan(const pf_methphase_opts_t *o, pf_mp_plan_t **out);
void pf_mp_free(pf_mp_plan_t *p);
uint32_t pf_mp_n_jobs(const pf_mp_plan_t *p, int kind);

typedef struct pf_mp_job_info {
    uint32_t contig;               /* index into the plan's gaps                    */
    const char *contig_name;
    uint32_t w0, w1;               /* windows [w0, w1) of pf_mp_windows             */
    int32_t rank;                  /* static LPT owner                              */
    uint32_t lpt_pos;              /* position in the longest-first order           */
    double cost;                   /* fetch span (bases) / contig length (-u)       */
    int32_t done;
    pf_cfg_t cfg;                  /* the contig's parameters (4357-4390)           */
} pf_mp_job_info_t;
int  pf_mp_job_info(const pf_mp_plan_t *p, int kind, uint32_t j, pf_mp_job_info_t *info);
/* All windows in (contig, window) order; contig c owns [off[c], off[c+1]). */
int  pf_mp_windows(const pf_mp_plan_t *p, const uint32_t **win_start, const uint32_t **win_end,
                   const uint64_t **contig_win_off, uint32_t *n_windows);

/* Run jobs of `kind` owned by run_opts->rank (all when world <= 1) on the
 * devices run_opts names (n_devices / devices / ctxs). */
int  pf_mp_run_mine(pf_mp_plan_t *p, const pf_methphase_opts_t *run_opts, int kind);
int  pf_mp_run_job(pf_mp_plan_t *p, pf_ctx_t *ctx, uint32_t j);          /* one window job */
int  pf_mp_run_haptag_job(pf_mp_plan_t *p, pf_ctx_t *ctx, uint32_t j);   /* one -u job     */
/* After every -u job has a result: the merged table (contig order, first
 * wins) that replaces HP in the window jobs (1114-1122). */
int  pf_mp_merge_raw(pf_mp_plan_t *p);

/* A job's result: decisions of its windows and the (qname, tag) entries of
 * its joined windows, window by window in read order (tag_off[w] ..
 * tag_off[w+1]); -u jobs: no windows, the contig's first-wins table in BAM
 * order.  get returns views into the plan; set copies. */
typedef struct pf_mp_job_result {
    uint32_t n_windows;
    const int8_t *decision;
    const uint64_t *tag_off;
    pf_qname_tags_t tags;
    uint32_t n_limit;              /* windows left undecided for a device limit */
} pf_mp_job_result_t;
int  pf_mp_get_job_result(const pf_mp_plan_t *p, int kind, uint32_t j, pf_mp_job_result_t *r);
int  pf_mp_set_job_result(pf_mp_plan_t *p, int kind, uint32_t j, const pf_mp_job_result_t *r);

/* Merge every job's result in (contig, window) order -- decisions, and the
 * joined windows' tags first-wins (4408-4423 then 4579-4595) -- then the
 * phase blocks and, with an output prefix, the files. */
int  pf_mp_finish(pf_mp_plan_t *p);
int  pf_mp_decisions(const pf_mp_plan_t *p, const int8_t **decision, uint32_t *n, uint32_t *n_limit);
const pf_gaps_t   *pf_mp_gaps(const pf_mp_plan_t *p);
const pf_blocks_t *pf_mp_blocks(const pf_mp_plan_t *p);
const pf_tags_t   *pf_mp_qname_hp(const pf_mp_plan_t *p);
const pf_tags_t   *pf_mp_raw_hp(const pf_mp_plan_t *p);     /* NULL without -u */
/* report: {correct, switch, fail} */
int  pf_mp_report_counts(const pf_mp_plan_t *p, double *counts3);
/* The qualifying positions the mask removed (pf_batch_masked_sites summed over
 * the window jobs this process ran; 0 with no mask) */
int  pf_mp_masked_sites(const pf_mp_plan_t *p, uint64_t *total);
/* measurement hook: wall seconds per phase of the run and the device-fetch
 * sums (pf_bam_dev_fetch_t's ms_* and byte counts) of its jobs; index 0 =
 * window jobs, 1 = -u pre-pass jobs */
typedef struct pf_mp_stats {
    double s_plan;              /* VCF gaps, coverage estimate, job plan      */
    double s_estimate;          /* the coverage pass (inside s_plan)          */
    double s_haptag;            /* -u pre-pass jobs + the merge of their tables */
    double s_windows;           /* window jobs                                 */
    double s_finish;            /* first-wins merge, phase blocks, writers    */
    double fetch_ms[2][7];      /* read, inflate, chain, decode, select, build, total */
    uint64_t comp_bytes[2], inflated_bytes[2];
    double run_ms[2];           /* pf_methphase_run / K4 wall, summed over jobs */
    uint64_t n_fetch[2];        /* device fetches */
    /* window jobs of a run that keeps the -u pre-pass's arenas: fetches served
     * from a kept arena, fetches that read and inflated the file again (their
     * compressed bytes), and jobs a context took from another device's queue */
    uint64_t arena_hits, arena_misses, reread_bytes, steals;
} pf_mp_stats_t;
int  pf_mp_stats(const pf_mp_plan_t *p, pf_mp_stats_t *s);

/* ------------------------------------------------------------------ */
/* BAM output: --write-bam and varhaptag.                               */

#define PF_RETAG_METHPHASE 0       /* output_modify_bam (blockjoin.c:3022-3103)   */
#define PF_RETAG_VARHAPTAG 1       /* main_varhaptag (4737-4836)                  */
#define PF_RETAG_INPUT_HAPTAG 2    /* methphase -u -U: the TSV alone (4494-4517)  */

/* Every record of bam_in, in file order (sam_itr_querys "."), with HP set
 * to the new haplotag + 1 as bam_aux_update_int does it (an existing
 * integer HP keeps its size when the value fits, else it grows in place; a
 * missing HP is appended as the smallest integer type; a non-integer HP or
 * corrupt aux data leaves the record unchanged), written to bam_out (NULL:
 * none) with its BAI at bai_out (NULL: none; sam_index_build3 at 4723), and
 * for varhaptag one TSV line per record to tsv_out (NULL: none):
 * "#qname\thaptag_input\thaptag_new", then qname, HP-tag value, new + 1.
 *   PF_RETAG_METHPHASE: the raw tag is raw's (the -u table; absent:
 *     unphased) or the HP tag's (get_hp_from_aln); a qname in `methphased`
 *     (st->qname2haptag) takes its tag, a raw 0/1 otherwise; either is
 *     flipped when the phased interval the read starts in
 *     (check_if_in_phased_intervals over g's merged gaps) needs it -- the
 *     flip of blk's raw gap at the merged index - 1, carried over until the
 *     next interval is entered, across contigs too (get_flip_status_by_idx).
 *   PF_RETAG_VARHAPTAG: the new tag is raw's (absent: unphased).
 *   PF_RETAG_INPUT_HAPTAG: as VARHAPTAG with no BAM (bam_out must be NULL)
 *     and the -U header "#qname\treal_hp\ttagged_hp" ({prefix}.mp.input_haptag.tsv:
 *     the HP tag's value, the -u table's tag + 1 or 255).
 * level: zlib level (htslib's "w" mode: -1, Z_DEFAULT_COMPRESSION).
 * The iteration stops, as htslib's does, at a record whose CIGAR query
 * length differs from l_qseq.  *n_records: records processed. */
int  pf_retag_bam(const char *bam_in, const char *bam_out, const char *bai_out, const char *tsv_out, int mode,
                  const pf_gaps_t *g, const pf_blocks_t *blk, const pf_tags_t *methphased, const pf_tags_t *raw,
                  int level, uint64_t *n_records);
/* The same with `threads` BGZF compression threads for bam_out (-T /
 * --bam-threads: htslib's bgzf_mt for the output, cli.c:261-264, 3036):
 * blocks deflated in parallel, written in order; the BAM and BAI bytes do not
 * depend on the thread count. */
int  pf_retag_bam_threads(const char *bam_in, const char *bam_out, const char *bai_out, const char *tsv_out, int mode,
                          const pf_gaps_t *g, const pf_blocks_t *blk, const pf_tags_t *methphased,
                          const pf_tags_t *raw, int level, int threads, uint64_t *n_records);

/* ------------------------------------------------------------------ */
/* hapmeth: per-haplotype CpG methylation of a haplotagged BAM (no reference
 * counterpart).  Host only: the sites of windows [w0, w1) of a pileup as BED
 * lines, tab-separated:
 *   chrom start start+1 h1_meth h1_unmeth h2_meth h2_unmeth other_meth other_unmeth asm_p
 * start the 0-based position of the CpG's C (strands combined), asm_p the
 * two-sided pf_fisher_exact(h1_meth, h1_unmeth, h2_meth, h2_unmeth) as %.6g.
 * header != 0 creates (truncates) the file and writes the column names behind
 * a '#' first; header == 0 appends to it.  Returns PF_OK, PF_ERR_ARG, or -1
 * when the file cannot be written. */
int  pf_write_hapmeth(const char *path, const char *chrom, const pf_pileup_t *p, uint32_t w0, uint32_t w1, int header);

typedef struct pf_hapmeth_opts {
    const char *bam_path;      /* sorted, indexed, haplotagged (HP)                        */
    const char *out_prefix;    /* writes {out_prefix}.hapmeth.bed                          */
    const char *region;        /* NULL: every contig in header order; else chrom or
                                  chrom:beg-end, 1-based inclusive (samtools style)        */
    uint32_t chunk_size;       /* window (fetch unit) length in bases; 0 -> 100,000        */
    uint32_t job_windows;      /* windows per device job; 0 -> 1024                        */
    pf_load_cfg_t load;        /* K0's filters and ML bands                                */
    int32_t threads;           /* host threads of --host-fetch                             */
    int32_t host_fetch;        /* records inflated and decoded on the host                 */
    int32_t device;
    int32_t verbose;
} pf_hapmeth_opts_t;

typedef struct pf_hapmeth_stats {
    uint64_t n_windows;        /* windows planned                                          */
    uint64_t n_skipped;        /* of those, windows the index holds no chunk for (not fetched) */
    uint64_t n_records;        /* records fetched                                          */
    uint64_t n_sites;          /* lines written                                            */
    double ms_kernels;         /* summed pf_pileup_t.ms_kernels                            */
} pf_hapmeth_stats_t;

/* The windows of each contig (or of the region) in order, jobs of job_windows
 * windows one after another on one device: the device fetch (or the host
 * fetch) with no read-back margin, pf_batch_pileup under the records' HP
 * tags, pf_write_hapmeth.  stats may be NULL. */
int  pf_hapmeth_main(const pf_hapmeth_opts_t *o, pf_hapmeth_stats_t *stats);

/* hapmeth --dmr: the allele-specific methylated regions (pf_dmr_regions,
 * stitched by pf_dmr_acc_*) as BED lines, tab-separated:
 *   chrom start end n_sites dir h1_meth h1_unmeth h2_meth h2_unmeth delta pooled_p
 * dir "h1>h2" or "h1<h2"; the counts are the members' pooled sums; delta =
 * h1_meth/(h1_meth+h1_unmeth) - h2_meth/(h2_meth+h2_unmeth) as %.4f; pooled_p
 * the two-sided pf_fisher_exact of the pooled sums as %.6g.  pooled_p is a
 * ranking score, not a calibrated p-value: one read contributes to many CpGs,
 * so the pooled counts are not independent.  Lines with pooled_p > max_p are
 * dropped (max_p 1 keeps everything).  header as in pf_write_hapmeth.  A
 * pooled sum above INT32_MAX returns PF_ERR_LIMIT before anything is written. */
int  pf_write_dmr(const char *path, const char *chrom, const pf_dmr_t *dmr, double max_p, int header);

typedef struct pf_hapmeth_dmr {
    pf_dmr_cfg_t cfg;
    double max_p;              /* lines with pooled_p above it are dropped; 1 keeps all    */
    const char *blocks_path;   /* NULL, or a phase-block GTF as methphase writes it
                                  ({prefix}.mp.gtf; columns 4/5, 1-based): per contig each
                                  block's 0-based start and its end are breaks            */
} pf_hapmeth_dmr_t;

typedef struct pf_hapmeth_dmr_stats {
    uint64_t n_regions;        /* lines written to {out_prefix}.hapmeth.dmr.bed            */
    uint64_t n_informative;    /* informative sites                                        */
    double ms_kernels;         /* summed pf_dmr_t.ms_kernels                               */
} pf_hapmeth_dmr_stats_t;

/* pf_hapmeth_main, and with dmr != NULL also {out_prefix}.hapmeth.dmr.bed:
 * after each job's pileup pf_dmr_regions over the job's windows, stitched per
 * contig, flushed and appended at the contig's end; neither a job boundary nor
 * a skipped window changes the file.  On failure both files are unlinked.
 * dmr == NULL: exactly pf_hapmeth_main.  st and dst may be NULL. */
int  pf_hapmeth_run(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, pf_hapmeth_stats_t *st,
                    pf_hapmeth_dmr_stats_t *dst);

/* hapmeth --dmr --dmr-perm: pf_write_dmr's eleven columns unchanged, followed
 * by reads_h1 reads_h2 perm_p.  Window k of perm (pf_batch_permtest) is run k
 * of dmr: reads_h1 / reads_h2 its participating reads tagged 0 / 1, perm_p =
 * (hits + 1) / (n_perm + 1) as %.6g, or "." when the window's status is not 0.
 * Unlike pooled_p, perm_p is a p-value: the reads' labels are permuted, so the
 * correlation of one read's calls is part of the null distribution; its
 * smallest value is 1 / (n_perm + 1).  max_p, header and the INT32_MAX limit
 * as in pf_write_dmr.  PF_ERR_ARG when perm is NULL or holds fewer windows
 * than dmr has runs. */
int  pf_write_dmr_perm(const char *path, const char *chrom, const pf_dmr_t *dmr, const pf_perm_t *perm, double max_p,
                       int header);

typedef struct pf_hapmeth_perm {
    uint32_t n_perm;           /* permutations per region, 1 .. PF_PERM_MAX_PERM           */
    uint32_t seed;             /* the CLI's default is 1                                   */
} pf_hapmeth_perm_t;

typedef struct pf_hapmeth_perm_stats {
    uint64_t n_tested;         /* lines written with a numeric perm_p                      */
    uint64_t n_untested;       /* lines written with "."                                   */
    uint64_t n_records;        /* records fetched by the second pass                       */
    double ms_kernels;         /* summed pf_perm_t.ms_kernels                              */
} pf_hapmeth_perm_stats_t;

/* pf_hapmeth_run, and with perm != NULL a second pass at each contig's end,
 * where its regions are final: the regions that pass dmr->max_p become the
 * windows [start, end) of jobs of job_windows windows, each fetched like a job
 * of the first pass (the device fetch or the host fetch, no read-back margin,
 * the same loader configuration) and tested by pf_batch_permtest under the
 * records' HP tags; every read overlapping a region is one whole read of that
 * region's window, so the result depends on neither chunk_size, job_windows
 * nor the fetch kind.  The region file is then written by pf_write_dmr_perm.
 * perm == NULL: exactly pf_hapmeth_run (pst is zeroed).  perm without dmr, or
 * n_perm outside [1, PF_PERM_MAX_PERM], returns PF_ERR_ARG.  A failing fetch
 * of the second pass (PF_ERR_LIMIT included) fails the run and unlinks both
 * files.  st, dst and pst may be NULL. */
int  pf_hapmeth_run_perm(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_perm_t *perm,
                         pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst, pf_hapmeth_perm_stats_t *pst);

/* hapmeth --dmr --assign: the scored candidates of a pf_batch_assign result
 * as lines of {out_prefix}.hapmeth.assign.tsv, tab-separated (host only):
 *   qname chrom start end n_calls llr hp
 * one line per (window, read of it with n_used >= 1), windows in order and the
 * batch's read order inside a window; start / end the window's, n_calls the
 * read's n_used, llr = S / 65536.0 as %.4f (bits; positive: haplotype 1), hp
 * "1", "2" or "." (not assigned).  win_start / win_end: [a->n_windows];
 * rec_of_read: [a->n_reads] each read's record (pf_batch_read_recs), NULL for
 * the identity; qname_off / qname: the records' names as the fetch holds them
 * (pf_bam_records_t, pf_bam_dev_fetch_t).  header as in pf_write_hapmeth (then
 * a may be NULL).  n_lines, when given, receives the lines written. */
int  pf_write_assign(const char *path, const char *chrom, const pf_assign_t *a, const uint32_t *win_start,
                     const uint32_t *win_end, const uint32_t *rec_of_read, const uint64_t *qname_off, const char *qname,
                     int header, uint64_t *n_lines);

typedef struct pf_hapmeth_assign {
    int64_t  min_llr_q16;      /* pf_assign_cfg_t's; the CLI's default is 3 bits           */
    uint32_t min_calls;        /* pf_assign_cfg_t's; the CLI's default is 2                */
    uint32_t reserved;
} pf_hapmeth_assign_t;

typedef struct pf_hapmeth_assign_stats {
    uint64_t n_lines;          /* lines written to {out_prefix}.hapmeth.assign.tsv         */
    uint64_t n_h1, n_h2;       /* of those, assigned to haplotype 1 / 2                    */
    uint64_t n_records;        /* records fetched by the second pass                       */
    double ms_kernels;         /* summed pf_assign_t.ms_kernels                            */
} pf_hapmeth_assign_stats_t;

/* pf_hapmeth_run_perm, and with assign != NULL {out_prefix}.hapmeth.assign.tsv:
 * the second pass at each contig's end (the regions that pass dmr->max_p as the
 * windows of jobs of job_windows windows, each fetched once) serves both:
 * pf_batch_permtest when perm is given and pf_batch_assign when assign is, on
 * the same batch, under the records' HP tags; with assign alone the pass still
 * runs.  min_cov is dmr->cfg.min_cov, so the sites used are the region's own
 * members.  Neither file of the other features changes with assign.  assign ==
 * NULL: exactly pf_hapmeth_run_perm (ast is zeroed).  The pass's one fetch is
 * counted in pst.n_records when perm is given and in ast.n_records when assign
 * is.  assign without dmr returns PF_ERR_ARG.  On failure every file is unlinked.
 * st, dst, pst and ast may be NULL. */
int  pf_hapmeth_run_assign(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_perm_t *perm,
                           const pf_hapmeth_assign_t *assign, pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst,
                           pf_hapmeth_perm_stats_t *pst, pf_hapmeth_assign_stats_t *ast);

/* hapmeth --dmr --tag-check: the scored tagged reads of a pf_batch_tagcheck
 * result as lines of {out_prefix}.hapmeth.tagcheck.tsv, tab-separated (host
 * only):
 *   qname chrom start end hp n_calls llr verdict
 * one line per (window, read of it tagged 0 / 1 with n_used >= 1), windows in
 * order and the batch's read order inside a window; hp "1" / "2" the read's own
 * tag (t->hp), n_calls its n_used, llr = S / 65536.0 as %.4f, verdict "ok",
 * "flip" or "." (undecided).  The other arguments as in pf_write_assign. */
int  pf_write_tagcheck(const char *path, const char *chrom, const pf_tagcheck_t *t, const uint32_t *win_start,
                       const uint32_t *win_end, const uint32_t *rec_of_read, const uint64_t *qname_off, const char *qname,
                       int header, uint64_t *n_lines);
/* ... and its windows' counters as lines of
 * {out_prefix}.hapmeth.tagcheck.regions.tsv:
 *   chrom start end reads_h1 scored_h1 ok_h1 flip_h1 reads_h2 scored_h2 ok_h2 flip_h2
 * one line per window, t->win_n's eight numbers, also where nothing was scored. */
int  pf_write_tagcheck_regions(const char *path, const char *chrom, const pf_tagcheck_t *t, const uint32_t *win_start,
                               const uint32_t *win_end, int header, uint64_t *n_lines);

#define PF_HAPMETH_TAGCHECK_RULE_ONLY 1u   /* assign names the rule to check; --assign itself is off */
typedef struct pf_hapmeth_tagcheck {
    uint32_t flags;            /* 0 or PF_HAPMETH_TAGCHECK_RULE_ONLY                       */
    uint32_t reserved;
} pf_hapmeth_tagcheck_t;

typedef struct pf_hapmeth_tagcheck_stats {
    uint64_t n_lines;          /* lines written to {out_prefix}.hapmeth.tagcheck.tsv       */
    uint64_t n_regions;        /* lines written to ...tagcheck.regions.tsv                 */
    uint64_t n_ok[2];          /* of n_lines, per tag 0 / 1: ok,                           */
    uint64_t n_flip[2];        /* flip                                                     */
    uint64_t n_undecided[2];   /* and undecided                                            */
    uint64_t n_records;        /* records fetched by the second pass                       */
    double ms_kernels;         /* summed pf_tagcheck_t.ms_kernels                          */
} pf_hapmeth_tagcheck_stats_t;

/* pf_hapmeth_run_assign, and with tagcheck != NULL the two tag-check files: the
 * same second pass (the regions that pass dmr->max_p, each job fetched once)
 * also runs pf_batch_tagcheck on the batch, under the records' HP tags, with
 * min_cov = dmr->cfg.min_cov and the thresholds of assign -- the rule being
 * checked -- or, where assign is NULL, 3 bits (196,608) and 2 calls; with
 * tagcheck alone the pass still runs.  PF_HAPMETH_TAGCHECK_RULE_ONLY in
 * tagcheck->flags: assign gives the thresholds and nothing else, no assign
 * file is written and ast stays zero (`--tag-check --assign-min-llr 2`).  The
 * concordance of the run is ok / (ok + flip) over both tags; the verbose line
 * prints "n/a" for it where both are 0.  No file of the other features changes with
 * tagcheck.  tagcheck == NULL: exactly pf_hapmeth_run_assign (tst is zeroed).
 * tagcheck without dmr returns PF_ERR_ARG.  On failure every file is unlinked.
 * Every stats pointer may be NULL. */
int  pf_hapmeth_run_tagcheck(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_perm_t *perm,
                             const pf_hapmeth_assign_t *assign, const pf_hapmeth_tagcheck_t *tagcheck,
                             pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst, pf_hapmeth_perm_stats_t *pst,
                             pf_hapmeth_assign_stats_t *ast, pf_hapmeth_tagcheck_stats_t *tst);

/* hapmeth --dmr --dmr-hmm: the regions by pf_dmr_hmm_regions instead of
 * pf_dmr_regions. */
typedef struct pf_hapmeth_hmm {
    pf_dmr_hmm_cfg_t cfg;
} pf_hapmeth_hmm_t;

typedef struct pf_hapmeth_hmm_stats {
    uint64_t n_chains;         /* summed pf_dmr_hmm_t.n_chains                             */
    double ms_kernels;         /* summed pf_dmr_hmm_t.ms_kernels                           */
} pf_hapmeth_hmm_stats_t;

/* pf_hapmeth_run_tagcheck, and with hmm != NULL the regions of a contig come
 * from one pf_dmr_hmm_regions call at its end: each job's informative sites
 * (dmr->cfg.min_cov; transparent sites change nothing and are dropped) are
 * kept on the host, the contig's sites go through the model as one range under
 * dmr->cfg and the contig's breaks, and the kept runs are the regions --
 * tested, assigned from, checked and written exactly as pf_dmr_regions' are,
 * into the same file with the same columns.  Neither the chunk size, the job
 * size nor a skipped window changes a byte of it.  dst->ms_kernels counts the
 * model's kernels as the region kernels.  hmm == NULL: exactly
 * pf_hapmeth_run_tagcheck (hst is zeroed).  hmm without dmr, or a cost outside
 * [0, 64*65536], returns PF_ERR_ARG.  Every stats pointer may be NULL. */
int  pf_hapmeth_run_hmm(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                        const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                        const pf_hapmeth_tagcheck_t *tagcheck, pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst,
                        pf_hapmeth_hmm_stats_t *hst, pf_hapmeth_perm_stats_t *pst, pf_hapmeth_assign_stats_t *ast,
                        pf_hapmeth_tagcheck_stats_t *tst);

/* hapmeth --regions: the regions come from the caller, not from the data.
 *
 * pf_regions_load reads a BED: lines `chrom start end [name ...]`, tab or
 * space separated, 0-based half-open, plain or gzipped.  Lines that are empty
 * or start with '#', "track" or "browser" are skipped.  A last line without a
 * newline IS read (pf_mask_load and the other loaders of pf_windows.c drop it,
 * as the reference's reader does; there is no reference to follow here).  The
 * name is column 4, "." when absent; further columns are ignored.  Fewer than
 * three columns, a non-numeric bound or start > end: PF_ERR_ARG; end > 2^29:
 * PF_ERR_LIMIT; both name the line (1-based, every line counted) on stderr.  A
 * file that cannot be read: -1.  Lines whose contig is not in `names` are
 * dropped and counted (pf_regions_unknown).  Per contig the regions are stably
 * sorted by (start, end): ties keep file order. */
typedef struct pf_region_list pf_region_list_t;
int  pf_regions_load(const char *bed_path, uint32_t n_contigs, const char *const *names, pf_region_list_t **out);
/* contig c's regions (valid until pf_region_list_free); NULL arrays when *n is 0 */
int  pf_regions_contig(const pf_region_list_t *list, uint32_t c, const uint32_t **start, const uint32_t **end,
                       const char *const **name, uint64_t *n);
uint64_t pf_regions_unknown(const pf_region_list_t *list);
void pf_region_list_free(pf_region_list_t *list);

/* Benjamini-Hochberg q-values over the tested entries of a run's regions, from
 * the permutation test's hits.  With m the number of tested entries,
 *   p_i    = (hits_i + 1.0) / (n_perm + 1.0),
 *   rank_i = the number of tested entries with hits <= hits_i (ties share the
 *            largest rank),
 *   q_i    = min(1.0, min over tested j with hits_j >= hits_i of
 *                     (p_j * (double)m) / (double)rank_j),
 * evaluated in exactly this order of operations in doubles.  q[i] is NaN for an
 * untested entry.  The correction is right for a list fixed in advance; the
 * regions of --dmr and --dmr-hmm are selected on the data and get none. */
int  pf_bh_adjust(const uint32_t *hits, const uint8_t *tested, uint64_t n, uint32_t n_perm, double *q);

#define PF_REGION_TEST_MAX_SPAN 1000000u   /* a longer region is summed and never tested: its one window would risk
                                              the fetch's 65,535 records per window, which fails the whole run */
#define PF_REGION_SPLIT    1u  /* flags: a phase-block break x with start < x < end; counted, never tested */
#define PF_REGION_ELIGIBLE 2u  /* flags: the second pass took it: reads, hits and status are set         */
typedef struct pf_region_rec {
    const char *chrom, *name;
    uint32_t start, end;
    pf_region_sum_t s;         /* summed over the contig's jobs                  */
    uint32_t flags;            /* PF_REGION_*                                    */
    uint32_t reads[2];         /* pf_perm_t.n_reads of its window                */
    uint32_t hits, status;     /* pf_perm_t.hits, .status of its window          */
} pf_region_rec_t;
/* {prefix}.hapmeth.regions.bed, the whole file, tab-separated:
 *   #chrom start end name n_cpg n_sites n_h1gt n_h2gt dir h1_meth h1_unmeth
 *   h2_meth h2_unmeth delta pooled_p llr_bits block
 * n_h1gt / n_h2gt: s.n_pos / s.n_neg.  dir, with M1,U1,M2,U2 = s.sum[], N1 =
 * M1+U1, N2 = M2+U2: "h1>h2" if M1*N2 > M2*N1 (128 bits), "h1<h2" if less, "."
 * otherwise.  delta (%.4f) and pooled_p (%.6g) as pf_write_dmr; pooled_p is "."
 * when a sum exceeds INT32_MAX (a whole chromosome can; no error here).
 * llr_bits: s.evidence / 65536.0 as %.3f.  block: "split" or "ok".  perm != 0:
 * four more columns, reads_h1 reads_h2 perm_p perm_q.  A region that is not
 * PF_REGION_ELIGIBLE prints "." in all four; an eligible one its reads, and
 * with status 0 perm_p = (hits + 1) / (n_perm + 1) and perm_q =
 * pf_bh_adjust over the eligible status-0 records of rec[0, n), both %.6g,
 * else "." in both.  *n_tested: the records with a numeric perm_p. */
int  pf_write_regions(const char *path, const pf_region_rec_t *rec, uint64_t n, int perm, uint32_t n_perm,
                      uint64_t *n_tested);

typedef struct pf_hapmeth_regions {
    const char *bed_path;
} pf_hapmeth_regions_t;

typedef struct pf_hapmeth_regions_stats {
    uint64_t n_regions;        /* lines of {prefix}.hapmeth.regions.bed                    */
    uint64_t n_unknown_contig; /* BED lines on a contig the BAM does not have              */
    uint64_t n_outside;        /* regions not wholly inside the run's range (opts.region)  */
    uint64_t n_split;          /* written regions with block "split"                       */
    uint64_t n_tested;         /* with perm: written regions with a perm_p                 */
    uint64_t n_untested;       /* with perm: the other written regions                     */
    double ms_kernels;         /* summed pf_regions_t.ms_kernels                           */
} pf_hapmeth_regions_stats_t;

/* pf_hapmeth_run_hmm, and with regions != NULL the second source of regions:
 * the BED's.  After each job's pileup pf_region_sums takes the contig's regions
 * that can intersect the job's span, and the records add up per region on the
 * host (additivity, above), so neither the chunk size, the job size, a skipped
 * window nor the fetch kind changes a byte.  With opts.region, regions not
 * wholly inside it are dropped and counted.  {out_prefix}.hapmeth.regions.bed
 * (pf_write_regions) holds one line per kept region, contigs in header order,
 * regions in pf_regions_load's order; it is written at the end of the run
 * because perm_q needs every region.  No .hapmeth.dmr.bed is written.  dmr
 * gives cfg (min_cov, min_delta_pct; min_sites and max_p for eligibility),
 * and blocks_path the breaks.  The second pass (perm, assign, tagcheck; files
 * and formats as before) runs on the windows [start, end) of the eligible
 * regions: not split, s.n_sites >= min_sites, pooled_p numeric and <= max_p,
 * start < end and end - start <= PF_REGION_TEST_MAX_SPAN.  regions == NULL:
 * exactly pf_hapmeth_run_hmm (rst is zeroed).  regions without dmr, or with
 * hmm, returns PF_ERR_ARG.  On failure every file is unlinked.  Every stats
 * pointer may be NULL. */
int  pf_hapmeth_run_regions(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                            const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                            const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                            pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst, pf_hapmeth_hmm_stats_t *hst,
                            pf_hapmeth_perm_stats_t *pst, pf_hapmeth_assign_stats_t *ast, pf_hapmeth_tagcheck_stats_t *tst,
                            pf_hapmeth_regions_stats_t *rst);

/* pf_bh_adjust with the p-values given as doubles: the tested entries sorted by
 * (p, index), a group of exactly equal p shares the rank b of its last member,
 * x = (p * (double)m) / (double)b with m the tested entries, q the running
 * minimum of x from the largest p down, capped at 1.0; NaN for an untested
 * entry.  A tested p that is NaN returns PF_ERR_ARG. */
int  pf_bh_adjust_p(const double *p, const uint8_t *tested, uint64_t n, double *q);

/* hapmeth --dmr-rank: one region of the second pass and its window of
 * pf_batch_ranktest. */
typedef struct pf_rank_rec {
    const char *chrom;
    uint32_t start, end;
    uint32_t reads[2];         /* pf_rank_t.n_reads of its window                 */
    uint32_t n_short[2];       /* .n_short                                        */
    uint32_t cls[6];           /* .cls                                            */
    uint32_t status;           /* .status                                         */
    uint64_t u2, ties;         /* .u2, .ties                                      */
} pf_rank_rec_t;
/* {prefix}.hapmeth.rank.tsv, the whole file, tab-separated:
 *   #chrom start end reads_h1 reads_h2 short_h1 short_h2 allmeth_h1
 *   allunmeth_h1 mixed_h1 allmeth_h2 allunmeth_h2 mixed_h2 auc z rank_p rank_q
 * one line per record in the given order.  With status 0: auc (%.4f), z (%.3f)
 * and rank_p (%.6g) by pf_rank_p, and with bh != 0 rank_q (%.6g) by
 * pf_bh_adjust_p over the status-0 records of rec[0, n), "." with bh == 0 (the
 * regions of --dmr are selected on the data and get no correction); any other
 * status prints "." in all four.  No record: the header alone.  *n_tested: the
 * records with a numeric rank_p. */
int  pf_write_rank(const char *path, const pf_rank_rec_t *rec, uint64_t n, int bh, uint64_t *n_tested);

typedef struct pf_hapmeth_rank {
    uint32_t min_calls;        /* pf_batch_ranktest's, 1 .. 65535; the CLI's default is 3  */
} pf_hapmeth_rank_t;

typedef struct pf_hapmeth_rank_stats {
    uint64_t n_tested;         /* lines of the rank file with a numeric rank_p             */
    uint64_t n_untested;       /* its other lines                                          */
    uint64_t n_records;        /* records fetched by the second pass                       */
    double ms_kernels;         /* summed pf_rank_t.ms_kernels                              */
} pf_hapmeth_rank_stats_t;

/* pf_hapmeth_run_regions, and with rank != NULL {out_prefix}.hapmeth.rank.tsv
 * (pf_write_rank): the second pass, on the batch it fetched for perm, assign
 * and tagcheck (with rank alone the pass still runs), also runs
 * pf_batch_ranktest under the records' HP tags.  The windows are the pass's own:
 * with dmr alone the regions that pass max_p, with regions the eligible ones.
 * One record per region of the pass, in the order the pass takes them, kept on
 * the host and written at the run's end, rank_q with regions only.  No file of
 * the other features changes with rank.  rank == NULL: exactly
 * pf_hapmeth_run_regions (kst is zeroed).  rank without dmr, or min_calls
 * outside [1, 65535], returns PF_ERR_ARG.  On failure every file is unlinked.
 * Every stats pointer may be NULL. */
int  pf_hapmeth_run_rank(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                         const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                         const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                         const pf_hapmeth_rank_t *rank, pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst,
                         pf_hapmeth_hmm_stats_t *hst, pf_hapmeth_perm_stats_t *pst, pf_hapmeth_assign_stats_t *ast,
                         pf_hapmeth_tagcheck_stats_t *tst, pf_hapmeth_regions_stats_t *rst, pf_hapmeth_rank_stats_t *kst);

/* hapmeth --dmr-rank-exact: a region's window of pf_batch_rankexact, parallel
 * to its pf_rank_rec_t. */
typedef struct pf_rank_exact_rec {
    uint64_t two, total;       /* pf_rank_exact_t.two, .total of its window       */
    uint32_t status;           /* .status                                         */
} pf_rank_exact_rec_t;
/* {prefix}.hapmeth.rank.tsv with the exact test: pf_write_rank's line, its 17
 * columns byte for byte, and three more,
 *   exact_p best_p best_q
 * exact_p = two / total (pf_rank_exact_p, %.6g) where xrec[i].status is 0, else
 * "."; best_p = exact_p where that is numeric, else rank_p (which may be ".");
 * best_q (%.6g) with bh != 0 by pf_bh_adjust_p over the records with a numeric
 * best_p, "." with bh == 0 and where best_p is ".": the rule rank_q follows.
 * *n_tested as in pf_write_rank; *n_exact: the records with a numeric exact_p.
 * n != 0 without xrec, a status-0 xrec with total == 0 or two > total:
 * PF_ERR_ARG. */
int  pf_write_rank_exact(const char *path, const pf_rank_rec_t *rec, const pf_rank_exact_rec_t *xrec, uint64_t n, int bh,
                         uint64_t *n_tested, uint64_t *n_exact);

typedef struct pf_hapmeth_rank_exact {
    uint32_t max_reads;        /* pf_batch_rankexact's, 2 .. 64; the CLI's default is 64   */
} pf_hapmeth_rank_exact_t;

typedef struct pf_hapmeth_rank_exact_stats {
    uint64_t n_exact;          /* lines of the rank file with a numeric exact_p            */
    uint64_t n_over;           /* lines whose region has more than max_reads counted reads */
    double ms_kernels;         /* summed pf_rank_exact_t.ms_kernels                        */
} pf_hapmeth_rank_exact_stats_t;

/* pf_hapmeth_run_rank, and with exact != NULL the second pass also runs
 * pf_batch_rankexact right after pf_batch_ranktest, on the same batch with the
 * same min_calls (no further fetch), and the rank file is written by
 * pf_write_rank_exact.  No other file changes.  exact == NULL: exactly
 * pf_hapmeth_run_rank (xst is zeroed).  exact without rank, or max_reads
 * outside [2, 64], returns PF_ERR_ARG. */
int  pf_hapmeth_run_rank_exact(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                               const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                               const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                               const pf_hapmeth_rank_t *rank, const pf_hapmeth_rank_exact_t *exact, pf_hapmeth_stats_t *st,
                               pf_hapmeth_dmr_stats_t *dst, pf_hapmeth_hmm_stats_t *hst, pf_hapmeth_perm_stats_t *pst,
                               pf_hapmeth_assign_stats_t *ast, pf_hapmeth_tagcheck_stats_t *tst,
                               pf_hapmeth_regions_stats_t *rst, pf_hapmeth_rank_stats_t *kst,
                               pf_hapmeth_rank_exact_stats_t *xst);

/* hapmeth --tile: what a tile's line holds beside its pf_rank_rec_t. */
typedef struct pf_rank_tile_rec {
    uint64_t sum[4];           /* pf_rank_t.sum of its range: the counted reads' m1, u1, m2, u2 */
    uint32_t split;            /* non-zero: a phase-block break x with start < x < end (the
                                  PF_REGION_SPLIT rule): counted, never tested             */
} pf_rank_tile_rec_t;
/* {prefix}.hapmeth.tiles.tsv, the whole file: pf_write_rank's line, its 17
 * columns by the same code, and six more,
 *   h1_meth h1_unmeth h2_meth h2_unmeth delta block
 * the counted reads' sums, delta as in pf_write_dmr (%.4f; "." where a
 * haplotype has no counted call) and block "ok" or "split".  A split record
 * prints "." in auc, z, rank_p and rank_q.  rank_q is pf_bh_adjust_p over the
 * status-0 records of rec[0, n) that are not split: the tiles are fixed in
 * advance, so the correction holds.  No record: the header alone.  *n_tested:
 * the records with a numeric rank_p.  n != 0 without trec: PF_ERR_ARG; -1 when
 * the file cannot be written. */
int  pf_write_rank_tiles(const char *path, const pf_rank_rec_t *rec, const pf_rank_tile_rec_t *trec, uint64_t n,
                         uint64_t *n_tested);

typedef struct pf_hapmeth_tiles {
    uint32_t tile;             /* tile width T in bases, 100 .. the chunk size, which must be a
                                  multiple of it                                           */
    uint32_t min_calls;        /* pf_batch_rankranges', 1 .. 65535; the CLI's default is 3  */
    const char *blocks_path;   /* NULL, or a phase-block GTF, read where the run has no dmr;
                                  with dmr the run's one table is dmr->blocks_path        */
} pf_hapmeth_tiles_t;

typedef struct pf_hapmeth_tiles_stats {
    uint64_t n_tiles;          /* tiles planned: ceil(span / T) over the run's spans        */
    uint64_t n_written;        /* lines of the tile file: tiles with a participating read   */
    uint64_t n_tested;         /* of those, with a numeric rank_p                           */
    uint64_t n_split;          /* of those, with block "split"                              */
    double ms_kernels;         /* summed pf_rank_t.ms_kernels of the range calls            */
} pf_hapmeth_tiles_stats_t;

/* pf_hapmeth_run_rank_exact, and with tiles != NULL {out_prefix}.hapmeth.tiles.tsv
 * (pf_write_rank_tiles): a genome-wide scan in the first pass.  A span [s, e)
 * -- a contig, or opts.region -- is cut into the tiles [s + j*T, min(s +
 * (j+1)*T, e)); the chunk size is a multiple of T, so a tile lies in one fetch
 * window, and a window the index holds no chunk for contributes none.  After
 * each job's pileup one pf_batch_rankranges call on the same batch (its calls
 * taken as the pileup left them, no second load stage) tests the tiles of the
 * job's windows under the records' HP tags; a tile with a participating read on
 * either haplotype becomes a record, kept on the host (120 bytes each) until
 * the file is written at the run's end, because rank_q needs all of them.
 * Neither the chunk size, the job size nor the fetch kind changes a byte.
 * Tiles need no dmr and combine with every other option; no other file
 * changes with tiles.  tiles == NULL: exactly pf_hapmeth_run_rank_exact (lst is
 * zeroed).  T below 100 or above the chunk size, a chunk size that is no
 * multiple of T, or min_calls outside [1, 65535] returns PF_ERR_ARG before
 * any file is made.  On failure every file is unlinked.  Every stats pointer
 * may be NULL. */
int  pf_hapmeth_run_tiles(const pf_hapmeth_opts_t *o, const pf_hapmeth_dmr_t *dmr, const pf_hapmeth_hmm_t *hmm,
                          const pf_hapmeth_perm_t *perm, const pf_hapmeth_assign_t *assign,
                          const pf_hapmeth_tagcheck_t *tagcheck, const pf_hapmeth_regions_t *regions,
                          const pf_hapmeth_rank_t *rank, const pf_hapmeth_rank_exact_t *exact, const pf_hapmeth_tiles_t *tiles,
                          pf_hapmeth_stats_t *st, pf_hapmeth_dmr_stats_t *dst, pf_hapmeth_hmm_stats_t *hst,
                          pf_hapmeth_perm_stats_t *pst, pf_hapmeth_assign_stats_t *ast, pf_hapmeth_tagcheck_stats_t *tst,
                          pf_hapmeth_regions_stats_t *rst, pf_hapmeth_rank_stats_t *kst, pf_hapmeth_rank_exact_stats_t *xst,
                          pf_hapmeth_tiles_stats_t *lst);

/* Host helper: htslib kt_fisher_exact semantics. Returns the probability of
 * the observed table. */
double pf_fisher_exact(int n11, int n12, int n21, int n22,
                       double *left, double *right, double *two);

#ifdef __cplusplus
}
#endif
#endif /* POMFRET_AMD_H */
