/*
 * pf_device.h -- device-side layout shared by the methphase kernels.
 *
 * HBM layout of one resident batch (all SoA, one allocation per array):
 *   windows : win_start/win_end/win_read_off/win_par          [W]
 *   reads   : read_start/end/first/last/win, read_hp           [R]
 *             read_call_off, read_call_end                      [R]
 *   calls   : call_pos (u32), call_cat (u8)
 *             read r's calls are [read_call_off[r], read_call_end[r]),
 *             sorted by (pos, cat).  A calls-level batch holds them as one
 *             run of N in read order (read_call_end = read_call_off + 1); a
 *             record-level batch reads them where K0 staged them (pf_load.h),
 *             in no order across reads and with unused slots between them
 *   sites   : per window a slice [site_off[w], +site_cap[w]) of
 *             site_pos, st1_pos, site_q1 (u32) and len0, len1 (u8)
 *   methmers: per (read, dir) a slice of the key arena (u32): methmer keys,
 *             rewritten in place to per-site slot ids before the greedy loop
 */
#ifndef PF_DEVICE_H
#define PF_DEVICE_H
#include <stdint.h>

#define PF_WAVE 64
#define PF_K1_THREADS 1024
#define PF_K1_TILE 32768          /* positions per dense LDS tile (128 KB of u32 counters) */
#define PF_K2_WAVES 4
#define PF_K2_ENT_CAP 1024        /* per-wave LDS entry buffer; larger reads use HBM scratch */
#define PF_K3_THREADS 256
#define PF_K3_WAVES (PF_K3_THREADS / PF_WAVE)
#define PF_K3S_THREADS 256         /* the main (slim) greedy kernel (512 measured: DESIGN.md 8) */
#ifndef PF_K3H_THREADS
#define PF_K3H_THREADS 256         /* pf_k3_heavy (512 measured in round 6: critical window 3.37 -> 3.65 ms, profiles/r06/ab_k3_heavy512.txt) */
#endif
#define PF_MAX_NCAND 256
#define PF_K12_CAPW 512           /* per-wave site-entry buffer of the fused methmer phase */
#define PF_K12_WB 8               /* bytes per wave-buffer entry: chars, crank, u16 irank, u32 staged key */
#define PF_K12_SMAX 4600          /* sites whose arrays (14 B/site) fit LDS beside 16 such buffers */
#define PF_K12C_READS 64          /* reads per item of pf_k12_chunks (the heavy windows' methmer phase) */
#define PF_K12C_WAVES 8           /* its waves per workgroup */
#define PF_K12C_LDS 61440         /* its dynamic LDS: 14 B per site + PF_K12C_WAVES wave buffers (2 per CU) */
#define PF_PILE_TILE 4096          /* positions per LDS tile of the pileup: 3 packed u32 each, 48 KB (3 workgroups per CU) */
#define PF_PILE_TILE_MAX 8192      /* PF_PILE_TILE=<n> override: 96 KB */
#define PF_PILE_THREADS 1024        /* 16 waves: a window's reads are searched 64 per wave at once */
#define PF_PILE_WAVES (PF_PILE_THREADS / PF_WAVE)
#define PF_PILE_SCAN_THREADS 1024
#ifndef PF_DMR_BLOCK
#define PF_DMR_BLOCK 1024           /* sites per workgroup of the region kernels, and the PF_DMR_BLOCK=<n> override's
                                      upper bound (measured against 256 .. 4096: profiles/dmr/README.md) */
#endif
#define PF_DMR_THREADS 256          /* each thread folds PF_DMR_BLOCK / PF_DMR_THREADS consecutive sites */
#define PF_DMR_WAVES (PF_DMR_THREADS / PF_WAVE)
#define PF_REG_BLOCK 1024           /* sites per workgroup of pf_region_sums' kernels (PF_DMR_THREADS threads), and the
                                      PF_REG_BLOCK=<n> override's upper bound */
#define PF_PERM_THREADS 256         /* the permutation test's workgroup (PF_PERM_THREADS=<64|256|1024> overrides it) */
#define PF_PERM_THREADS_MAX 1024
#define PF_PERM_READS 4096          /* participating reads per window held in LDS (PF_PERM_MAX_READS): 8 B each */
#define PF_RANK_THREADS 256         /* the rank test's workgroup, pf_rank_ranges' too (PF_RANK_THREADS=<64|256|1024>
                                      overrides it; for the ranges measured in profiles/rank_ranges/README.md) */
#define PF_RANK_THREADS_MAX 1024
#define PF_RANK_READS 4096          /* counted reads per window held in LDS (PF_RANK_MAX_READS): 8 B each, 32 KB */
#define PF_RANK_NARROW_MAX 65535u   /* a window whose largest n_i is at most this compares 32-bit products */
#define PF_RANKX_THREADS 1024       /* the exact rank test's workgroup (PF_RANKX_THREADS=<64|256|1024> overrides it;
                                      measured: profiles/rank_exact/README.md) */
#define PF_RANKX_READS 64           /* counted reads of a window the exact test takes (PF_RANK_EXACT_MAX_READS) */
#define PF_RANKX_LDS_CELLS 8113u    /* its LDS array in cells of 8 B: the table of 36 reads, 18 a class (63.4 KB); during
                                      the read loop the same array holds the counted reads */
#define PF_RANKX_SLAB_CELLS 44737u  /* the table of 64 reads, 32 a class: the largest per-workgroup slab in HBM, 358 KB */
#define PF_RANKX_GRID 512u          /* at most this many workgroups, one slab each (PF_RANKX_GRID=<n> overrides it) */
#define PF_ASSIGN_TILE 4096         /* sites per LDS tile of pf_assign_score: position and two weights, 12 B each, 48 KB
                                      (PF_ASSIGN_TILE=<n> overrides it downwards) */
#define PF_ASSIGN_THREADS 256       /* its workgroup: each wave takes 64 of the window's reads at a time (1,024 measured:
                                      profiles/assign/README.md) */
#define PF_ASSIGN_WAVES (PF_ASSIGN_THREADS / PF_WAVE)
#define PF_TAGCHECK_TILE 2048       /* sites per LDS tile of pf_tagcheck_score: position and four weights, 20 B each, 40 KB
                                      (PF_TAGCHECK_TILE=<n> overrides it downwards; 4,096 would be 80 KB) */
#define PF_TAGCHECK_THREADS 256     /* its workgroup: 256 of the window's reads at a time, one per lane, their hits dealt
                                      to the four waves */
#define PF_TAGCHECK_WAVES (PF_TAGCHECK_THREADS / PF_WAVE)
#define PF_NONE 0xFFFFFFFFu

/* status bits */
#define PF_ST_KEYS_OVF   1u
#define PF_ST_BIG_OVF    2u
#define PF_ST_SCR_OVF    4u
#define PF_ST_SITE_OVF   8u
#define PF_ST_INTERNAL  16u

struct pf_dev_batch {
    uint32_t W, R;
    uint64_t N;
    int32_t k, k_span, hard_cov, mw;   /* mw: 64-bit mask words per site = max(1, 4^k/64) */
    /* windows */
    const uint32_t *win_start, *win_end, *win_read_off;
    const int32_t *win_par;            /* [W*4]: cov_sel, cov_rt, n_cand, 0 */
    const uint64_t *win_site_off;
    const uint32_t *win_site_cap;
    /* reads */
    const uint32_t *read_start, *read_end, *read_first, *read_last, *read_win;
    const uint8_t *read_hp;
    const uint64_t *read_call_off, *read_call_end;   /* read r's calls: [off[r], end[r]) */
    /* calls */
    const uint32_t *call_pos;
    const uint8_t *call_cat;
    uint32_t *fb_list, *fb_ctr;        /* reads left to the K2 fallback kernel */
    uint32_t *k12c_list, *k12c_ctr;    /* (window, first read) chunks of the heavy windows for pf_k12_chunks */
    uint32_t *k12c_next;               /* pf_k12_chunks' next item */
    uint32_t k12c_minr, k12c_smax;     /* windows with >= k12c_minr reads and <= k12c_smax sites go there */
    /* per-window results of K1 */
    uint32_t *win_S, *win_nreads;
    const uint32_t *k3_order;          /* [2W] greedy problems (w<<1|dir), heaviest first */
    const uint32_t *k12_order;         /* [W] windows for K12's workgroups, heaviest first */
    uint32_t *k3_fb_list, *k3_fb_ctr;  /* problems the main greedy kernel defers to pf_k3_fallback */
    uint32_t *k3_next;                 /* the persistent main greedy kernel's next problem (rank in k3_order) */
    uint32_t k3_n;                     /* its problems: k3_order[0, k3_n) */
    uint32_t *site_pos, *st1_pos, *site_q1;
    uint8_t *len0, *len1;
    uint32_t *rev_ord;                 /* [R] window-local read index, ascending (end, idx) */
    /* methmers */
    uint32_t *mmr_n, *mmr_start;       /* [2R] */
    uint64_t *mmr_off;                 /* [2R] */
    uint32_t *mmr_cap;                 /* [R]  */
    uint64_t *big_off;                 /* [R]  */
    uint32_t *keys; uint64_t keys_cap; unsigned long long *keys_ctr;
    uint8_t *big; uint64_t big_cap; unsigned long long *big_ctr;
    uint8_t *scr; uint64_t scr_cap; unsigned long long *scr_ctr;
    /* the slim greedy loop's per-read side arrays in HBM, when its slot lists
     * miss LDS (k3_side_mem): hp, flg [2R] bytes, ord [R] u16, aux [2R] u32 */
    uint8_t *k3_side;
    /* outputs */
    int32_t *table;                    /* [W*2*4] */
    uint8_t *hp_fwd;                   /* [R] */
    unsigned long long *stats;         /* [W*2*4] per problem: lookups, inserts, iterations, scanned */
    uint32_t *status;
    unsigned long long *prof;          /* [W*2*8] diagnostic build only */
    uint32_t lds_bytes;                /* dynamic LDS of the main greedy kernel */
    uint32_t lds_fb;                   /* dynamic LDS of the fallback greedy kernel (>= lds_bytes) */
    uint32_t lds_heavy;                /* dynamic LDS of pf_k3_heavy (the heavy problems' slim loop) */
    uint32_t lds_w;                    /* dynamic LDS of the one-wave greedy kernel */
    uint32_t k12_capw, k12_smax;       /* fused methmer phase limits (test overrides) */
    uint32_t k12_dense;                /* 1: every window takes K12's dense (HBM) site path (tests) */
    uint32_t k2_entcap;                /* fallback reads above this bound use HBM scratch */
    uint32_t k3_mode;                  /* test override: 0 exact pick, 1 always fold, 2 chunked record rows */
    uint32_t k3_cache;                 /* 1: candidate slot-list cache when a window's lists miss LDS (PF_K3_CACHE=0: off) */
    uint32_t k3_gcnt;                  /* 1: path 6 (cache + count table in HBM) for every cache problem (PF_K3_GCNT=force) */
    /* k > 5 (or PF_K3_KDICT=1): the slot dictionary is built by pf_k3_kdict
     * before the greedy kernels (per-site hash tables in HBM scratch instead
     * of 4^k-bit masks), which rewrite no keys and read ntot from k3_ntot */
    uint32_t kdict;
    uint8_t *k12_path;                 /* [W] K12's sites path of the last run: 1 / 2 the fast path over 1 / 2
                                          segments, 3 the dense path, 0 none (no calls, left coverage) */
    uint32_t *k3_ntot;                 /* [2W] slots of each problem (kdict) */
    /* masked reference positions (pf_batch_set_mask): a position that qualifies
     * as a site by its counts and is in the mask is no site (blockjoin.c:3202-3205,
     * 3277-3283); K12 alone reads them */
    const uint32_t *mask_pos;          /* [mask_n] ascending, unique */
    const uint32_t *win_mask_rng;      /* [2W] window w sees mask_pos[rng[2w], rng[2w+1]); NULL: all of it */
    uint32_t *win_masked;              /* [W] qualifying positions the mask removed (the reference's n_filtered) */
    uint32_t mask_n;                   /* 0: no mask */
};

/* What a per-window consumer of the batch's calls reads (pf_reads.h has the
 * scan over it and pf_calls_view_of, which fills it from a pf_dev_batch) */
struct pf_calls_view {
    const uint32_t *win_start, *win_end, *win_read_off;
    const uint8_t *read_hp;                          /* the batch's tags or the caller's */
    const uint64_t *read_call_off, *read_call_end;   /* read r's calls: [off[r], end[r]) */
    const uint32_t *call_pos;
    const uint8_t *call_cat;
};

/* The per-haplotype pileup (pf_pileup.hip): one workgroup per item, an item
 * being one tile of T positions of one window; window w owns the items
 * [tile_off[w], tile_off[w+1]), tile j covering [win_start + j*T, +T) cut at
 * win_end.  The count pass writes each item's sites to item_cnt, the scan
 * turns them into item_off and win_off, the emit pass rebuilds each tile and
 * writes its sites at item_off. */
struct pf_pile_args {
    uint32_t W, T, n_items;
    pf_calls_view v;
    const uint32_t *tile_off;                        /* [W+1] */
    uint32_t *item_cnt;                              /* [n_items] */
    uint64_t *item_off;                              /* [n_items+1] */
    uint64_t *win_off;                               /* [W+1] */
    uint32_t *out_pos;                               /* [n_sites] */
    uint32_t *out_cnt;                               /* [n_sites*6] */
    uint32_t *status;                                /* bit 0: a 16-bit counter wrapped */
};

/* pf_batch_pileup's site CSR left in HBM (pf_batch_pileup_dev, pf_api.hip) for
 * a consumer in another file (pf_assign.hip); pf_pile_dev_free releases it */
struct pf_pile_dev {
    uint32_t W;
    uint64_t n_sites;                                /* 0: the three arrays are NULL */
    uint64_t *win_off;                               /* [W+1] */
    uint32_t *pos;                                   /* [n_sites] ascending inside a window */
    uint32_t *cnt;                                   /* [n_sites*6] */
    float ms_kernels;                                /* the pileup kernels */
};

#endif
