// pf_rank.hip -- read-level rank-sum test of a batch's windows
// (pf_batch_ranktest; include/pomfret_amd.h has the definition).
//
// One workgroup per window, two phases, all in integers.
//
// Phase 1 takes the window's reads blockDim.x at a time, one per lane, and
// counts each one's meth and unmeth entries inside the window: the shared
// read-slice scan (pf_reads.h, window_read_counts).  The counted reads (tag 0
// or 1, at least min_calls entries) are compacted in read order into LDS
// (block_compact) as (m, n | tag << 31), 8 B each; the class counters, the
// sums, the short reads and the largest n are collected by LDS integer
// atomics.
//
// Phase 2 is the all-pairs pass.  A lane owns a row i (rows tid, tid +
// blockDim.x, ...); every j comes as a broadcast, all lanes reading one LDS
// address, which costs no bank conflict.  Per pair two products and two
// compares: the lane counts g_i (f_i > f_j) and c_i (f_i == f_j) over the j
// tagged 1 -- they enter G and E only where i is tagged 0 -- and e_i (f_i ==
// f_j) over every j.  The waves reduce the three sums, add them in LDS as
// 64-bit integers, and the window is stored once.  No HBM atomic, no scratch.
// The pass is instantiated for 32-bit and for 64-bit products and chosen per
// window: where the window's largest n is at most 65,535 every product is
// below 2^32.  Integer sums only: neither the workgroup size, the product
// width nor the order of the atomics reaches the result.
//
// pf_rank_ranges (pf_batch_rankranges) is the same test over position ranges
// inside the windows, one workgroup per range: the genome-wide tiles of hapmeth
// --tile, tested in the first pass from the calls the pileup has just read.
// The two phases are one body, rank_one, for both kernels.  The counted reads
// lie in dynamic LDS sized to the batch's largest window: a tile counts tens of
// reads, and a 32 KB request keeps workgroups off a CU (2.9 x at 12,800
// ranges).  A pre-test of each read's span (first and last call position,
// stored once a call) against the range, to spare the slice's two dependent
// loads for the reads that lie elsewhere, was built and measured: 2 to 4 %,
// less than the extra kernel costs, so it is not here
// (profiles/rank_ranges/README.md).
//
// pf_rank_exact (pf_batch_rankexact) counts the exact null distribution of the
// same statistic for windows of at most 64 counted reads.  A workgroup takes
// the windows blockIdx.x, blockIdx.x + gridDim.x, ... and per window:
//   1  the read loop above; the counted reads go into s_buf, the one large LDS
//      array, 8 B each;
//   2  r_i = 2 * #{f_j < f_i} + #{f_j == f_i} of every counted read by the
//      all-pairs pass, products as above; u2 = (sum of r_i over the reads
//      tagged 0) - n1^2.  A window over max_reads is not counted, but its u2 is
//      still pf_rank_test's: rank_rows runs over s_buf;
//   3  ways[c][s], the subsets of c reads whose r_i sum to s, for c up to k,
//      the smaller class: one pass per read, rows walked downwards with a
//      barrier after each, the threads spread over a row's cells.  Row c holds
//      s in [c^2, c(2n - c)] and a pass touches only the rows that this read
//      can reach and that can still reach row k.  The table replaces the reads
//      in s_buf where it fits (PF_RANKX_LDS_CELLS) and lies in the workgroup's
//      slab in HBM otherwise, read and written by consecutive lanes;
//   4  row k summed into total, le, ge and two: wave sums, one LDS add a wave.
// Rows are walked in place, not double-buffered: a second buffer halves what
// fits in LDS (30 reads instead of 36) and the double-buffered walk was not
// built, so the choice rests on capacity, not on a timing.  64-bit integer
// adds only; no HBM atomic, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "pf_device.h"
#include "pf_reads.h"
#include "pf_call.h"
#include "../../include/pomfret_amd.h"

struct pf_ctx;
struct pf_dbatch;
extern "C" int pf_ctx_device(const pf_ctx *c);
extern "C" hipStream_t pf_ctx_stream(const pf_ctx *c);
extern "C" int pf_batch_calls_view(pf_ctx *ctx, pf_dbatch *b, pf_dev_batch *view);       // pf_api.hip
extern "C" int pf_batch_calls_loaded(pf_ctx *ctx, pf_dbatch *b, pf_dev_batch *view);

namespace {

static_assert(PF_RANK_READS == PF_RANK_MAX_READS, "the LDS array holds exactly the documented limit");

#define RANK_ST_LIMIT 3u            /* internal: N >= 2^31, the call returns PF_ERR_LIMIT */
#ifndef PF_RANK_UNROLL
#define PF_RANK_UNROLL 4             /* pairs per trip of the j loop (measured: profiles/rank/README.md) */
#endif
#define RANK_UNROLL PF_RANK_UNROLL

struct rank_out {
    uint64_t sum[4];
    uint64_t u2, ties;
    uint32_t n_reads[2], n_short[2], cls[6];
    uint32_t status, wide;                           /* wide: the products the window took (not part of pf_rank_t) */
};
static_assert(sizeof(rank_out) == 96, "rank_out is copied back as 96-byte records");

struct rankx_out {
    uint64_t u2, total, le, ge, two;
    uint32_t n_reads[2], n_short[2];
    uint32_t status, hbm;                            /* hbm: where the table lay (not part of pf_rank_exact_t) */
};
static_assert(sizeof(rankx_out) == 64, "rankx_out is copied back as 64-byte records");

struct rankx_args {
    uint32_t W, min_calls, max_reads, force_hbm;
    pf_calls_view v;
    rankx_out *out;                                  /* [W] */
    uint64_t *slab;                                  /* [gridDim.x * slab_cells], NULL where every table fits in LDS */
    uint64_t slab_cells;
};

// the cells of rows 0 .. c - 1 of a window of n counted reads: row c' has 2 c' (n - c') + 1
__host__ __device__ constexpr uint32_t rankx_off(uint32_t n, uint32_t c) {
    return c ? n * c * (c - 1u) - (c - 1u) * c * (2u * c - 1u) / 3u + c : 0u;
}
static_assert(rankx_off(PF_RANKX_READS, PF_RANKX_READS / 2u + 1u) == PF_RANKX_SLAB_CELLS, "the largest slab");
static_assert(rankx_off(36u, 19u) == PF_RANKX_LDS_CELLS, "the LDS array is the table of 36 reads, 18 a class");

struct rank_args {
    uint32_t W, min_calls, force_wide, pad;
    pf_calls_view v;                                 /* read_hp: the batch's tags or the caller's */
    rank_out *out;                                   /* [W] */
};

// The rows tid, tid + nt, ... of the n counted reads in s_r against every j.
// P: the products' type, uint32_t where every n is at most 65,535.
template <typename P>
__device__ __forceinline__ void rank_rows(const uint2 *s_r, uint32_t n, uint32_t tid, uint32_t nt, uint64_t &G, uint64_t &E,
                                          uint64_t &T) {
    for (uint32_t i = tid; i < n; i += nt) {
        const uint2 ri = s_r[i];
        const P mi = (P)ri.x, ni = (P)(ri.y & 0x7FFFFFFFu);
        uint32_t g = 0, c = 0, e = 0;
        auto pair = [&](uint32_t j) {
            const uint2 rj = s_r[j];                  // the same address in every lane: a broadcast
            const uint32_t tj = rj.y >> 31;
            const P a = mi * (P)(rj.y & 0x7FFFFFFFu), b = (P)rj.x * ni;
            g += a > b ? tj : 0u;
            c += a == b ? tj : 0u;
            e += a == b ? 1u : 0u;
        };
        uint32_t j = 0;
        for (; j + RANK_UNROLL <= n; j += RANK_UNROLL) {
#pragma unroll
            for (uint32_t q = 0; q < RANK_UNROLL; q++) pair(j + q);
        }
        for (; j < n; j++) pair(j);
        const bool h1 = (ri.y >> 31) == 0u;           // only rows of haplotype 1 count against haplotype 2
        G += h1 ? g : 0u;
        E += h1 ? c : 0u;
        T += (uint64_t)e * e - 1ull;                  // e >= 1: the read itself
    }
}

// One workgroup's test of the position range [*p_ws, *p_we) over the reads
// [p_r0[0], p_r0[1]): pf_rank_test's whole body, shared with pf_rank_ranges.
// s_r holds cap counted reads, cap at least min(PF_RANK_READS, r1 - r0).  Every
// thread of the workgroup calls it.
__device__ __forceinline__ void rank_one(const pf_calls_view &v, uint32_t min_calls, uint32_t force_wide, uint2 *s_r,
                                         uint32_t cap, const uint32_t *p_ws, const uint32_t *p_we, const uint32_t *p_r0,
                                         rank_out *out) {
    __shared__ unsigned long long s_sum[4], s_N, s_acc[3];
    __shared__ uint32_t s_nr[2], s_short[2], s_cls[6], s_max, wsum[PF_RANK_THREADS_MAX / PF_WAVE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nt = blockDim.x, nw = nt >> 6;
    if (tid < 4u) s_sum[tid] = 0ull;
    if (tid < 3u) s_acc[tid] = 0ull;
    if (tid < 2u) { s_nr[tid] = 0u; s_short[tid] = 0u; }
    if (tid < 6u) s_cls[tid] = 0u;
    if (tid == 0u) { s_N = 0ull; s_max = 0u; }
    __syncthreads();

    // ---- phase 1: the counted reads in read order
    const uint32_t ws = *p_ws, we = *p_we;
    const uint32_t r0 = p_r0[0], r1 = p_r0[1];
    uint32_t n = 0;
    for (uint32_t g = r0; g < r1; g += nt) {          // the same rounds in every thread: barriers inside
        uint32_t hp, my_m, my_u, tot;
        bool hit;
        window_read_counts(v, g, r1, ws, we, tid, hp, hit, my_m, my_u);
        const uint32_t my_n = my_m + my_u;
        const bool part = hit && my_n != 0u;
        const bool counted = part && my_n >= min_calls;
        const uint32_t slot = block_compact(counted, wsum, nw, lane, wave, tot);
        if (part) atomicAdd(&s_N, (unsigned long long)my_n);
        if (part && !counted) atomicAdd(&s_short[hp], 1u);
        if (counted) {
            const uint32_t idx = n + slot;
            if (idx < cap) s_r[idx] = make_uint2(my_m, (my_n & 0x7FFFFFFFu) | (hp << 31));
            atomicAdd(&s_sum[2u * hp], (unsigned long long)my_m);
            atomicAdd(&s_sum[2u * hp + 1u], (unsigned long long)my_u);
            atomicAdd(&s_nr[hp], 1u);
            atomicAdd(&s_cls[3u * hp + (my_u == 0u ? 0u : my_m == 0u ? 1u : 2u)], 1u);
            atomicMax(&s_max, my_n);
        }
        n += tot;
        __syncthreads();
    }

    const uint32_t n1 = s_nr[0], n2 = s_nr[1];
    const bool over = s_N >= 0x80000000ull;
    const uint32_t status = over ? RANK_ST_LIMIT : n > PF_RANK_READS ? 2u : (n1 == 0u || n2 == 0u) ? 1u : 0u;
    const bool wide = force_wide != 0u || s_max > PF_RANK_NARROW_MAX;

    // ---- phase 2: all pairs
    if (status == 0u) {
        uint64_t G = 0, E = 0, T = 0;
        if (wide) rank_rows<uint64_t>(s_r, n, tid, nt, G, E, T);
        else rank_rows<uint32_t>(s_r, n, tid, nt, G, E, T);
        G = wave_sum64(G);
        E = wave_sum64(E);
        T = wave_sum64(T);
        if (lane == 0u) {
            if (G) atomicAdd(&s_acc[0], (unsigned long long)G);
            if (E) atomicAdd(&s_acc[1], (unsigned long long)E);
            if (T) atomicAdd(&s_acc[2], (unsigned long long)T);
        }
    }
    __syncthreads();
    if (tid == 0u) {
        rank_out o;
        for (int k = 0; k < 4; k++) o.sum[k] = s_sum[k];
        o.u2 = 2ull * s_acc[0] + s_acc[1];
        o.ties = s_acc[2];
        o.n_reads[0] = n1; o.n_reads[1] = n2;
        o.n_short[0] = s_short[0]; o.n_short[1] = s_short[1];
        for (int k = 0; k < 6; k++) o.cls[k] = s_cls[k];
        o.status = status;
        o.wide = wide ? 1u : 0u;
        *out = o;
    }
}

struct rankr_args {
    uint32_t W, n_rng, min_calls, force_wide, cap, pad;
    pf_calls_view v;                                 /* read_hp: the batch's tags or the caller's */
    const uint64_t *rng_off;                         /* [W + 1] */
    const uint32_t *rng_start, *rng_end;             /* [n_rng] */
    rank_out *out;                                   /* [n_rng] */
};

}  // namespace

__global__ __launch_bounds__(PF_RANK_THREADS_MAX) void pf_rank_test(rank_args a) {
    __shared__ uint2 s_r[PF_RANK_READS];             // per counted read: m, n | tag << 31
    const uint32_t w = blockIdx.x;
    if (w >= a.W) return;
    rank_one(a.v, a.min_calls, a.force_wide, s_r, PF_RANK_READS, a.v.win_start + w, a.v.win_end + w, a.v.win_read_off + w,
             a.out + w);
}

// ---- the same test over position ranges inside the windows (pf_batch_rankranges)
//
// One workgroup per range.  The range's window is the w with rng_off[w] <= i <
// rng_off[w + 1], found by binary search (windows without a range are stepped
// over: the search looks for the first offset above i).  The counted reads lie
// in dynamic LDS, 8 B times a.cap.
__global__ __launch_bounds__(PF_RANK_THREADS_MAX) void pf_rank_ranges(rankr_args a) {
    extern __shared__ uint2 s_dyn[];
    const uint32_t i = blockIdx.x;
    if (i >= a.n_rng) return;
    uint32_t lo = 0, hi = a.W;                        // the first w in [0, W) with rng_off[w + 1] > i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.rng_off[mid + 1] > (uint64_t)i) hi = mid; else lo = mid + 1;
    }
    if (lo >= a.W) return;                            // not reached: rng_off[W] == n_rng > i
    rank_one(a.v, a.min_calls, a.force_wide, s_dyn, a.cap, a.rng_start + i, a.rng_end + i, a.v.win_read_off + lo, a.out + i);
}

// ---- the exact test
namespace {

// r_i of the rows tid, tid + nt, ... of the n <= 64 counted reads in s_r; s_v[h] collects the r_i of the reads tagged h
template <typename P>
__device__ __forceinline__ void rankx_midranks(const uint2 *s_r, uint32_t n, uint32_t tid, uint32_t nt, uint32_t *s_rv,
                                               uint32_t *s_v) {
    for (uint32_t i = tid; i < n; i += nt) {
        const uint2 ri = s_r[i];
        const P mi = (P)ri.x, ni = (P)(ri.y & 0x7FFFFFFFu);
        uint32_t l = 0, t = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint2 rj = s_r[j];                  // a broadcast
            const P a = mi * (P)(rj.y & 0x7FFFFFFFu), b = (P)rj.x * ni;
            l += a > b ? 1u : 0u;                     // f_j < f_i
            t += a == b ? 1u : 0u;
        }
        const uint32_t r = 2u * l + t;
        s_rv[i] = r;
        atomicAdd(&s_v[ri.y >> 31], r);
    }
}

// Phases 3 and 4 on the table T (LDS or the slab; inlined per address space):
// every thread of the workgroup calls this, acc[4] collects total, le, ge, two
// of row k against v0, the observed value of the class that is counted.
__device__ __forceinline__ void rankx_table(uint64_t *T, const uint32_t *s_rv, int n, int k, int64_t v0, int64_t a12,
                                            uint32_t tid, uint32_t nt, unsigned long long *acc) {
    const uint32_t cells = rankx_off((uint32_t)n, (uint32_t)k + 1u);
    for (uint32_t x = tid; x < cells; x += nt) T[x] = x == 0u ? 1ull : 0ull;
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const int r = (int)s_rv[i];
        const int c_hi = i + 1 < k ? i + 1 : k, c_lo = k - (n - 1 - i) > 1 ? k - (n - 1 - i) : 1;
        for (int c = c_hi; c >= c_lo; c--) {          // uniform bounds: the barrier is met by every thread
            const int sq = c * c, lo_p = (c - 1) * (c - 1), hi_p = (c - 1) * (2 * n - c + 1), len = 2 * c * (n - c) + 1;
            const int x0 = r + lo_p - sq > 0 ? r + lo_p - sq : 0, x1 = r + hi_p - sq < len - 1 ? r + hi_p - sq : len - 1;
            uint64_t *row = T + rankx_off((uint32_t)n, (uint32_t)c);
            const uint64_t *prev = T + rankx_off((uint32_t)n, (uint32_t)c - 1u);
            for (int x = x0 + (int)tid; x <= x1; x += (int)nt) row[x] += prev[x + sq - r - lo_p];
            __syncthreads();                          // row c - 1 is written only after row c has read it
        }
    }
    const uint64_t *row = T + rankx_off((uint32_t)n, (uint32_t)k);
    const int len = 2 * k * (n - k) + 1;
    const int64_t d0 = v0 > a12 ? v0 - a12 : a12 - v0;
    uint64_t tot = 0, le = 0, ge = 0, two = 0;
    for (int x = (int)tid; x < len; x += (int)nt) {
        const uint64_t cnt = row[x];
        const int64_t v = (int64_t)x, d = v > a12 ? v - a12 : a12 - v;
        tot += cnt;
        le += v <= v0 ? cnt : 0ull;
        ge += v >= v0 ? cnt : 0ull;
        two += d >= d0 ? cnt : 0ull;
    }
    tot = wave_sum64(tot);
    le = wave_sum64(le);
    ge = wave_sum64(ge);
    two = wave_sum64(two);
    if ((tid & 63u) == 0u) {
        if (tot) atomicAdd(&acc[0], (unsigned long long)tot);
        if (le) atomicAdd(&acc[1], (unsigned long long)le);
        if (ge) atomicAdd(&acc[2], (unsigned long long)ge);
        if (two) atomicAdd(&acc[3], (unsigned long long)two);
    }
}

}  // namespace

__global__ __launch_bounds__(PF_RANK_THREADS_MAX) void pf_rank_exact(rankx_args a) {
    __shared__ uint64_t s_buf[PF_RANKX_LDS_CELLS];   // the counted reads (m, n | tag << 31), then the table
    __shared__ unsigned long long s_N, s_acc[4], s_ge[2];
    __shared__ uint32_t s_nr[2], s_short[2], s_v[2], s_max, s_rv[PF_RANKX_READS], wsum[PF_RANK_THREADS_MAX / PF_WAVE];
    static_assert(PF_RANKX_LDS_CELLS >= PF_RANK_READS, "s_buf holds the reads pf_rank_test holds");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nt = blockDim.x, nw = nt >> 6;
    uint2 *s_r = reinterpret_cast<uint2 *>(s_buf);
    for (uint32_t w = blockIdx.x; w < a.W; w += gridDim.x) {
        if (tid < 4u) s_acc[tid] = 0ull;
        if (tid < 2u) { s_nr[tid] = 0u; s_short[tid] = 0u; s_v[tid] = 0u; s_ge[tid] = 0ull; }
        if (tid == 0u) { s_N = 0ull; s_max = 0u; }
        __syncthreads();

        // ---- phase 1: the counted reads in read order, as in pf_rank_test
        const uint32_t ws = a.v.win_start[w], we = a.v.win_end[w];
        const uint32_t r0 = a.v.win_read_off[w], r1 = a.v.win_read_off[w + 1];
        uint32_t n = 0;
        for (uint32_t g = r0; g < r1; g += nt) {
            uint32_t hp, my_m, my_u, tot;
            bool hit;
            window_read_counts(a.v, g, r1, ws, we, tid, hp, hit, my_m, my_u);
            const uint32_t my_n = my_m + my_u;
            const bool part = hit && my_n != 0u;
            const bool counted = part && my_n >= a.min_calls;
            const uint32_t slot = block_compact(counted, wsum, nw, lane, wave, tot);
            if (part) atomicAdd(&s_N, (unsigned long long)my_n);
            if (part && !counted) atomicAdd(&s_short[hp], 1u);
            if (counted) {
                const uint32_t idx = n + slot;
                if (idx < PF_RANK_READS) s_r[idx] = make_uint2(my_m, (my_n & 0x7FFFFFFFu) | (hp << 31));
                atomicAdd(&s_nr[hp], 1u);
                atomicMax(&s_max, my_n);
            }
            n += tot;
            __syncthreads();
        }
        const uint32_t n1 = s_nr[0], n2 = s_nr[1];
        const bool limit = s_N >= 0x80000000ull;
        const bool pairs = !limit && n <= PF_RANK_READS && n1 != 0u && n2 != 0u;      // pf_rank_test's status 0
        const uint32_t status = limit ? RANK_ST_LIMIT : n > a.max_reads ? 2u : (n1 == 0u || n2 == 0u) ? 1u : 0u;
        const bool wide = s_max > PF_RANK_NARROW_MAX;
        const uint32_t k = n1 <= n2 ? n1 : n2;
        const bool swap = n2 < n1;                    // the reads tagged 1 are the smaller class
        const bool hbm = status == 0u && (a.force_hbm != 0u || rankx_off(n, k + 1u) > PF_RANKX_LDS_CELLS);

        // ---- phase 2
        if (status == 0u) {
            if (wide) rankx_midranks<uint64_t>(s_r, n, tid, nt, s_rv, s_v);
            else rankx_midranks<uint32_t>(s_r, n, tid, nt, s_rv, s_v);
        } else if (pairs) {                           // over max_reads: u2 alone, as pf_rank_test has it
            uint64_t G = 0, E = 0, T = 0;
            if (wide) rank_rows<uint64_t>(s_r, n, tid, nt, G, E, T);
            else rank_rows<uint32_t>(s_r, n, tid, nt, G, E, T);
            G = wave_sum64(G);
            E = wave_sum64(E);
            if (lane == 0u) {
                if (G) atomicAdd(&s_ge[0], (unsigned long long)G);
                if (E) atomicAdd(&s_ge[1], (unsigned long long)E);
            }
        }
        __syncthreads();                              // the reads are done with: the table may take s_buf

        // ---- phases 3 and 4
        const int64_t a12 = (int64_t)n1 * (int64_t)n2;
        const int64_t v0 = status == 0u ? (int64_t)s_v[swap ? 1u : 0u] - (int64_t)k * (int64_t)k : 0;
        if (status == 0u) {
            if (hbm) rankx_table(a.slab + (size_t)blockIdx.x * a.slab_cells, s_rv, (int)n, (int)k, v0, a12, tid, nt, s_acc);
            else rankx_table(s_buf, s_rv, (int)n, (int)k, v0, a12, tid, nt, s_acc);
        }
        __syncthreads();
        if (tid == 0u) {
            rankx_out o;
            o.u2 = status == 0u ? (uint64_t)(swap ? 2 * a12 - v0 : v0) : pairs ? 2ull * s_ge[0] + s_ge[1] : 0ull;
            o.total = s_acc[0];
            o.le = swap ? s_acc[2] : s_acc[1];
            o.ge = swap ? s_acc[1] : s_acc[2];
            o.two = s_acc[3];
            o.n_reads[0] = n1; o.n_reads[1] = n2;
            o.n_short[0] = s_short[0]; o.n_short[1] = s_short[1];
            o.status = status;
            o.hbm = hbm ? 1u : 0u;
            a.out[w] = o;
        }
        __syncthreads();                              // the next window clears what thread 0 has just read
    }
}

// ---- host side
extern "C" void pf_rank_free(pf_rank_t *p) {
    if (!p) return;
    free(const_cast<uint32_t *>(p->n_reads));
    free(const_cast<uint32_t *>(p->n_short));
    free(const_cast<uint32_t *>(p->cls));
    free(const_cast<uint64_t *>(p->sum));
    free(const_cast<uint64_t *>(p->u2));
    free(const_cast<uint64_t *>(p->ties));
    free(const_cast<uint32_t *>(p->status));
    free(p);
}

// PF_RANK_WIDE: unset or "0" 0, "1" 1 (64-bit products for every window), anything else -1
static int rank_wide() {
    const char *e = getenv("PF_RANK_WIDE");
    if (!e || !strcmp(e, "0")) return 0;
    if (!strcmp(e, "1")) return 1;
    return -1;
}

// a result of n entries with every array allocated and zeroed; NULL: no memory
static pf_rank_t *rank_result_new(uint32_t n, uint32_t min_calls) {
    pf_rank_t *res = (pf_rank_t *)calloc(1, sizeof(pf_rank_t));
    if (!res) return nullptr;
    res->n_windows = n;
    res->min_calls = min_calls;
    if (n == 0) return res;
    res->n_reads = (uint32_t *)calloc(2ull * n, 4); res->n_short = (uint32_t *)calloc(2ull * n, 4);
    res->cls = (uint32_t *)calloc(6ull * n, 4); res->status = (uint32_t *)calloc(n, 4);
    res->sum = (uint64_t *)calloc(4ull * n, 8); res->u2 = (uint64_t *)calloc(n, 8); res->ties = (uint64_t *)calloc(n, 8);
    if (!res->n_reads || !res->n_short || !res->cls || !res->status || !res->sum || !res->u2 || !res->ties) {
        pf_rank_free(res);
        return nullptr;
    }
    return res;
}

// the kernels' records into the result's arrays; PF_ERR_LIMIT where one holds 2^31 or more calls
static int rank_result_fill(pf_rank_t *res, const std::vector<rank_out> &h_out, const char *what) {
    uint32_t *h_nr = const_cast<uint32_t *>(res->n_reads), *h_short = const_cast<uint32_t *>(res->n_short);
    uint32_t *h_cls = const_cast<uint32_t *>(res->cls), *h_stat = const_cast<uint32_t *>(res->status);
    uint64_t *h_sum = const_cast<uint64_t *>(res->sum), *h_u2 = const_cast<uint64_t *>(res->u2);
    uint64_t *h_ties = const_cast<uint64_t *>(res->ties);
    for (uint32_t w = 0; w < res->n_windows; w++) {
        const rank_out &o = h_out[w];
        if (o.status == RANK_ST_LIMIT) {
            fprintf(stderr, "[E::pomfret_amd] %s holds 2^31 or more calls\n", what);
            return PF_ERR_LIMIT;
        }
        for (int k = 0; k < 4; k++) h_sum[4ull * w + k] = o.sum[k];
        for (int k = 0; k < 2; k++) { h_nr[2ull * w + k] = o.n_reads[k]; h_short[2ull * w + k] = o.n_short[k]; }
        for (int k = 0; k < 6; k++) h_cls[6ull * w + k] = o.cls[k];
        h_u2[w] = o.u2;
        h_ties[w] = o.ties;
        h_stat[w] = o.status;
    }
    return PF_OK;
}

// PF_RANKR_LDS_FIXED: unset or "0" 0, "1" 1 (pf_rank_ranges takes pf_rank_test's 32 KB whatever the batch), anything else -1
static int rankr_lds_fixed() {
    const char *e = getenv("PF_RANKR_LDS_FIXED");
    if (!e || !strcmp(e, "0")) return 0;
    if (!strcmp(e, "1")) return 1;
    return -1;
}

extern "C" int pf_batch_ranktest(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                                 pf_rank_t **out) {
    if (!ctx || !db || !out) return PF_ERR_ARG;
    *out = nullptr;
    if (min_calls < 1u || min_calls > 65535u) return PF_ERR_ARG;
    const uint32_t nt = pf_env_threads("PF_RANK_THREADS", PF_RANK_THREADS);
    const int fw = rank_wide();
    if (!nt || fw < 0) return PF_ERR_ARG;
    pf_dev_batch d;
    const int vrc = pf_batch_calls_view(ctx, db, &d);
    if (vrc) return vrc;
    const uint32_t W = d.W, R = d.R;
    if (read_hp && n_hp != R) return PF_ERR_ARG;

    pf_rank_t *res = rank_result_new(W, min_calls);
    if (!res) return PF_ERR_NOMEM;
    if (W == 0) { *out = res; return PF_OK; }
    std::unique_ptr<pf_rank_t, void (*)(pf_rank_t *)> own(res, pf_rank_free);      // freed on every return but the last
    std::vector<rank_out> h_out;
    try { h_out.resize(W); } catch (...) { return PF_ERR_NOMEM; }
    pf_call call(pf_ctx_stream(ctx));
    rank_args a;
    memset(&a, 0, sizeof a);
    a.W = W; a.min_calls = min_calls; a.force_wide = (uint32_t)fw;
    a.v = pf_calls_view_of(d);
    const int hrc = call.upload_hp(read_hp, R, a.v);
    if (hrc) return hrc;
    a.out = static_cast<rank_out *>(call.alloc(sizeof(rank_out) * (size_t)W));
    if (!a.out) return PF_ERR_NOMEM;
    if (!call.mark(0)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_rank_test, dim3(W), dim3(nt), 0, call.st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(h_out.data(), a.out, sizeof(rank_out) * (size_t)W, hipMemcpyDeviceToHost, call.st) != hipSuccess ||
        hipStreamSynchronize(call.st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_kernels = call.ms(0, 1);
    const int frc = rank_result_fill(res, h_out, "ranktest: a window");
    if (frc) return frc;
    *out = own.release();
    return PF_OK;
}

// pf_batch_rankranges, and with loaded != 0 the entry for a caller that has
// just run another consumer on the same batch (pf_batch_rankranges_loaded):
// the calls are taken as they stand.
static int rank_ranges_run(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                           const uint64_t *rng_off, const uint32_t *rng_start, const uint32_t *rng_end, pf_rank_t **out,
                           int loaded) {
    if (!ctx || !db || !out) return PF_ERR_ARG;
    *out = nullptr;
    if (min_calls < 1u || min_calls > 65535u) return PF_ERR_ARG;
    const uint32_t nt = pf_env_threads("PF_RANK_THREADS", PF_RANK_THREADS);
    const int fw = rank_wide(), fl = rankr_lds_fixed();
    if (!nt || fw < 0 || fl < 0) return PF_ERR_ARG;
    pf_dev_batch d;
    const int vrc = loaded ? pf_batch_calls_loaded(ctx, db, &d) : pf_batch_calls_view(ctx, db, &d);
    if (vrc) return vrc;
    const uint32_t W = d.W, R = d.R;
    if (read_hp && n_hp != R) return PF_ERR_ARG;
    if (W && !rng_off) return PF_ERR_ARG;
    uint64_t n64 = 0;
    if (W) {
        if (rng_off[0] != 0) return PF_ERR_ARG;
        for (uint32_t w = 0; w < W; w++)
            if (rng_off[w + 1] < rng_off[w]) return PF_ERR_ARG;
        n64 = rng_off[W];
    }
    if (n64 > 0x7FFFFFFFull || (n64 && (!rng_start || !rng_end))) return PF_ERR_ARG;
    const uint32_t n = (uint32_t)n64;
    if (n64 * nt > 0xFFFFFFFFull) {                  // one workgroup per range: a launch holds fewer than 2^32 threads
        fprintf(stderr, "[E::pomfret_amd] rankranges: %u ranges at %u threads each pass 2^32 threads in one launch\n", n, nt);
        return PF_ERR_LIMIT;
    }
    hipStream_t st = pf_ctx_stream(ctx);

    // every range inside its window; the LDS array after the largest window's reads
    uint32_t max_reads = 0;
    if (n) {
        std::vector<uint32_t> hws, hwe, hro;
        try { hws.resize(W); hwe.resize(W); hro.resize((size_t)W + 1); } catch (...) { return PF_ERR_NOMEM; }
        if (hipMemcpyAsync(hws.data(), d.win_start, 4ull * W, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(hwe.data(), d.win_end, 4ull * W, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(hro.data(), d.win_read_off, 4ull * (W + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PF_ERR_HIP;
        for (uint32_t w = 0; w < W; w++) {
            for (uint64_t i = rng_off[w]; i < rng_off[w + 1]; i++)
                if (rng_start[i] < hws[w] || rng_end[i] < rng_start[i] || rng_end[i] > hwe[w]) return PF_ERR_ARG;
            if (hro[w + 1] < hro[w] || hro[w + 1] > R) return PF_ERR_INTERNAL;
            if (rng_off[w + 1] > rng_off[w] && hro[w + 1] - hro[w] > max_reads) max_reads = hro[w + 1] - hro[w];
        }
    }

    pf_rank_t *res = rank_result_new(n, min_calls);
    if (!res) return PF_ERR_NOMEM;
    if (n == 0) { *out = res; return PF_OK; }
    std::unique_ptr<pf_rank_t, void (*)(pf_rank_t *)> own(res, pf_rank_free);      // freed on every return but the last
    std::vector<rank_out> h_out;
    try { h_out.resize(n); } catch (...) { return PF_ERR_NOMEM; }
    pf_call call(st);
    rankr_args a;
    memset(&a, 0, sizeof a);
    a.W = W; a.n_rng = n; a.min_calls = min_calls; a.force_wide = (uint32_t)fw;
    // min(PF_RANK_READS, the reads of the largest window with a range), as a power of two, one wave's reads at least
    a.cap = 64u;
    while (a.cap < PF_RANK_READS && a.cap < max_reads) a.cap <<= 1;
    if (fl) a.cap = PF_RANK_READS;
    a.v = pf_calls_view_of(d);
    const int hrc = call.upload_hp(read_hp, R, a.v);
    if (hrc) return hrc;
    void *p_off = call.alloc(8ull * ((size_t)W + 1)), *p_s = call.alloc(4ull * n), *p_e = call.alloc(4ull * n);
    a.out = static_cast<rank_out *>(call.alloc(sizeof(rank_out) * (size_t)n));
    if (!p_off || !p_s || !p_e || !a.out) return PF_ERR_NOMEM;
    a.rng_off = static_cast<const uint64_t *>(p_off);
    a.rng_start = static_cast<const uint32_t *>(p_s);
    a.rng_end = static_cast<const uint32_t *>(p_e);
    if (hipMemcpyAsync(p_off, rng_off, 8ull * ((size_t)W + 1), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(p_s, rng_start, 4ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(p_e, rng_end, 4ull * n, hipMemcpyHostToDevice, st) != hipSuccess || !call.mark(0))
        return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_rank_ranges, dim3(n), dim3(nt), sizeof(uint2) * (size_t)a.cap, st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(h_out.data(), a.out, sizeof(rank_out) * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_kernels = call.ms(0, 1);
    const int frc = rank_result_fill(res, h_out, "rankranges: a range");
    if (frc) return frc;
    *out = own.release();
    return PF_OK;
}

extern "C" int pf_batch_rankranges(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                                   const uint64_t *rng_off, const uint32_t *rng_start, const uint32_t *rng_end,
                                   pf_rank_t **out) {
    return rank_ranges_run(ctx, db, read_hp, n_hp, min_calls, rng_off, rng_start, rng_end, out, 0);
}

// ---- the same call on a batch whose load stage the caller has just run
// (pf_hapmeth.c, right after pf_batch_pileup): a record-level batch's loader is
// not run a second time.  Not part of the public header.
extern "C" int pf_batch_rankranges_loaded(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp,
                                          uint32_t min_calls, const uint64_t *rng_off, const uint32_t *rng_start,
                                          const uint32_t *rng_end, pf_rank_t **out) {
    return rank_ranges_run(ctx, db, read_hp, n_hp, min_calls, rng_off, rng_start, rng_end, out, 1);
}

extern "C" void pf_rank_exact_free(pf_rank_exact_t *p) {
    if (!p) return;
    free(const_cast<uint32_t *>(p->n_reads));
    free(const_cast<uint32_t *>(p->n_short));
    free(const_cast<uint32_t *>(p->status));
    free(const_cast<uint64_t *>(p->u2));
    free(const_cast<uint64_t *>(p->total));
    free(const_cast<uint64_t *>(p->le));
    free(const_cast<uint64_t *>(p->ge));
    free(const_cast<uint64_t *>(p->two));
    free(p);
}

// PF_RANKX_HBM: unset or "0" 0, "1" 1 (every window's table in its slab), anything else -1
static int rankx_hbm() {
    const char *e = getenv("PF_RANKX_HBM");
    if (!e || !strcmp(e, "0")) return 0;
    if (!strcmp(e, "1")) return 1;
    return -1;
}

// PF_RANKX_GRID=<n>, 1 .. 65536 in digits alone: the most workgroups; the default where unset, 0 for any other value
static uint32_t rankx_grid() {
    const char *e = getenv("PF_RANKX_GRID");
    if (!e) return PF_RANKX_GRID;
    if (*e < '1' || *e > '9') return 0;
    char *end = nullptr;
    const long n = strtol(e, &end, 10);
    if (*end || n < 1 || n > 65536) return 0;
    return (uint32_t)n;
}

extern "C" int pf_batch_rankexact(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t min_calls,
                                  uint32_t max_reads, pf_rank_exact_t **out) {
    static_assert(PF_RANKX_READS == PF_RANK_EXACT_MAX_READS, "the kernel's r_i array holds exactly the documented limit");
    if (!ctx || !db || !out) return PF_ERR_ARG;
    *out = nullptr;
    if (min_calls < 1u || min_calls > 65535u) return PF_ERR_ARG;
    if (max_reads < 2u || max_reads > PF_RANK_EXACT_MAX_READS) return PF_ERR_ARG;
    const uint32_t nt = pf_env_threads("PF_RANKX_THREADS", PF_RANKX_THREADS);
    const int fh = rankx_hbm();
    const uint32_t G = rankx_grid();
    if (!nt || fh < 0 || !G) return PF_ERR_ARG;
    pf_dev_batch d;
    const int vrc = pf_batch_calls_view(ctx, db, &d);
    if (vrc) return vrc;
    const uint32_t W = d.W, R = d.R;
    if (read_hp && n_hp != R) return PF_ERR_ARG;

    pf_rank_exact_t *res = (pf_rank_exact_t *)calloc(1, sizeof(pf_rank_exact_t));
    if (!res) return PF_ERR_NOMEM;
    res->n_windows = W;
    res->min_calls = min_calls;
    res->max_reads = max_reads;
    if (W == 0) { *out = res; return PF_OK; }
    std::unique_ptr<pf_rank_exact_t, void (*)(pf_rank_exact_t *)> own(res, pf_rank_exact_free);
    uint32_t *h_nr = (uint32_t *)calloc(2ull * W, 4), *h_short = (uint32_t *)calloc(2ull * W, 4), *h_stat = (uint32_t *)calloc(W, 4);
    uint64_t *h_u2 = (uint64_t *)calloc(W, 8), *h_tot = (uint64_t *)calloc(W, 8), *h_le = (uint64_t *)calloc(W, 8);
    uint64_t *h_ge = (uint64_t *)calloc(W, 8), *h_two = (uint64_t *)calloc(W, 8);
    res->n_reads = h_nr; res->n_short = h_short; res->status = h_stat; res->u2 = h_u2; res->total = h_tot; res->le = h_le;
    res->ge = h_ge; res->two = h_two;
    if (!h_nr || !h_short || !h_stat || !h_u2 || !h_tot || !h_le || !h_ge || !h_two) return PF_ERR_NOMEM;
    std::vector<rankx_out> h_out;
    try { h_out.resize(W); } catch (...) { return PF_ERR_NOMEM; }
    pf_call call(pf_ctx_stream(ctx));
    rankx_args a;
    memset(&a, 0, sizeof a);
    a.W = W; a.min_calls = min_calls; a.max_reads = max_reads; a.force_hbm = (uint32_t)fh;
    a.v = pf_calls_view_of(d);
    const int hrc = call.upload_hp(read_hp, R, a.v);
    if (hrc) return hrc;
    a.out = static_cast<rankx_out *>(call.alloc(sizeof(rankx_out) * (size_t)W));
    if (!a.out) return PF_ERR_NOMEM;
    const uint32_t grid = W < G ? W : G;
    // the largest table max_reads allows; no slab where even that one fits in LDS
    a.slab_cells = rankx_off(max_reads, max_reads / 2u + 1u);
    if (fh || a.slab_cells > PF_RANKX_LDS_CELLS) {
        a.slab = static_cast<uint64_t *>(call.alloc(8ull * a.slab_cells * grid));
        if (!a.slab) return PF_ERR_NOMEM;
    }
    if (!call.mark(0)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_rank_exact, dim3(grid), dim3(nt), 0, call.st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(h_out.data(), a.out, sizeof(rankx_out) * (size_t)W, hipMemcpyDeviceToHost, call.st) != hipSuccess ||
        hipStreamSynchronize(call.st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_kernels = call.ms(0, 1);
    for (uint32_t w = 0; w < W; w++) {
        const rankx_out &o = h_out[w];
        if (o.status == RANK_ST_LIMIT) {
            fprintf(stderr, "[E::pomfret_amd] rankexact: a window holds 2^31 or more calls\n");
            return PF_ERR_LIMIT;
        }
        for (int k = 0; k < 2; k++) { h_nr[2ull * w + k] = o.n_reads[k]; h_short[2ull * w + k] = o.n_short[k]; }
        h_stat[w] = o.status;
        h_u2[w] = o.u2;
        h_tot[w] = o.total; h_le[w] = o.le; h_ge[w] = o.ge; h_two[w] = o.two;
    }
    *out = own.release();
    return PF_OK;
}
