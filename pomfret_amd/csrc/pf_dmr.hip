// pf_dmr.hip -- allele-specific methylated regions of a pileup (pf_dmr_regions).
//
// A segmented scan over the position-sorted sites of a pileup's windows: the
// informative sites (both haplotypes covered) carry a sign, consecutive
// informative sites of one non-zero sign within max_gap and with no break
// between them chain into a run, and each run leaves one record (include/
// pomfret_amd.h has the rules).  All integer.
//
// Any stretch of sites is summarised by one dmr_agg: its first and its last
// informative site (position, sign, break rank), the run that holds the first
// (the prefix run: whether it goes on to the left is not known inside the
// stretch), the run that holds the last (the suffix run, open to the right),
// whether the two are one run, and the number of kept runs closed in between.
// Two neighbouring stretches combine into one under the join rule alone, and
// that operator is associative, so the aggregate of the whole range does not
// depend on how it was cut: not on the block, not on the launch.
//
//   pf_dmr_count  one workgroup per block of B sites: each thread folds its
//                 B / PF_DMR_THREADS consecutive sites, the wave scans the
//                 threads' aggregates with __shfl_up, the waves meet in LDS;
//                 the block's aggregate goes to agg[block];
//   pf_dmr_scan   one workgroup turns agg[] into its exclusive prefix (each
//                 block's carry-in) and leaves the totals: records, informative;
//   pf_dmr_emit   rebuilds each thread's carry-in and replays its sites: an
//                 informative site that does not join closes the run before it,
//                 whose record index is the number of records final before it
//                 (the prefix run once it is closed, plus the kept closed
//                 runs) -- exact, no atomics, no guess.  The last thread of
//                 the last block writes the run that is still open at the end.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <memory>
#include "pf_device.h"
#include "pf_site.h"
#include "pf_call.h"
#include "../../include/pomfret_amd.h"

struct pf_ctx;
extern "C" int pf_ctx_device(const pf_ctx *c);
extern "C" hipStream_t pf_ctx_stream(const pf_ctx *c);

namespace {

// flags: bit 0 the stretch has an informative site, bit 1 all of them are one
// run, bits 2-3 the first one's sign, bits 4-5 the last one's (0 none, 1 +, 2 -)
struct dmr_agg {
    uint32_t flags;
    uint32_t f_pos, f_rank, l_pos, l_rank;
    uint32_t n_inf, closed;
    uint32_t p_n, p_last;          // prefix run: members, last member (it starts at f_pos)
    uint32_t s_n, s_start;         // suffix run: members, first member (it ends at l_pos)
    uint32_t pad;
    uint64_t p_sum[4], s_sum[4];
};
static_assert(sizeof(dmr_agg) == 112, "dmr_agg is shuffled and stored as 28 dwords");
struct dmr_raw { uint32_t w[28]; };

struct dmr_args {
    uint32_t n, B, K, n_blocks;    // sites, sites per block, sites per thread, blocks
    uint32_t min_cov, min_delta_pct, max_gap, min_sites;
    const uint32_t *pos;           // [n]
    const uint32_t *cnt;           // [n*6]
    const uint32_t *brk;           // [n_brk] ascending
    uint32_t n_brk;
    dmr_agg *agg;                  // [n_blocks]: the blocks' aggregates, then their exclusive prefix
    uint64_t *tot;                 // [2]: records, informative sites
    uint32_t *status;              // bit 0: positions not ascending, bit 1: a count above 65,535
    pf_dmr_run_t *out;             // [n_out]
    uint64_t n_out;
    const uint8_t *state;          // [n] pf_dmr_hmm_regions' runs only: a site's sign code, 255 a transparent site
};

__device__ __forceinline__ dmr_agg agg_none() {
    dmr_agg r;
    r.flags = 0; r.f_pos = r.f_rank = r.l_pos = r.l_rank = 0; r.n_inf = r.closed = 0;
    r.p_n = r.p_last = r.s_n = r.s_start = r.pad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) r.p_sum[k] = r.s_sum[k] = 0;
    return r;
}

__device__ __forceinline__ bool agg_joins(const dmr_agg &A, const dmr_agg &B, uint32_t max_gap) {
    const uint32_t ls = (A.flags >> 4) & 3u, fs = (B.flags >> 2) & 3u;
    return ls != 0u && ls == fs && B.f_pos - A.l_pos <= max_gap && A.l_rank == B.f_rank;
}

// records that nothing to the right can change any more
__device__ __forceinline__ uint32_t agg_final(const dmr_agg &A) {
    return ((A.p_n != 0u && !(A.flags & 2u)) ? 1u : 0u) + A.closed;
}

// A then B as one stretch.  Straight-line selects: an empty side (flags 0, all
// fields 0) leaves the other one unchanged.
__device__ __forceinline__ dmr_agg agg_combine(const dmr_agg &A, const dmr_agg &B, uint32_t max_gap, uint32_t min_sites) {
    const bool ha = A.flags & 1u, hb = B.flags & 1u, both = ha && hb;
    const bool aw = A.flags & 2u, bw = B.flags & 2u;
    const bool join = both && agg_joins(A, B, max_gap);      // A's suffix run and B's prefix run are one
    const bool mp = join && aw, ms = join && bw;             // ... and that one is the prefix / the suffix run
    const uint32_t mn = A.s_n + B.p_n;
    const uint32_t extra = join ? ((!aw && !bw && mn >= min_sites) ? 1u : 0u)
                                : ((!aw && A.s_n != 0u && A.s_n >= min_sites) ? 1u : 0u) +
                                  ((!bw && B.p_n != 0u && B.p_n >= min_sites) ? 1u : 0u);
    const bool whole = both ? (join && aw && bw) : (ha ? aw : bw);
    dmr_agg R;
    R.flags = ((ha || hb) ? 1u : 0u) | (whole ? 2u : 0u) | ((ha ? A.flags : B.flags) & 0xCu) | ((hb ? B.flags : A.flags) & 0x30u);
    R.f_pos = ha ? A.f_pos : B.f_pos;
    R.f_rank = ha ? A.f_rank : B.f_rank;
    R.l_pos = hb ? B.l_pos : A.l_pos;
    R.l_rank = hb ? B.l_rank : A.l_rank;
    R.n_inf = A.n_inf + B.n_inf;
    R.closed = A.closed + B.closed + (both ? extra : 0u);
    R.p_n = mp ? mn : (ha ? A.p_n : B.p_n);
    R.p_last = mp ? B.p_last : (ha ? A.p_last : B.p_last);
    R.s_n = ms ? mn : (hb ? B.s_n : A.s_n);
    R.s_start = ms ? A.s_start : (hb ? B.s_start : A.s_start);
    R.pad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint64_t m = A.s_sum[k] + B.p_sum[k];
        R.p_sum[k] = mp ? m : (ha ? A.p_sum[k] : B.p_sum[k]);
        R.s_sum[k] = ms ? m : (hb ? B.s_sum[k] : A.s_sum[k]);
    }
    return R;
}

// field by field, so that the aggregate stays in registers
__device__ __forceinline__ dmr_agg agg_load(const dmr_agg *p) {
    dmr_agg r;
    r.flags = p->flags; r.f_pos = p->f_pos; r.f_rank = p->f_rank; r.l_pos = p->l_pos; r.l_rank = p->l_rank;
    r.n_inf = p->n_inf; r.closed = p->closed; r.p_n = p->p_n; r.p_last = p->p_last; r.s_n = p->s_n;
    r.s_start = p->s_start; r.pad = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { r.p_sum[k] = p->p_sum[k]; r.s_sum[k] = p->s_sum[k]; }
    return r;
}

__device__ __forceinline__ dmr_agg agg_shfl_up(const dmr_agg &v, uint32_t d) {
    const dmr_raw s = __builtin_bit_cast(dmr_raw, v);
    dmr_raw r;
#pragma unroll
    for (int k = 0; k < 28; k++) r.w[k] = (uint32_t)__shfl_up((int)s.w[k], d);
    return __builtin_bit_cast(dmr_agg, r);
}

// the exclusive prefix of the workgroup's aggregates in thread order
__device__ __forceinline__ dmr_agg block_exclusive(const dmr_agg &mine, dmr_agg *wtot, uint32_t max_gap, uint32_t min_sites) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    dmr_agg inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        dmr_agg o = agg_shfl_up(inc, d);
        if (lane < d) o = agg_none();                        // nothing to the left: the combine leaves inc as it is
        inc = agg_combine(o, inc, max_gap, min_sites);
    }
    if (lane == 63u) wtot[wave] = inc;
    __syncthreads();
    dmr_agg ex = agg_shfl_up(inc, 1);
    if (lane == 0u) ex = agg_none();
    dmr_agg pre = agg_none();
#pragma unroll
    for (uint32_t k = 0; k + 1 < PF_DMR_WAVES; k++) {
        dmr_agg w = agg_load(wtot + k);
        if (k >= wave) w = agg_none();
        pre = agg_combine(pre, w, max_gap, min_sites);
    }
    __syncthreads();
    return agg_combine(pre, ex, max_gap, min_sites);
}

// site i as an aggregate of its own; flags 0 when it is not informative.
// STATE: the sign is the site's entry of a.state (the range was checked when
// the states were made), not the delta rule's
template <bool STATE>
__device__ __forceinline__ dmr_agg site_agg(const dmr_args &a, uint32_t i, uint32_t &st) {
    dmr_agg r = agg_none();
    const uint32_t p = a.pos[i];
    if constexpr (STATE) {
        const uint32_t sg = a.state[i];
        if (sg > 2u) return r;
        uint32_t lo = 0, hi = a.n_brk;                       // breaks <= p
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.brk[mid] <= p) lo = mid + 1; else hi = mid;
        }
        r.flags = 1u | (sg ? 2u : 0u) | (sg << 2) | (sg << 4);
        r.f_pos = r.l_pos = p;
        r.f_rank = r.l_rank = lo;
        r.n_inf = 1;
        if (sg) {
            const uint2 c01 = *reinterpret_cast<const uint2 *>(a.cnt + 6ull * i);
            const uint2 c23 = *reinterpret_cast<const uint2 *>(a.cnt + 6ull * i + 2);
            r.p_n = r.s_n = 1;
            r.p_last = r.s_start = p;
            r.p_sum[0] = r.s_sum[0] = c01.x; r.p_sum[1] = r.s_sum[1] = c01.y;
            r.p_sum[2] = r.s_sum[2] = c23.x; r.p_sum[3] = r.s_sum[3] = c23.y;
        }
        return r;
    }
    const uint2 c01 = *reinterpret_cast<const uint2 *>(a.cnt + 6ull * i);
    const uint2 c23 = *reinterpret_cast<const uint2 *>(a.cnt + 6ull * i + 2);
    const uint32_t m1 = c01.x, u1 = c01.y, m2 = c23.x, u2 = c23.y;
    if (i > 0u && a.pos[i - 1] >= p) st |= 1u;
    if ((m1 | u1 | m2 | u2) > 0xFFFFu) { st |= 2u; return r; }
    const uint32_t n1 = m1 + u1, n2 = m2 + u2;
    if (!site_informative(n1, n2, a.min_cov)) return r;
    const uint32_t sg = site_sign(m1, n1, m2, n2, a.min_delta_pct);
    uint32_t lo = 0, hi = a.n_brk;                           // breaks <= p
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.brk[mid] <= p) lo = mid + 1; else hi = mid;
    }
    r.flags = 1u | (sg ? 2u : 0u) | (sg << 2) | (sg << 4);
    r.f_pos = r.l_pos = p;
    r.f_rank = r.l_rank = lo;
    r.n_inf = 1;
    if (sg) {
        r.p_n = r.s_n = 1;
        r.p_last = r.s_start = p;
        r.p_sum[0] = r.s_sum[0] = m1; r.p_sum[1] = r.s_sum[1] = u1;
        r.p_sum[2] = r.s_sum[2] = m2; r.p_sum[3] = r.s_sum[3] = u2;
    }
    return r;
}

// X's suffix run as a record
__device__ __forceinline__ void write_run(const dmr_args &a, const dmr_agg &X, uint32_t open) {
    const uint64_t idx = agg_final(X);
    if (idx >= a.n_out) return;                              // holds: both passes fold the same sites
    pf_dmr_run_t r;
    r.start = X.s_start;
    r.end = X.l_pos + 1u;
    r.n_sites = X.s_n;
    r.sign = ((X.flags >> 4) & 3u) == 1u ? 1 : -1;
#pragma unroll
    for (int k = 0; k < 4; k++) r.sum[k] = X.s_sum[k];
    r.open = open;
    r.reserved = 0;
    a.out[idx] = r;
}

template <bool EMIT, bool STATE>
__device__ __forceinline__ void dmr_block(const dmr_args &a) {
    __shared__ dmr_agg wtot[PF_DMR_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= a.n_blocks) return;
    // thread tid owns the block's sites [tid*K, +K)
    const uint64_t b0 = (uint64_t)blk * a.B;
    const uint64_t bend = b0 + a.B < a.n ? b0 + a.B : a.n;
    uint64_t i0 = b0 + (uint64_t)tid * a.K, i1 = i0 + a.K;
    if (i0 > bend) i0 = bend;
    if (i1 > bend) i1 = bend;
    uint32_t st = 0;
    dmr_agg X = agg_none();
    for (uint64_t i = i0; i < i1; i++) {
        const dmr_agg s = site_agg<STATE>(a, (uint32_t)i, st);
        X = agg_combine(X, s, a.max_gap, a.min_sites);
    }
    if (!EMIT && st) atomicOr(a.status, st);                 // the error path only
    const dmr_agg ex = block_exclusive(X, wtot, a.max_gap, a.min_sites);
    if (!EMIT) {
        if (tid == PF_DMR_THREADS - 1u) a.agg[blk] = agg_combine(ex, X, a.max_gap, a.min_sites);
        return;
    }
    X = agg_combine(agg_load(a.agg + blk), ex, a.max_gap, a.min_sites); // everything left of this thread's sites
    for (uint64_t i = i0; i < i1; i++) {
        const dmr_agg s = site_agg<STATE>(a, (uint32_t)i, st);
        if (!(s.flags & 1u)) continue;
        if ((X.flags & 1u) && X.s_n && !agg_joins(X, s, a.max_gap)) {
            const bool whole = X.flags & 2u;                 // the run that starts at the range's first informative site
            if (whole || X.s_n >= a.min_sites) write_run(a, X, whole ? PF_DMR_OPEN_LEFT : 0u);
        }
        X = agg_combine(X, s, a.max_gap, a.min_sites);
    }
    if (blk == a.n_blocks - 1u && tid == PF_DMR_THREADS - 1u && X.s_n)
        write_run(a, X, PF_DMR_OPEN_RIGHT | ((X.flags & 2u) ? PF_DMR_OPEN_LEFT : 0u));
}

}  // namespace

__global__ __launch_bounds__(PF_DMR_THREADS) void pf_dmr_count(dmr_args a) { dmr_block<false, false>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_dmr_emit(dmr_args a) { dmr_block<true, false>(a); }
// the same two passes over the states of pf_dmr_hmm_regions
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_dmr_count_state(dmr_args a) { dmr_block<false, true>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_dmr_emit_state(dmr_args a) { dmr_block<true, true>(a); }

// agg[b] <- the aggregate of the blocks before b; tot <- records, informative
// sites: one workgroup, each thread a contiguous run of blocks
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_dmr_scan(dmr_args a) {
    __shared__ dmr_agg wtot[PF_DMR_WAVES];
    const uint32_t tid = threadIdx.x, n = a.n_blocks;
    const uint32_t chunk = (n + PF_DMR_THREADS - 1u) / PF_DMR_THREADS;
    const uint64_t c0 = (uint64_t)tid * chunk;
    const uint32_t i0 = (uint32_t)(c0 < n ? c0 : n), i1 = (uint32_t)(c0 + chunk < n ? c0 + chunk : n);
    dmr_agg X = agg_none();
    for (uint32_t i = i0; i < i1; i++) X = agg_combine(X, agg_load(a.agg + i), a.max_gap, a.min_sites);
    dmr_agg c = block_exclusive(X, wtot, a.max_gap, a.min_sites);
    for (uint32_t i = i0; i < i1; i++) {
        const dmr_agg t = agg_load(a.agg + i);
        a.agg[i] = c;
        c = agg_combine(c, t, a.max_gap, a.min_sites);
    }
    if (tid == PF_DMR_THREADS - 1u) {                        // its chunk is the last: c is the whole range
        a.tot[0] = (uint64_t)agg_final(c) + (c.s_n ? 1u : 0u);
        a.tot[1] = c.n_inf;
    }
}

// ---- host side
extern "C" void pf_dmr_free(pf_dmr_t *d) {
    if (!d) return;
    free(const_cast<pf_dmr_run_t *>(d->runs));
    free(d);
}

extern "C" int pf_dmr_regions_block(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1,
                                    const pf_dmr_cfg_t *cfg, const uint32_t *breaks, uint32_t n_breaks, uint32_t block,
                                    pf_dmr_t **out) {
    if (!ctx || !pile || !cfg || !out || w1 < w0 || w1 > pile->n_windows || (w1 > w0 && !pile->win_off) ||
        (n_breaks && !breaks) || cfg->min_delta_pct > 100u)
        return PF_ERR_ARG;
    *out = nullptr;
    const uint32_t B = block ? block : pf_env_pow2("PF_DMR_BLOCK", 64, PF_DMR_BLOCK, PF_DMR_BLOCK);
    if (B < 64u || B > PF_DMR_BLOCK || (B & (B - 1u))) return PF_ERR_ARG;
    for (uint32_t i = 1; i < n_breaks; i++)
        if (breaks[i] < breaks[i - 1]) return PF_ERR_ARG;
    const uint64_t s0 = w1 > w0 ? pile->win_off[w0] : 0, s1 = w1 > w0 ? pile->win_off[w1] : 0;
    if (s1 < s0 || s1 > pile->n_sites || (s1 > s0 && (!pile->pos || !pile->cnt))) return PF_ERR_ARG;
    const uint64_t n = s1 - s0;
    if (n > 0x7FFFFFFFull) return PF_ERR_LIMIT;

    pf_dmr_t *res = (pf_dmr_t *)calloc(1, sizeof(pf_dmr_t));
    if (!res) return PF_ERR_NOMEM;
    if (n == 0) { *out = res; return PF_OK; }
    std::unique_ptr<pf_dmr_t, void (*)(pf_dmr_t *)> own(res, pf_dmr_free);     // freed on every return but the last
    if (hipSetDevice(pf_ctx_device(ctx)) != hipSuccess) return PF_ERR_HIP;
    uint64_t tot[2] = {0, 0};
    uint32_t stt = 0;
    pf_call call(pf_ctx_stream(ctx));
    hipStream_t st = call.st;
    dmr_args a;
    memset(&a, 0, sizeof a);
    a.n = (uint32_t)n; a.B = B; a.K = B > PF_DMR_THREADS ? B / PF_DMR_THREADS : 1u;
    a.n_blocks = (uint32_t)((n + B - 1) / B);
    a.min_cov = cfg->min_cov; a.min_delta_pct = cfg->min_delta_pct; a.max_gap = cfg->max_gap; a.min_sites = cfg->min_sites;
    a.n_brk = n_breaks;
    void *p_pos = nullptr, *p_cnt = nullptr, *p_brk = nullptr;
    if (!(p_pos = call.alloc(4ull * n)) || !(p_cnt = call.alloc(24ull * n)) || !(p_brk = call.alloc(4ull * n_breaks)) ||
        !(a.agg = static_cast<dmr_agg *>(call.alloc(sizeof(dmr_agg) * (size_t)a.n_blocks))) ||
        !(a.tot = static_cast<uint64_t *>(call.alloc(16))) || !(a.status = static_cast<uint32_t *>(call.alloc(8))))
        return PF_ERR_NOMEM;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipMemcpyAsync(p_pos, pile->pos + s0, 4ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(p_cnt, pile->cnt + 6ull * s0, 24ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_breaks && hipMemcpyAsync(p_brk, breaks, 4ull * n_breaks, hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    a.pos = static_cast<const uint32_t *>(p_pos);
    a.cnt = static_cast<const uint32_t *>(p_cnt);
    a.brk = static_cast<const uint32_t *>(p_brk);
    if (hipMemsetAsync(a.status, 0, 8, st) != hipSuccess || !call.mark(0)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_dmr_count, dim3(a.n_blocks), dim3(PF_DMR_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_dmr_scan, dim3(1), dim3(PF_DMR_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(tot, a.tot, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&stt, a.status, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    if (stt & 1u) return PF_ERR_ARG;                          // positions not ascending over the range
    if (stt & 2u) return PF_ERR_LIMIT;
    float ms1 = 0.0f;
    if (tot[0]) {
        pf_dmr_run_t *h = (pf_dmr_run_t *)malloc(sizeof(pf_dmr_run_t) * (size_t)tot[0]);
        res->runs = h;
        if (!h || !(a.out = static_cast<pf_dmr_run_t *>(call.alloc(sizeof(pf_dmr_run_t) * (size_t)tot[0])))) return PF_ERR_NOMEM;
        a.n_out = tot[0];
        if (!call.mark(2)) return PF_ERR_HIP;
        hipLaunchKernelGGL(pf_dmr_emit, dim3(a.n_blocks), dim3(PF_DMR_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess || !call.mark(3) ||
            hipMemcpyAsync(h, a.out, sizeof(pf_dmr_run_t) * (size_t)tot[0], hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PF_ERR_HIP;
        ms1 = call.ms(2, 3);
    }
    res->n_runs = tot[0];
    res->n_informative = tot[1];
    res->ms_kernels = call.ms(0, 1) + ms1;
    *out = own.release();
    return PF_OK;
}

extern "C" int pf_dmr_regions(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                              const uint32_t *breaks, uint32_t n_breaks, pf_dmr_t **out) {
    return pf_dmr_regions_block(ctx, pile, w0, w1, cfg, breaks, n_breaks, 0, out);
}

// pf_dmr_hmm.hip's run extraction: the three passes above over arrays that are
// on the device already, the sign of a site taken from d_state.  Enqueues on
// ctx's stream and waits; *runs is malloc'ed, exactly sized, with the open bits
// of pf_dmr_regions (the caller closes and filters them).
int pf_dmr_state_runs(pf_ctx_t *ctx, const uint32_t *d_pos, const uint32_t *d_cnt, const uint32_t *d_brk, uint32_t n_brk,
                      const uint8_t *d_state, uint32_t n, uint32_t B, const pf_dmr_cfg_t *cfg, pf_dmr_run_t **runs,
                      uint64_t *n_runs, float *ms) {
    *runs = nullptr; *n_runs = 0; *ms = 0.0f;
    if (n == 0) return PF_OK;
    std::unique_ptr<pf_dmr_run_t, void (*)(void *)> h(nullptr, free);
    uint64_t tot[2] = {0, 0};
    pf_call call(pf_ctx_stream(ctx));
    hipStream_t st = call.st;
    dmr_args a;
    memset(&a, 0, sizeof a);
    a.n = n; a.B = B; a.K = B > PF_DMR_THREADS ? B / PF_DMR_THREADS : 1u;
    a.n_blocks = (uint32_t)(((uint64_t)n + B - 1) / B);
    a.min_cov = cfg->min_cov; a.min_delta_pct = cfg->min_delta_pct; a.max_gap = cfg->max_gap; a.min_sites = cfg->min_sites;
    a.pos = d_pos; a.cnt = d_cnt; a.brk = d_brk; a.n_brk = n_brk; a.state = d_state;
    if (!(a.agg = static_cast<dmr_agg *>(call.alloc(sizeof(dmr_agg) * (size_t)a.n_blocks))) ||
        !(a.tot = static_cast<uint64_t *>(call.alloc(16))) || !(a.status = static_cast<uint32_t *>(call.alloc(8))))
        return PF_ERR_NOMEM;
    if (hipMemsetAsync(a.status, 0, 8, st) != hipSuccess || !call.mark(0)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_dmr_count_state, dim3(a.n_blocks), dim3(PF_DMR_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_dmr_scan, dim3(1), dim3(PF_DMR_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(tot, a.tot, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    float ms1 = 0.0f;
    if (tot[0]) {
        h.reset((pf_dmr_run_t *)malloc(sizeof(pf_dmr_run_t) * (size_t)tot[0]));
        if (!h || !(a.out = static_cast<pf_dmr_run_t *>(call.alloc(sizeof(pf_dmr_run_t) * (size_t)tot[0])))) return PF_ERR_NOMEM;
        a.n_out = tot[0];
        if (!call.mark(2)) return PF_ERR_HIP;
        hipLaunchKernelGGL(pf_dmr_emit_state, dim3(a.n_blocks), dim3(PF_DMR_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess || !call.mark(3) ||
            hipMemcpyAsync(h.get(), a.out, sizeof(pf_dmr_run_t) * (size_t)tot[0], hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PF_ERR_HIP;
        ms1 = call.ms(2, 3);
    }
    *ms = call.ms(0, 1) + ms1;
    *n_runs = tot[0];
    *runs = h.release();
    return PF_OK;
}
