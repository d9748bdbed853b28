// pf_regions.hip -- the per-haplotype sums of caller-given regions over a pileup
// (pf_region_sums).
//
// Every field of a region's record is a sum over the sites it holds, so the
// record of [start, end) is the difference of two prefixes of the
// position-sorted sites: the one before the first site at or past end and the
// one before the first site at or past start.  The prefixes are made once for
// the whole range; after that a region costs two binary searches and two rows,
// whether it overlaps, nests in or repeats another one.  All integer, exact,
// and the same for any block.
//
//   pf_reg_count   one workgroup per block of B sites: each thread folds its
//                  B / PF_DMR_THREADS consecutive sites into one reg_agg, the
//                  wave scans with __shfl_up, the waves meet in LDS; the block's
//                  total goes to blk[block];
//   pf_reg_scan    one workgroup turns blk[] into its exclusive prefix and
//                  leaves the range's total: row[n] and tot;
//   pf_reg_prefix  rebuilds each thread's carry-in and writes the exclusive
//                  prefix in front of every site: row[i], one 64-byte row each
//                  (52 bytes used), so that the lookup reads two whole rows;
//   pf_reg_lookup  one lane per region: lo = lower_bound(pos, start), hi =
//                  lower_bound(pos, end), the record is row[hi] - row[lo] and
//                  n_cpg = hi - lo.  No atomics, nothing sized by a guess.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <memory>
#include "pf_device.h"
#include "pf_llr.h"
#include "pf_site.h"
#include "pf_call.h"
#include "../../include/pomfret_amd.h"

struct pf_ctx;
extern "C" int pf_ctx_device(const pf_ctx *c);
extern "C" hipStream_t pf_ctx_stream(const pf_ctx *c);

namespace {

// the sums of a stretch of sites; also a row of the prefix table
struct alignas(16) reg_agg {
    uint32_t n_sites, n_pos, n_neg, pad0;
    uint64_t sum[4];
    int64_t ev;
    uint64_t pad1;
};
static_assert(sizeof(reg_agg) == 64, "one 64-byte row per site boundary");

struct alignas(8) reg_cnt4 { uint32_t m1, u1, m2, u2; };     // cnt[6*i .. 6*i+3]: 24-byte stride, 8-byte aligned

struct reg_args {
    uint32_t n, B, K, n_blocks;    // sites, sites per block, sites per thread, blocks
    uint32_t min_cov, min_delta_pct;
    const uint32_t *pos;           // [n]
    const uint32_t *cnt;           // [n*6]
    reg_agg *blk;                  // [n_blocks]: the blocks' totals, then their exclusive prefix
    reg_agg *row;                  // [n+1]: row[i] the sums of sites [0, i)
    uint64_t *tot;                 // [1]: informative sites
    uint32_t *status;              // bit 0: positions not ascending, bit 1: a count above 65,535
    const uint32_t *rs, *re;       // [n_reg] the regions
    pf_region_sum_t *out;          // [n_reg]
    uint32_t n_reg;
};

__device__ __forceinline__ reg_agg agg_none() {
    reg_agg r;
    r.n_sites = r.n_pos = r.n_neg = r.pad0 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) r.sum[k] = 0;
    r.ev = 0; r.pad1 = 0;
    return r;
}

__device__ __forceinline__ reg_agg agg_add(const reg_agg &A, const reg_agg &B) {
    reg_agg r;
    r.n_sites = A.n_sites + B.n_sites; r.n_pos = A.n_pos + B.n_pos; r.n_neg = A.n_neg + B.n_neg; r.pad0 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) r.sum[k] = A.sum[k] + B.sum[k];
    r.ev = A.ev + B.ev; r.pad1 = 0;
    return r;
}

// field by field, so that the aggregate stays in registers
__device__ __forceinline__ reg_agg agg_load(const reg_agg *p) {
    reg_agg r;
    r.n_sites = p->n_sites; r.n_pos = p->n_pos; r.n_neg = p->n_neg; r.pad0 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) r.sum[k] = p->sum[k];
    r.ev = p->ev; r.pad1 = 0;
    return r;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ reg_agg agg_shfl_up(const reg_agg &v, uint32_t d) {
    reg_agg r;
    r.n_sites = (uint32_t)__shfl_up((int)v.n_sites, d);
    r.n_pos = (uint32_t)__shfl_up((int)v.n_pos, d);
    r.n_neg = (uint32_t)__shfl_up((int)v.n_neg, d);
    r.pad0 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) r.sum[k] = shfl_up64(v.sum[k], d);
    r.ev = (int64_t)shfl_up64((uint64_t)v.ev, d);
    r.pad1 = 0;
    return r;
}

// the exclusive prefix of the workgroup's aggregates in thread order
__device__ __forceinline__ reg_agg block_exclusive(const reg_agg &mine, reg_agg *wtot) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    reg_agg inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        reg_agg o = agg_shfl_up(inc, d);
        if (lane < d) o = agg_none();
        inc = agg_add(o, inc);
    }
    if (lane == 63u) wtot[wave] = inc;
    __syncthreads();
    reg_agg ex = agg_shfl_up(inc, 1);
    if (lane == 0u) ex = agg_none();
    reg_agg pre = agg_none();
#pragma unroll
    for (uint32_t k = 0; k + 1 < PF_DMR_WAVES; k++) {
        reg_agg w = agg_load(wtot + k);
        if (k >= wave) w = agg_none();
        pre = agg_add(pre, w);
    }
    __syncthreads();
    return agg_add(pre, ex);
}

// X += site i; the rules are pf_dmr_regions' (pf_site.h) and pf_dmr_hmm_regions' evidence (pf_llr.h)
__device__ __forceinline__ void site_fold(const reg_args &a, uint32_t i, reg_agg &X, uint32_t &st) {
    const uint32_t p = a.pos[i];
    const reg_cnt4 c = *reinterpret_cast<const reg_cnt4 *>(a.cnt + 6ull * i);
    if (i > 0u && a.pos[i - 1] >= p) st |= 1u;
    if ((c.m1 | c.u1 | c.m2 | c.u2) > 0xFFFFu) { st |= 2u; return; }
    const uint32_t n1 = c.m1 + c.u1, n2 = c.m2 + c.u2;
    if (!site_informative(n1, n2, a.min_cov)) return;
    const uint32_t sg = site_sign(c.m1, n1, c.m2, n2, a.min_delta_pct);
    X.n_sites += 1u;
    X.n_pos += sg == 1u ? 1u : 0u;
    X.n_neg += sg == 2u ? 1u : 0u;
    X.sum[0] += c.m1; X.sum[1] += c.u1; X.sum[2] += c.m2; X.sum[3] += c.u2;
    X.ev += hmm_evidence(c.m1, c.u1, c.m2, c.u2);
}

template <bool PREFIX>
__device__ __forceinline__ void reg_block(const reg_args &a) {
    __shared__ reg_agg wtot[PF_DMR_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= a.n_blocks) return;
    // thread tid owns the block's sites [tid*K, +K)
    const uint64_t b0 = (uint64_t)blk * a.B;
    const uint64_t bend = b0 + a.B < a.n ? b0 + a.B : a.n;
    uint64_t i0 = b0 + (uint64_t)tid * a.K, i1 = i0 + a.K;
    if (i0 > bend) i0 = bend;
    if (i1 > bend) i1 = bend;
    uint32_t st = 0;
    reg_agg X = agg_none();
    for (uint64_t i = i0; i < i1; i++) site_fold(a, (uint32_t)i, X, st);
    if (!PREFIX && st) atomicOr(a.status, st);               // the error path only
    const reg_agg ex = block_exclusive(X, wtot);
    if (!PREFIX) {
        if (tid == PF_DMR_THREADS - 1u) a.blk[blk] = agg_add(ex, X);
        return;
    }
    X = agg_add(agg_load(a.blk + blk), ex);                  // everything left of this thread's sites
    for (uint64_t i = i0; i < i1; i++) {                     // i < n: row[n] is pf_reg_scan's
        a.row[i] = X;
        site_fold(a, (uint32_t)i, X, st);
    }
}

}  // namespace

__global__ __launch_bounds__(PF_DMR_THREADS) void pf_reg_count(reg_args a) { reg_block<false>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_reg_prefix(reg_args a) { reg_block<true>(a); }

// blk[b] <- the sums of the blocks before b; row[n] and tot <- the range's:
// one workgroup, each thread a contiguous run of blocks
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_reg_scan(reg_args a) {
    __shared__ reg_agg wtot[PF_DMR_WAVES];
    const uint32_t tid = threadIdx.x, n = a.n_blocks;
    const uint32_t chunk = (n + PF_DMR_THREADS - 1u) / PF_DMR_THREADS;
    const uint64_t c0 = (uint64_t)tid * chunk;
    const uint32_t i0 = (uint32_t)(c0 < n ? c0 : n), i1 = (uint32_t)(c0 + chunk < n ? c0 + chunk : n);
    reg_agg X = agg_none();
    for (uint32_t i = i0; i < i1; i++) X = agg_add(X, agg_load(a.blk + i));
    reg_agg c = block_exclusive(X, wtot);
    for (uint32_t i = i0; i < i1; i++) {
        const reg_agg t = agg_load(a.blk + i);
        a.blk[i] = c;
        c = agg_add(c, t);
    }
    if (tid == PF_DMR_THREADS - 1u) {                        // its chunk is the last: c is the whole range
        if (a.row) a.row[a.n] = c;                           // no table without regions
        a.tot[0] = c.n_sites;
    }
}

// sites of pos[0, n) below x
__device__ __forceinline__ uint32_t reg_lower_bound(const uint32_t *pos, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PF_DMR_THREADS) void pf_reg_lookup(reg_args a) {
    const uint64_t r = (uint64_t)blockIdx.x * PF_DMR_THREADS + threadIdx.x;
    if (r >= a.n_reg) return;
    const uint32_t s = a.rs[r], e = a.re[r];                 // s <= e: checked on the host
    // both at most n whatever pos holds; lo <= hi where the positions ascend (any other range is refused)
    const uint32_t lo = reg_lower_bound(a.pos, a.n, s), hi = reg_lower_bound(a.pos, a.n, e);
    const reg_agg L = agg_load(a.row + lo), H = agg_load(a.row + hi);
    pf_region_sum_t o;
    o.n_cpg = hi - lo;
    o.n_sites = H.n_sites - L.n_sites;
    o.n_pos = H.n_pos - L.n_pos;
    o.n_neg = H.n_neg - L.n_neg;
#pragma unroll
    for (int k = 0; k < 4; k++) o.sum[k] = H.sum[k] - L.sum[k];
    o.evidence = H.ev - L.ev;
    a.out[r] = o;
}

// ---- host side
extern "C" void pf_regions_free(pf_regions_t *r) {
    if (!r) return;
    free(const_cast<pf_region_sum_t *>(r->r));
    free(r);
}

extern "C" int pf_region_sums(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                              const uint32_t *reg_start, const uint32_t *reg_end, uint64_t n_regions, uint32_t block,
                              pf_regions_t **out) {
    if (!ctx || !pile || !cfg || !out || w1 < w0 || w1 > pile->n_windows || (w1 > w0 && !pile->win_off) ||
        (n_regions && (!reg_start || !reg_end)) || cfg->min_delta_pct > 100u)
        return PF_ERR_ARG;
    *out = nullptr;
    const uint32_t B = block ? block : pf_env_pow2("PF_REG_BLOCK", 64, PF_REG_BLOCK, PF_REG_BLOCK);
    if (B < 64u || B > PF_REG_BLOCK || (B & (B - 1u))) return PF_ERR_ARG;
    if (n_regions >= 0x80000000ull) return PF_ERR_LIMIT;
    for (uint64_t i = 0; i < n_regions; i++)
        if (reg_start[i] > reg_end[i]) return PF_ERR_ARG;
    const uint64_t s0 = w1 > w0 ? pile->win_off[w0] : 0, s1 = w1 > w0 ? pile->win_off[w1] : 0;
    if (s1 < s0 || s1 > pile->n_sites || (s1 > s0 && (!pile->pos || !pile->cnt))) return PF_ERR_ARG;
    const uint64_t n = s1 - s0;
    if (n > 0x7FFFFFFFull) return PF_ERR_LIMIT;

    pf_regions_t *res = (pf_regions_t *)calloc(1, sizeof(pf_regions_t));
    if (!res) return PF_ERR_NOMEM;
    pf_region_sum_t *h = nullptr;
    if (n_regions) {
        h = (pf_region_sum_t *)calloc((size_t)n_regions, sizeof(pf_region_sum_t));
        if (!h) { free(res); return PF_ERR_NOMEM; }
    }
    res->n = n_regions;
    res->r = h;
    if (n == 0) { *out = res; return PF_OK; }                 // no site: every record is all zero
    std::unique_ptr<pf_regions_t, void (*)(pf_regions_t *)> own(res, pf_regions_free);     // freed on every return but the last
    if (hipSetDevice(pf_ctx_device(ctx)) != hipSuccess) return PF_ERR_HIP;
    uint64_t tot = 0;
    uint32_t stt = 0;
    pf_call call(pf_ctx_stream(ctx));
    hipStream_t st = call.st;
    reg_args a;
    memset(&a, 0, sizeof a);
    a.n = (uint32_t)n; a.B = B; a.K = B > PF_DMR_THREADS ? B / PF_DMR_THREADS : 1u;
    a.n_blocks = (uint32_t)((n + B - 1) / B);
    a.min_cov = cfg->min_cov; a.min_delta_pct = cfg->min_delta_pct;
    a.n_reg = (uint32_t)n_regions;
    void *p_pos = nullptr, *p_cnt = nullptr, *p_rs = nullptr, *p_re = nullptr;
    if (!(p_pos = call.alloc(4ull * n)) || !(p_cnt = call.alloc(24ull * n)) ||
        !(a.blk = static_cast<reg_agg *>(call.alloc(sizeof(reg_agg) * (size_t)a.n_blocks))) ||
        !(a.tot = static_cast<uint64_t *>(call.alloc(8))) || !(a.status = static_cast<uint32_t *>(call.alloc(8))))
        return PF_ERR_NOMEM;
    if (n_regions && (!(a.row = static_cast<reg_agg *>(call.alloc(sizeof(reg_agg) * (size_t)(n + 1)))) ||
                      !(p_rs = call.alloc(4ull * n_regions)) || !(p_re = call.alloc(4ull * n_regions)) ||
                      !(a.out = static_cast<pf_region_sum_t *>(call.alloc(sizeof(pf_region_sum_t) * (size_t)n_regions)))))
        return PF_ERR_NOMEM;
    const auto t0 = std::chrono::steady_clock::now();
    if (hipMemcpyAsync(p_pos, pile->pos + s0, 4ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(p_cnt, pile->cnt + 6ull * s0, 24ull * n, hipMemcpyHostToDevice, st) != hipSuccess ||
        (n_regions && (hipMemcpyAsync(p_rs, reg_start, 4ull * n_regions, hipMemcpyHostToDevice, st) != hipSuccess ||
                       hipMemcpyAsync(p_re, reg_end, 4ull * n_regions, hipMemcpyHostToDevice, st) != hipSuccess)) ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_upload = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    a.pos = static_cast<const uint32_t *>(p_pos);
    a.cnt = static_cast<const uint32_t *>(p_cnt);
    a.rs = static_cast<const uint32_t *>(p_rs);
    a.re = static_cast<const uint32_t *>(p_re);
    if (hipMemsetAsync(a.status, 0, 8, st) != hipSuccess || !call.mark(0)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_reg_count, dim3(a.n_blocks), dim3(PF_DMR_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_reg_scan, dim3(1), dim3(PF_DMR_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    if (n_regions) {
        // a range that the count refuses goes through the other two kernels all
        // the same, in one submission: every index they form is bounded by n and
        // n_regions whatever the sites hold, and the records are dropped below
        hipLaunchKernelGGL(pf_reg_prefix, dim3(a.n_blocks), dim3(PF_DMR_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
        hipLaunchKernelGGL(pf_reg_lookup, dim3((uint32_t)((n_regions + PF_DMR_THREADS - 1) / PF_DMR_THREADS)),
                           dim3(PF_DMR_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    }
    if (!call.mark(1) || hipMemcpyAsync(&tot, a.tot, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&stt, a.status, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (n_regions && hipMemcpyAsync(h, a.out, sizeof(pf_region_sum_t) * (size_t)n_regions, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    if (stt & 1u) return PF_ERR_ARG;                          // positions not ascending over the range
    if (stt & 2u) return PF_ERR_LIMIT;
    res->n_informative = tot;
    res->ms_kernels = call.ms(0, 1);
    *out = own.release();
    return PF_OK;
}
