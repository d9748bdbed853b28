// pf_perm.hip -- read-label permutation test of a batch's windows
// (pf_batch_permtest; include/pomfret_amd.h has the definition).
//
// One workgroup per window, two phases, all in integers.
//
// Phase 1 takes the window's reads blockDim.x at a time, one per lane, and
// counts each one's meth and unmeth entries inside the window: the shared
// read-slice scan (pf_reads.h, window_read_counts).  The participating reads
// (tag 0 or 1, a count above zero) are compacted in read order into LDS
// (block_compact): m and m + u per read, 8 B each.  Their true labels are
// needed only through the sums n1, m1, u1, m2, u2, which LDS integer atomics
// collect.
//
// Phase 2 deals the permutations to the waves.  A permutation's keys are
// hashes of (window, b, i) and are recomputed wherever they are needed, never
// stored.  mix is a bijection of uint32 (xor-shifts and odd multipliers), so
// the keys mix(kb ^ i) of one permutation are distinct and the order by
// (key, i) is the order by key: the index never has to break a tie.  The n1
// reads of label 0 are those with the n1 smallest keys: the n1-th smallest key
// t is built bit by bit from the top, 32 steps of "count the keys below
// t | bit" (one compare and one scalar popcount per 64 reads), and one more
// pass labels a read 0 when its key is at most t; that pass also sums the
// label-0 reads' m and m + u, the wave reduces the two sums and the 128-bit
// products are compared on the scalar unit.  The keys of the first 256 reads
// stay in registers: the loop is instantiated for one to four chunks of 64
// reads and chosen per window, so that the 32 steps are straight-line code
// (at up to 64 reads: v_cmp, s_bcnt1, s_cmp, s_cselect, s_or); only reads past
// 256 have their keys recomputed in every step.  Hits are counted per wave,
// added once per wave in LDS and stored once per window.  The wave-uniform
// decisions are selects, not branches.  Integer sums and a total order on the
// keys: neither the workgroup size nor the order of the atomics reaches the
// result.
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

namespace {

static_assert(PF_PERM_READS == PF_PERM_MAX_READS, "the LDS arrays hold exactly the documented limit");

#define PF_PERM_KC 4                /* keys per lane held in registers: up to 256 reads recompute none */
static_assert(PF_PERM_KC == 4, "pf_perm_test dispatches perm_wave<1 .. 4>");
#define PERM_ST_LIMIT 3u            /* internal: N >= 2^31, the call returns PF_ERR_LIMIT */

struct perm_out {
    uint64_t sum[4];
    uint32_t n_reads[2];
    uint32_t hits, status;
};
static_assert(sizeof(perm_out) == 48, "perm_out is copied back as 48-byte records");

struct perm_args {
    uint32_t W, n_perm, seed, pad;
    pf_calls_view v;                                 /* read_hp: the batch's tags or the caller's */
    perm_out *out;                                   /* [W] */
};

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    return x ^ (x >> 16);
}

// a value that is the same in every lane, as a scalar
__device__ __forceinline__ uint32_t sfirst(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t sfirst64(uint64_t x) {
    return ((uint64_t)sfirst((uint32_t)(x >> 32)) << 32) | sfirst((uint32_t)x);
}

// one wave's share of a window's permutations; all of p is wave-uniform
struct perm_w {
    uint32_t n, n1, base, b0, step, n_perm;
    uint64_t M, N, A0, D0;
};

// NQ: the chunks of 64 reads whose keys stay in registers, ceil(n / 64) cut at
// PF_PERM_KC; only NQ == PF_PERM_KC has reads past them, whose keys are
// recomputed in every pass.  Returns the hits of permutations b0, b0 + step, ...
template <int NQ>
__device__ __forceinline__ uint32_t perm_wave(const perm_w &p, const uint32_t *s_m, const uint32_t *s_t, uint32_t lane) {
    uint32_t hits = 0;
    for (uint32_t b = p.b0; b < p.n_perm; b += p.step) {
        const uint32_t kb = mix(p.base + b);
        uint32_t kr[NQ];                              // a lane past n holds 0xFFFFFFFF, below no threshold
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const uint32_t i = 64u * q + lane;
            kr[q] = i < p.n ? mix(kb ^ i) : 0xFFFFFFFFu;
        }
        uint32_t t = 0;                               // the n1-th smallest key
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t cand = t | (1u << bit);
            uint32_t c = 0;
#pragma unroll
            for (int q = 0; q < NQ; q++) c += (uint32_t)__popcll(__ballot(kr[q] < cand));
            if (NQ == PF_PERM_KC)
                for (uint32_t i0 = 64u * PF_PERM_KC; i0 < p.n; i0 += 64u) {
                    const uint32_t i = i0 + lane;
                    c += (uint32_t)__popcll(__ballot((i < p.n) & (mix(kb ^ i) < cand)));
                }
            t = c < p.n1 ? cand : t;                  // fewer than n1 keys below cand: the n1-th smallest is >= cand
        }
        uint32_t M0 = 0, N0 = 0;
        auto label = [&](uint32_t i, uint32_t k) {
            const bool v = i < p.n;
            const bool take = v & (k <= t);           // distinct keys: exactly n1 reads
            const uint32_t j = v ? i : 0u;
            const uint32_t mm = s_m[j], tt = s_t[j];
            M0 += take ? mm : 0u;
            N0 += take ? tt : 0u;
        };
#pragma unroll
        for (int q = 0; q < NQ; q++) label(64u * q + lane, kr[q]);
        if (NQ == PF_PERM_KC)
            for (uint32_t i0 = 64u * PF_PERM_KC; i0 < p.n; i0 += 64u) label(i0 + lane, mix(kb ^ (i0 + lane)));
        M0 = wave_sum32(M0);
        N0 = wave_sum32(N0);
        const uint64_t M0s = sfirst(M0), N0s = sfirst(N0);
        const uint64_t x = M0s * p.N, y = p.M * N0s;
        const uint64_t A = x > y ? x - y : y - x;
        const uint64_t D = N0s * (p.N - N0s);
        const bool hit = D > 0ull && (unsigned __int128)A * p.D0 >= (unsigned __int128)p.A0 * D;
        hits += hit ? 1u : 0u;
    }
    return hits;
}

}  // namespace

__global__ __launch_bounds__(PF_PERM_THREADS_MAX) void pf_perm_test(perm_args a) {
    __shared__ uint32_t s_m[PF_PERM_READS], s_t[PF_PERM_READS];      // per participating read: m, m + u
    __shared__ unsigned long long s_sum[4];
    __shared__ uint32_t s_nr[2], s_hits, wsum[PF_PERM_THREADS_MAX / PF_WAVE];
    const uint32_t w = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nt = blockDim.x, nw = nt >> 6;
    if (w >= a.W) return;
    if (tid < 4u) s_sum[tid] = 0ull;
    if (tid < 2u) s_nr[tid] = 0u;
    if (tid == 0u) s_hits = 0u;
    __syncthreads();

    // ---- phase 1: the participating reads in read order
    const uint32_t ws = a.v.win_start[w], we = a.v.win_end[w];
    const uint32_t r0 = a.v.win_read_off[w], r1 = a.v.win_read_off[w + 1];
    uint32_t n = 0;
    for (uint32_t g = r0; g < r1; g += nt) {          // the same rounds in every thread: barriers inside
        uint32_t hp, my_m, my_u, tot;
        bool hit;
        window_read_counts(a.v, g, r1, ws, we, tid, hp, hit, my_m, my_u);
        const bool part = hit && (my_m | my_u) != 0u;
        const uint32_t slot = block_compact(part, wsum, nw, lane, wave, tot);
        if (part) {
            const uint32_t idx = n + slot;
            if (idx < PF_PERM_READS) {
                s_m[idx] = my_m;
                s_t[idx] = my_m + my_u;
            }
            atomicAdd(&s_sum[2u * hp], (unsigned long long)my_m);
            atomicAdd(&s_sum[2u * hp + 1u], (unsigned long long)my_u);
            atomicAdd(&s_nr[hp], 1u);
        }
        n += tot;
        __syncthreads();
    }

    const uint64_t m1 = s_sum[0], u1 = s_sum[1], m2 = s_sum[2], u2 = s_sum[3];
    const uint32_t n1 = s_nr[0];
    const uint64_t M = m1 + m2, N = M + u1 + u2, N0t = m1 + u1;
    const bool over = N >= 0x80000000ull;
    // below 2^31 each: the products fit 64 bits
    const uint64_t x0 = over ? 0ull : m1 * N, y0 = over ? 0ull : M * N0t;
    const uint64_t A0 = x0 > y0 ? x0 - y0 : y0 - x0;
    const uint64_t D0 = over ? 0ull : N0t * (N - N0t);
    const uint32_t status = over ? PERM_ST_LIMIT : n > PF_PERM_READS ? 2u : (n1 == 0u || n1 == n || D0 == 0ull) ? 1u : 0u;

    // ---- phase 2: the permutations, one wave each.  What is the same in every
    // lane goes through readfirstlane, so that the selection runs on the scalar
    // unit but for one compare per 64 keys.
    if (status == 0u) {
        perm_w p;
        p.n = sfirst(n); p.n1 = sfirst(n1);
        p.M = sfirst64(M); p.N = sfirst64(N); p.A0 = sfirst64(A0); p.D0 = sfirst64(D0);
        p.base = sfirst(mix(a.seed ^ mix(ws ^ mix(we))));
        p.b0 = sfirst(wave); p.step = nw; p.n_perm = a.n_perm;
        const uint32_t nq = (p.n + 63u) / 64u;
        const uint32_t hits = nq <= 1u ? perm_wave<1>(p, s_m, s_t, lane) : nq == 2u ? perm_wave<2>(p, s_m, s_t, lane)
                            : nq == 3u ? perm_wave<3>(p, s_m, s_t, lane) : perm_wave<PF_PERM_KC>(p, s_m, s_t, lane);
        if (lane == 0u && hits) atomicAdd(&s_hits, hits);
    }
    __syncthreads();
    if (tid == 0u) {
        perm_out o;
        o.sum[0] = m1; o.sum[1] = u1; o.sum[2] = m2; o.sum[3] = u2;
        o.n_reads[0] = n1; o.n_reads[1] = s_nr[1];
        o.hits = s_hits;
        o.status = status;
        a.out[w] = o;
    }
}

// ---- host side
extern "C" void pf_perm_free(pf_perm_t *p) {
    if (!p) return;
    free(const_cast<uint32_t *>(p->n_reads));
    free(const_cast<uint64_t *>(p->sum));
    free(const_cast<uint32_t *>(p->hits));
    free(const_cast<uint32_t *>(p->status));
    free(p);
}

extern "C" int pf_batch_permtest(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, uint32_t n_perm,
                                 uint32_t seed, pf_perm_t **out) {
    if (!ctx || !db || !out) return PF_ERR_ARG;
    *out = nullptr;
    if (n_perm < 1u || n_perm > PF_PERM_MAX_PERM) return PF_ERR_ARG;
    const uint32_t nt = pf_env_threads("PF_PERM_THREADS", PF_PERM_THREADS);
    if (!nt) return PF_ERR_ARG;
    pf_dev_batch d;
    const int vrc = pf_batch_calls_view(ctx, db, &d);
    if (vrc) return vrc;
    const uint32_t W = d.W, R = d.R;
    if (read_hp && n_hp != R) return PF_ERR_ARG;

    pf_perm_t *res = (pf_perm_t *)calloc(1, sizeof(pf_perm_t));
    if (!res) return PF_ERR_NOMEM;
    res->n_windows = W;
    res->n_perm = n_perm;
    res->seed = seed;
    if (W == 0) { *out = res; return PF_OK; }
    std::unique_ptr<pf_perm_t, void (*)(pf_perm_t *)> own(res, pf_perm_free);      // freed on every return but the last
    uint32_t *h_nr = (uint32_t *)calloc(2ull * W, 4), *h_hits = (uint32_t *)calloc(W, 4), *h_stat = (uint32_t *)calloc(W, 4);
    uint64_t *h_sum = (uint64_t *)calloc(4ull * W, 8);
    res->n_reads = h_nr; res->sum = h_sum; res->hits = h_hits; res->status = h_stat;
    if (!h_nr || !h_hits || !h_stat || !h_sum) return PF_ERR_NOMEM;
    std::vector<perm_out> h_out;
    try { h_out.resize(W); } catch (...) { return PF_ERR_NOMEM; }
    pf_call call(pf_ctx_stream(ctx));
    perm_args a;
    memset(&a, 0, sizeof a);
    a.W = W; a.n_perm = n_perm; a.seed = seed;
    a.v = pf_calls_view_of(d);
    const int hrc = call.upload_hp(read_hp, R, a.v);
    if (hrc) return hrc;
    a.out = static_cast<perm_out *>(call.alloc(sizeof(perm_out) * (size_t)W));
    if (!a.out) return PF_ERR_NOMEM;
    if (!call.mark(0)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_perm_test, dim3(W), dim3(nt), 0, call.st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(h_out.data(), a.out, sizeof(perm_out) * (size_t)W, hipMemcpyDeviceToHost, call.st) != hipSuccess ||
        hipStreamSynchronize(call.st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_kernels = call.ms(0, 1);
    for (uint32_t w = 0; w < W; w++) {
        const perm_out &o = h_out[w];
        if (o.status == PERM_ST_LIMIT) {
            fprintf(stderr, "[E::pomfret_amd] permtest: a window holds 2^31 or more calls\n");
            return PF_ERR_LIMIT;
        }
        for (int k = 0; k < 4; k++) h_sum[4ull * w + k] = o.sum[k];
        h_nr[2ull * w] = o.n_reads[0];
        h_nr[2ull * w + 1] = o.n_reads[1];
        h_hits[w] = o.hits;
        h_stat[w] = o.status;
    }
    *out = own.release();
    return PF_OK;
}
