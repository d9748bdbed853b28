// pf_dmr_hmm.hip -- allele-specific regions by a three-state hidden Markov model
// (pf_dmr_hmm_regions; include/pomfret_amd.h has the model).  All integer, and
// every step is a scan under an exact associative operator, so the result is
// the sequential Viterbi path bit for bit whatever the block.
//
// The model runs on the compacted informative sites j = 0 .. m-1:
//
//   pf_hmm_count     one workgroup per block of B sites of the range: the
//                    informative sites of the block, and the status bits
//                    (positions not ascending, a count above 65,535);
//   pf_hmm_offsets   one workgroup: the blocks' counts to their exclusive prefix;
//   pf_hmm_compact   the informative sites in order -- position, original index,
//                    break rank, evidence e -- each thread's slot from the
//                    block's offset and a prefix sum inside the block: no atomics;
//                    255 into the state of every transparent site;
//   pf_hmm_fwd_count / pf_hmm_fwd_scan / pf_hmm_fwd_apply
//                    Viterbi forward.  Site j is the 3x3 max-plus matrix
//                    M_j[r][s] = em_j[s] - (r != s ? switch : 0); a chain's first
//                    site is M_j[r][s] = em_j[s], which ignores what lies to its
//                    left, so chains need no segment flag.  Site 0 starts a chain,
//                    so every prefix product has three equal rows, and a row of
//                    M_0 x ... x M_j is V_j.  Every entry is a finite path sum
//                    (below 2^60); "nothing to the left" is a flag, not a value.
//                    Each thread folds its K consecutive sites, the wave scans the
//                    18 dwords with __shfl_up, the waves meet in LDS; the blocks'
//                    aggregates are scanned by one workgroup; apply replays each
//                    thread's sites from its carry-in and stores V_j[3];
//   pf_hmm_back_count / pf_hmm_back_scan / pf_hmm_back_apply
//                    the backtrace, the same three passes over j descending.
//                    g_j maps x_{j+1} to x_j: bp_{j+1}, computed from the stored
//                    V_j; at a chain's last site the constant map to its final
//                    state.  A map {0,1,2} -> {0,1,2} is six bits, composition is
//                    associative, and x_j = (g_j o g_{j+1} o ... o g_{m-1})(0).
//                    apply scatters x_j to state[original index];
//   pf_dmr_count_state / pf_dmr_scan / pf_dmr_emit_state  (pf_dmr.hip)
//                    the runs of the states.
//
// The host closes the runs at the range's ends and applies min_sites to them and
// the pooled-delta rule to every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <memory>
#include "pf_device.h"
#include "pf_llr.h"
#include "pf_call.h"
#include "../../include/pomfret_amd.h"

struct pf_ctx;
extern "C" int pf_ctx_device(const pf_ctx *c);
extern "C" hipStream_t pf_ctx_stream(const pf_ctx *c);
int pf_dmr_state_runs(pf_ctx_t *ctx, const uint32_t *d_pos, const uint32_t *d_cnt, const uint32_t *d_brk, uint32_t n_brk,
                      const uint8_t *d_state, uint32_t n, uint32_t B, const pf_dmr_cfg_t *cfg, pf_dmr_run_t **runs,
                      uint64_t *n_runs, float *ms);

namespace {

// a stretch of informative sites as a max-plus matrix; valid 0: an empty stretch
struct hmm_mat {
    int64_t v[9];                  // [r*3 + s]
    uint32_t valid, pad;
};
static_assert(sizeof(hmm_mat) == 80, "hmm_mat is shuffled and stored as 20 dwords");

struct hmm_args {
    uint32_t n, m, B, K;           // sites, informative sites, sites per block, sites per thread
    uint32_t nb_n, nb_m;           // blocks of the range, blocks of the informative sites
    uint32_t min_cov, max_gap;
    int32_t site_cost, sw;
    const uint32_t *pos;           // [n]
    const uint32_t *cnt;           // [n*6]
    const uint32_t *brk;           // [n_brk] ascending
    uint32_t n_brk;
    uint32_t *blk;                 // [nb_n]: the blocks' informative sites, then their exclusive prefix
    unsigned long long *tot;       // [2]: informative sites, chains
    uint32_t *status;              // bit 0: positions not ascending, bit 1: a count above 65,535
    uint32_t *cpos, *cidx, *crank; // [m]: position, index in the range, breaks <= position
    int64_t *ce;                   // [m]: evidence
    int64_t *V;                    // [m*3]
    hmm_mat *agg;                  // [nb_m]: the blocks' matrices, then their exclusive prefix
    uint32_t *magg;                // [nb_m]: the blocks' maps (descending j), then their exclusive prefix
    uint8_t *state;                // [n]
    int64_t *evid;                 // [n] or NULL
};

template <class T>
__device__ __forceinline__ T shfl_up_words(const T &v, uint32_t d) {
    struct raw { uint32_t w[sizeof(T) / 4]; };
    const raw s = __builtin_bit_cast(raw, v);
    raw r;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 4; k++) r.w[k] = (uint32_t)__shfl_up((int)s.w[k], d);
    return __builtin_bit_cast(T, r);
}

// the exclusive prefix of the workgroup's values in thread order under op
// (op.none() is neutral on either side); wtot: PF_DMR_WAVES values in LDS
template <class T, class Op>
__device__ __forceinline__ T block_exclusive(const T &mine, T *wtot, const Op &op) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    T inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        T o = shfl_up_words(inc, d);
        if (lane < d) o = op.none();
        inc = op(o, inc);
    }
    if (lane == 63u) wtot[wave] = inc;
    __syncthreads();
    T ex = shfl_up_words(inc, 1);
    if (lane == 0u) ex = op.none();
    T pre = op.none();
#pragma unroll
    for (uint32_t k = 0; k + 1 < PF_DMR_WAVES; k++) {
        T w = wtot[k];
        if (k >= wave) w = op.none();
        pre = op(pre, w);
    }
    __syncthreads();
    return op(pre, ex);
}

struct op_sum {
    __device__ __forceinline__ uint32_t none() const { return 0u; }
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};

// maps as six bits: x -> (map >> 2x) & 3.  A is applied first, then B
#define HMM_MAP_ID 0x24u
struct op_map {
    __device__ __forceinline__ uint32_t none() const { return HMM_MAP_ID; }
    __device__ __forceinline__ uint32_t operator()(uint32_t A, uint32_t B) const {
        uint32_t r = 0;
#pragma unroll
        for (uint32_t x = 0; x < 3u; x++) r |= ((B >> (2u * ((A >> (2u * x)) & 3u))) & 3u) << (2u * x);
        return r;
    }
};

struct op_mat {
    __device__ __forceinline__ hmm_mat none() const {
        hmm_mat r;
#pragma unroll
        for (int k = 0; k < 9; k++) r.v[k] = 0;
        r.valid = 0; r.pad = 0;
        return r;
    }
    // A then B: straight-line selects, an empty side leaves the other unchanged
    __device__ __forceinline__ hmm_mat operator()(const hmm_mat &A, const hmm_mat &B) const {
        hmm_mat R;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int s = 0; s < 3; s++) {
                int64_t b = A.v[r * 3] + B.v[s];
                const int64_t c1 = A.v[r * 3 + 1] + B.v[3 + s], c2 = A.v[r * 3 + 2] + B.v[6 + s];
                if (c1 > b) b = c1;
                if (c2 > b) b = c2;
                R.v[r * 3 + s] = (A.valid && B.valid) ? b : (A.valid ? A.v[r * 3 + s] : B.v[r * 3 + s]);
            }
        R.valid = A.valid | B.valid;
        R.pad = 0;
        return R;
    }
};

// thread tid's share [i0, i1) of block blk of `total` items
__device__ __forceinline__ void thread_range(const hmm_args &a, uint32_t blk, uint32_t total, uint64_t &i0, uint64_t &i1) {
    const uint64_t b0 = (uint64_t)blk * a.B;
    const uint64_t bend = b0 + a.B < total ? b0 + a.B : total;
    i0 = b0 + (uint64_t)threadIdx.x * a.K;
    i1 = i0 + a.K;
    if (i0 > bend) i0 = bend;
    if (i1 > bend) i1 = bend;
}

__device__ __forceinline__ bool site_informative(const hmm_args &a, uint32_t i, uint32_t c[4], uint32_t &st) {
    const uint2 c01 = *reinterpret_cast<const uint2 *>(a.cnt + 6ull * i);
    const uint2 c23 = *reinterpret_cast<const uint2 *>(a.cnt + 6ull * i + 2);
    c[0] = c01.x; c[1] = c01.y; c[2] = c23.x; c[3] = c23.y;
    if (i > 0u && a.pos[i - 1] >= a.pos[i]) st |= 1u;
    if ((c[0] | c[1] | c[2] | c[3]) > 0xFFFFu) { st |= 2u; return false; }
    return c[0] + c[1] >= a.min_cov && c[2] + c[3] >= a.min_cov;
}

// informative site j opens a chain
__device__ __forceinline__ bool chain_start(const hmm_args &a, uint32_t j) {
    return j == 0u || a.cpos[j] - a.cpos[j - 1] > a.max_gap || a.crank[j] != a.crank[j - 1];
}

__device__ __forceinline__ void emission(const hmm_args &a, uint32_t j, int64_t em[3]) {
    const int64_t e = a.ce[j];
    em[0] = 0; em[1] = e - a.site_cost; em[2] = -e - a.site_cost;
}

// X x M_j
__device__ __forceinline__ hmm_mat mat_step(const hmm_args &a, const hmm_mat &X, uint32_t j) {
    int64_t em[3];
    emission(a, j, em);
    const bool cs = chain_start(a, j), fresh = !X.valid || cs;
    hmm_mat R;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int s = 0; s < 3; s++) {
            int64_t b = X.v[r * 3] - (s != 0 ? a.sw : 0);
            const int64_t c1 = X.v[r * 3 + 1] - (s != 1 ? a.sw : 0), c2 = X.v[r * 3 + 2] - (s != 2 ? a.sw : 0);
            if (c1 > b) b = c1;
            if (c2 > b) b = c2;
            // a thread's first site stands for itself: M_j, or em alone where a chain starts
            const int64_t own = cs ? 0 : -(int64_t)(r != s ? a.sw : 0);
            R.v[r * 3 + s] = em[s] + (fresh ? (X.valid ? 0 : own) : b);
        }
    R.valid = 1; R.pad = 0;
    return R;
}

// g_j from V_j: x_{j+1} -> x_j
__device__ __forceinline__ uint32_t back_map(const hmm_args &a, uint32_t j) {
    const int64_t v0 = a.V[3ull * j], v1 = a.V[3ull * j + 1], v2 = a.V[3ull * j + 2];
    if (j + 1u >= a.m || chain_start(a, j + 1u)) {           // the chain's last site: the smallest s that attains the maximum
        uint32_t x = 0;
        int64_t b = v0;
        if (v1 > b) { b = v1; x = 1; }
        if (v2 > b) { b = v2; x = 2; }
        return x | (x << 2) | (x << 4);
    }
    const int64_t v[3] = {v0, v1, v2};
    uint32_t map = 0;
#pragma unroll
    for (int s = 0; s < 3; s++) {
        int64_t c[3];
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] = v[r] - (r != s ? a.sw : 0);
        uint32_t x = 0;
        int64_t b = c[0];
        if (c[1] > b) { b = c[1]; x = 1; }
        if (c[2] > b) { b = c[2]; x = 2; }
        if (c[s] == b) x = (uint32_t)s;
        map |= x << (2 * s);
    }
    return map;
}

template <bool COMPACT>
__device__ __forceinline__ void count_block(const hmm_args &a) {
    __shared__ uint32_t wtot[PF_DMR_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= a.nb_n) return;
    uint64_t i0, i1;
    thread_range(a, blk, a.n, i0, i1);
    uint32_t st = 0, c = 0, q[4];
    for (uint64_t i = i0; i < i1; i++) c += site_informative(a, (uint32_t)i, q, st) ? 1u : 0u;
    if (!COMPACT && st) atomicOr(a.status, st);              // the error path only
    const uint32_t ex = block_exclusive(c, wtot, op_sum());
    if (!COMPACT) {
        if (tid == PF_DMR_THREADS - 1u) a.blk[blk] = ex + c;
        return;
    }
    uint64_t j = (uint64_t)a.blk[blk] + ex;
    for (uint64_t i = i0; i < i1; i++) {
        const bool inf = site_informative(a, (uint32_t)i, q, st);
        const int64_t e = inf ? hmm_evidence(q[0], q[1], q[2], q[3]) : 0;
        if (a.evid) a.evid[i] = e;
        if (!inf) { a.state[i] = 255; continue; }
        if (j >= a.m) continue;                              // holds: both passes count the same sites
        const uint32_t p = a.pos[i];
        uint32_t lo = 0, hi = a.n_brk;                       // breaks <= p
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.brk[mid] <= p) lo = mid + 1; else hi = mid;
        }
        a.cpos[j] = p; a.cidx[j] = (uint32_t)i; a.crank[j] = lo; a.ce[j] = e;
        j++;
    }
}

template <bool APPLY>
__device__ __forceinline__ void fwd_block(const hmm_args &a) {
    __shared__ hmm_mat wtot[PF_DMR_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= a.nb_m) return;
    uint64_t j0, j1;
    thread_range(a, blk, a.m, j0, j1);
    const op_mat op;
    hmm_mat X = op.none();
    for (uint64_t j = j0; j < j1; j++) X = mat_step(a, X, (uint32_t)j);
    const hmm_mat ex = block_exclusive(X, wtot, op);
    if (!APPLY) {
        if (tid == PF_DMR_THREADS - 1u) a.agg[blk] = op(ex, X);
        return;
    }
    const hmm_mat pre = op(a.agg[blk], ex);                  // everything left of this thread's sites: three equal rows
    int64_t v[3] = {pre.v[0], pre.v[1], pre.v[2]};
    uint32_t chains = 0;
    for (uint64_t j = j0; j < j1; j++) {
        int64_t em[3], w[3];
        emission(a, (uint32_t)j, em);
        const bool cs = chain_start(a, (uint32_t)j);         // pre is valid wherever cs is false: site 0 opens a chain
        chains += cs ? 1u : 0u;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            int64_t b = v[0] - (s != 0 ? a.sw : 0);
            const int64_t c1 = v[1] - (s != 1 ? a.sw : 0), c2 = v[2] - (s != 2 ? a.sw : 0);
            if (c1 > b) b = c1;
            if (c2 > b) b = c2;
            w[s] = em[s] + (cs ? 0 : b);
        }
#pragma unroll
        for (int s = 0; s < 3; s++) { v[s] = w[s]; a.V[3ull * j + s] = w[s]; }
    }
    if (chains) atomicAdd(a.tot + 1, (unsigned long long)chains);     // a count: no order depends on it
}

// item q of the descending order is site m-1-q
template <bool APPLY>
__device__ __forceinline__ void back_block(const hmm_args &a) {
    __shared__ uint32_t wtot[PF_DMR_WAVES];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= a.nb_m) return;
    uint64_t q0, q1;
    thread_range(a, blk, a.m, q0, q1);
    const op_map op;
    uint32_t F = HMM_MAP_ID;
    for (uint64_t q = q0; q < q1; q++) F = op(F, back_map(a, a.m - 1u - (uint32_t)q));
    const uint32_t ex = block_exclusive(F, wtot, op);
    if (!APPLY) {
        if (tid == PF_DMR_THREADS - 1u) a.magg[blk] = op(ex, F);
        return;
    }
    F = op(a.magg[blk], ex);
    for (uint64_t q = q0; q < q1; q++) {
        const uint32_t j = a.m - 1u - (uint32_t)q;
        F = op(F, back_map(a, j));
        const uint32_t i = a.cidx[j];
        if (i < a.n) a.state[i] = (uint8_t)(F & 3u);         // the last map is constant: any argument, 0 here
    }
}

// arr[0, n) <- its exclusive prefix under op, one workgroup, each thread a
// contiguous run; returns the whole in the last thread
template <class T, class Op>
__device__ __forceinline__ T scan_in_place(T *arr, uint32_t n, T *wtot, const Op &op) {
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = (n + PF_DMR_THREADS - 1u) / PF_DMR_THREADS;
    const uint64_t c0 = (uint64_t)tid * chunk;
    const uint32_t i0 = (uint32_t)(c0 < n ? c0 : n), i1 = (uint32_t)(c0 + chunk < n ? c0 + chunk : n);
    T X = op.none();
    for (uint32_t i = i0; i < i1; i++) X = op(X, arr[i]);
    T c = block_exclusive(X, wtot, op);
    for (uint32_t i = i0; i < i1; i++) {
        const T t = arr[i];
        arr[i] = c;
        c = op(c, t);
    }
    return c;
}

}  // namespace

__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_count(hmm_args a) { count_block<false>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_compact(hmm_args a) { count_block<true>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_offsets(hmm_args a) {
    __shared__ uint32_t wtot[PF_DMR_WAVES];
    const uint32_t c = scan_in_place(a.blk, a.nb_n, wtot, op_sum());
    if (threadIdx.x == PF_DMR_THREADS - 1u) a.tot[0] = c;
}
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_fwd_count(hmm_args a) { fwd_block<false>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_fwd_apply(hmm_args a) { fwd_block<true>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_fwd_scan(hmm_args a) {
    __shared__ hmm_mat wtot[PF_DMR_WAVES];
    (void)scan_in_place(a.agg, a.nb_m, wtot, op_mat());
}
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_back_count(hmm_args a) { back_block<false>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_back_apply(hmm_args a) { back_block<true>(a); }
__global__ __launch_bounds__(PF_DMR_THREADS) void pf_hmm_back_scan(hmm_args a) {
    __shared__ uint32_t wtot[PF_DMR_WAVES];
    (void)scan_in_place(a.magg, a.nb_m, wtot, op_map());
}

// ---- host side
extern "C" int64_t pf_dmr_hmm_evidence(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2) {
    if ((m1 | u1 | m2 | u2) > 0xFFFFu) return 0;
    return hmm_evidence(m1, u1, m2, u2);
}

extern "C" void pf_dmr_hmm_free(pf_dmr_hmm_t *h) {
    if (!h) return;
    free(const_cast<pf_dmr_run_t *>(h->runs));
    free(const_cast<uint8_t *>(h->state));
    free(const_cast<int64_t *>(h->evidence));
    free(h);
}

// the pooled levels differ by min_delta_pct in the run's direction
static bool hmm_delta_ok(const pf_dmr_run_t &r, uint32_t min_delta_pct) {
    const __int128 M1 = r.sum[0], M2 = r.sum[2], N1 = (__int128)r.sum[0] + r.sum[1], N2 = (__int128)r.sum[2] + r.sum[3];
    return (__int128)r.sign * (M1 * N2 - M2 * N1) * 100 >= (__int128)min_delta_pct * N1 * N2;
}

extern "C" int pf_dmr_hmm_regions(pf_ctx_t *ctx, const pf_pileup_t *pile, uint32_t w0, uint32_t w1, const pf_dmr_cfg_t *cfg,
                                  const pf_dmr_hmm_cfg_t *hcfg, const uint32_t *breaks, uint32_t n_breaks, uint32_t block,
                                  uint32_t flags, pf_dmr_hmm_t **out) {
    if (!ctx || !pile || !cfg || !hcfg || !out || w1 < w0 || w1 > pile->n_windows || (w1 > w0 && !pile->win_off) ||
        (n_breaks && !breaks) || cfg->min_delta_pct > 100u || hcfg->site_cost_q16 < 0 || hcfg->site_cost_q16 > 64 * 65536 ||
        hcfg->switch_q16 < 0 || hcfg->switch_q16 > 64 * 65536)
        return PF_ERR_ARG;
    *out = nullptr;
    const uint32_t B = block ? block : pf_env_pow2("PF_DMR_BLOCK", 64, PF_DMR_BLOCK, PF_DMR_BLOCK);   // as pf_dmr_regions reads it
    if (B < 64u || B > PF_DMR_BLOCK || (B & (B - 1u))) return PF_ERR_ARG;
    for (uint32_t i = 1; i < n_breaks; i++)
        if (breaks[i] < breaks[i - 1]) return PF_ERR_ARG;
    const uint64_t s0 = w1 > w0 ? pile->win_off[w0] : 0, s1 = w1 > w0 ? pile->win_off[w1] : 0;
    if (s1 < s0 || s1 > pile->n_sites || (s1 > s0 && (!pile->pos || !pile->cnt))) return PF_ERR_ARG;
    const uint64_t n = s1 - s0;
    if (n > 0x7FFFFFFFull) return PF_ERR_LIMIT;

    pf_dmr_hmm_t *res = (pf_dmr_hmm_t *)calloc(1, sizeof(pf_dmr_hmm_t));
    if (!res) return PF_ERR_NOMEM;
    res->n_sites = n;
    if (n == 0) { *out = res; return PF_OK; }
    std::unique_ptr<pf_dmr_hmm_t, void (*)(pf_dmr_hmm_t *)> own(res, pf_dmr_hmm_free);     // freed on every return but the last
    if (hipSetDevice(pf_ctx_device(ctx)) != hipSuccess) return PF_ERR_HIP;
    unsigned long long tot[2] = {0, 0};
    uint32_t stt = 0;
    pf_call call(pf_ctx_stream(ctx));
    hipStream_t st = call.st;
    hmm_args a;
    memset(&a, 0, sizeof a);
    a.n = (uint32_t)n; a.B = B; a.K = B > PF_DMR_THREADS ? B / PF_DMR_THREADS : 1u;
    a.nb_n = (uint32_t)((n + B - 1) / B);
    a.min_cov = cfg->min_cov; a.max_gap = cfg->max_gap;
    a.site_cost = hcfg->site_cost_q16; a.sw = hcfg->switch_q16;
    a.n_brk = n_breaks;
    const bool sites = flags & PF_DMR_HMM_SITES;
    void *p_pos = nullptr, *p_cnt = nullptr, *p_brk = nullptr;
    if (!(p_pos = call.alloc(4ull * n)) || !(p_cnt = call.alloc(24ull * n)) || !(p_brk = call.alloc(4ull * n_breaks)) ||
        !(a.blk = static_cast<uint32_t *>(call.alloc(4ull * a.nb_n))) ||
        !(a.tot = static_cast<unsigned long long *>(call.alloc(16))) || !(a.status = static_cast<uint32_t *>(call.alloc(8))) ||
        !(a.state = static_cast<uint8_t *>(call.alloc(n))) || (sites && !(a.evid = static_cast<int64_t *>(call.alloc(8ull * n)))))
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
    const dim3 T(PF_DMR_THREADS);
    if (hipMemsetAsync(a.status, 0, 8, st) != hipSuccess || hipMemsetAsync(a.tot, 0, 16, st) != hipSuccess || !call.mark(0))
        return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_hmm_count, dim3(a.nb_n), T, 0, st, a);
    if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_hmm_offsets, dim3(1), T, 0, st, a);
    if (hipGetLastError() != hipSuccess || !call.mark(1) ||
        hipMemcpyAsync(tot, a.tot, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&stt, a.status, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    if (stt & 1u) return PF_ERR_ARG;                          // positions not ascending over the range
    if (stt & 2u) return PF_ERR_LIMIT;
    const uint64_t m = tot[0];
    if (m > n) return PF_ERR_INTERNAL;
    a.m = (uint32_t)m;
    a.nb_m = (uint32_t)((m + B - 1) / B);
    if (!(a.cpos = static_cast<uint32_t *>(call.alloc(4ull * m))) || !(a.cidx = static_cast<uint32_t *>(call.alloc(4ull * m))) ||
        !(a.crank = static_cast<uint32_t *>(call.alloc(4ull * m))) || !(a.ce = static_cast<int64_t *>(call.alloc(8ull * m))) ||
        !(a.V = static_cast<int64_t *>(call.alloc(24ull * m))) ||
        !(a.agg = static_cast<hmm_mat *>(call.alloc(sizeof(hmm_mat) * (size_t)a.nb_m))) ||
        !(a.magg = static_cast<uint32_t *>(call.alloc(4ull * a.nb_m))))
        return PF_ERR_NOMEM;
    if (!call.mark(2)) return PF_ERR_HIP;
    hipLaunchKernelGGL(pf_hmm_compact, dim3(a.nb_n), T, 0, st, a);
    if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    if (m) {
        hipLaunchKernelGGL(pf_hmm_fwd_count, dim3(a.nb_m), T, 0, st, a);
        hipLaunchKernelGGL(pf_hmm_fwd_scan, dim3(1), T, 0, st, a);
        hipLaunchKernelGGL(pf_hmm_fwd_apply, dim3(a.nb_m), T, 0, st, a);
        hipLaunchKernelGGL(pf_hmm_back_count, dim3(a.nb_m), T, 0, st, a);
        hipLaunchKernelGGL(pf_hmm_back_scan, dim3(1), T, 0, st, a);
        hipLaunchKernelGGL(pf_hmm_back_apply, dim3(a.nb_m), T, 0, st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    }
    if (!call.mark(3) || hipMemcpyAsync(tot + 1, a.tot + 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    const float ms01 = call.ms(0, 1) + call.ms(2, 3);
    float ms2 = 0.0f;
    res->n_informative = m;
    res->n_chains = tot[1];
    if (sites) {
        uint8_t *hs = (uint8_t *)malloc(n);
        int64_t *he = (int64_t *)malloc(8ull * n);
        res->state = hs;
        res->evidence = he;
        if (!hs || !he) return PF_ERR_NOMEM;
        if (hipMemcpyAsync(hs, a.state, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(he, a.evid, 8ull * n, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PF_ERR_HIP;
    }
    if (m) {
        pf_dmr_run_t *runs = nullptr;
        uint64_t n_runs = 0;
        const int rc = pf_dmr_state_runs(ctx, a.pos, a.cnt, a.brk, n_breaks, a.state, a.n, B, cfg, &runs, &n_runs, &ms2);
        if (rc) return rc;
        // the runs at the range's ends are closed here, and filtered like any other
        uint64_t k = 0;
        for (uint64_t i = 0; i < n_runs; i++) {
            if (runs[i].n_sites < cfg->min_sites || !hmm_delta_ok(runs[i], cfg->min_delta_pct)) continue;
            runs[k] = runs[i];
            runs[k].open = 0;
            k++;
        }
        if (k == 0) { free(runs); runs = nullptr; }
        res->runs = runs;
        res->n_runs = k;
    }
    res->ms_kernels = ms01 + ms2;
    *out = own.release();
    return PF_OK;
}
