// pf_tagcheck.hip -- leave-one-out check of read tags against a window's
// allele-specific methylation (pf_batch_tagcheck; include/pomfret_amd.h has the
// definition).
//
// The site table is the pileup's, as in pf_assign.hip: pf_batch_pileup_dev runs
// the pileup kernels under the call's tags and leaves the per-window site CSR
// (pos, cnt) in HBM.  Two kernels follow, all in integers.
//
// pf_tagcheck_weights, one thread per site: taking one entry out of a site's
// counts changes them by one in a place that (tag, category) names, so the
// weight of every entry a tagged read can have there is one of four values;
// twelve distinct evaluations of the Q16 log2 (pf_llr.h), stored as one int4
// beside the site.  A tag whose entries are not usable at the site gets
// PF_LLR_NONE -- a value no weight takes -- so that "usable with weight 0"
// stays distinct from it.
//
// pf_tagcheck_score, one workgroup per window.  The window's sites go through
// LDS in tiles of T (position and four weights, 20 B per site).  About two
// thirds of a window's reads are scored here, so the waves do not step over the
// reads 64 at a time as pf_assign_score's do; per tile and per 256 reads
//   A  one read per lane, read index -> lane fixed: a scored read (tag 0 / 1)
//      whose sorted call slice can touch the tile's position range
//      binary-searches it for the tile's first position; a read that hits
//      takes the next slot of a list in LDS (one LDS atomic per wave);
//   B  the list's entries are dealt to the waves round robin: the wave strides
//      over the read's calls up to the tile's last position, every lane
//      binary-searching its call's position in the LDS tile, reduces the int64
//      sum and the count, and leaves both in the entry;
//   C  the lane that owns the read folds the entry into the read's row of the
//      output -- that lane alone reads and writes the row, whatever wave did
//      the sum -- and after the last tile gives the verdict.
// The window's eight counters are ballot counts added in LDS.  No HBM atomics;
// integer sums: neither the tile, the workgroup size nor the order in which the
// list fills reaches the result.  pf_assign_score's layout -- every wave steps
// over the reads 64 at a time and sums its own hits one after the other --
// takes 1.5 to 1.7 x as long on all three batches of
// profiles/tagcheck/README.md.
//
// The tile in LDS is no larger than the batch's largest window needs (a power of
// two): the windows of hapmeth's second pass hold about a hundred sites, and a
// workgroup that asks for the full 2,048-site tile keeps two more workgroups
// off its CU for nothing (profiles/tagcheck/README.md).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "pf_device.h"
#include "pf_llr.h"
#include "pf_reads.h"
#include "pf_call.h"
#include "../../include/pomfret_amd.h"

struct pf_ctx;
struct pf_dbatch;
extern "C" hipStream_t pf_ctx_stream(const pf_ctx *c);
extern "C" int pf_batch_calls_view(pf_ctx *ctx, pf_dbatch *b, pf_dev_batch *view);                                 // pf_api.hip
extern "C" int pf_batch_pileup_dev(pf_ctx *ctx, pf_dbatch *b, const uint8_t *read_hp, uint32_t n_hp, pf_pile_dev *dev);
extern "C" void pf_pile_dev_free(pf_pile_dev *dev);

namespace {

struct tagcheck_args {
    uint32_t W, T, min_cov, min_calls;
    long long min_llr;
    uint64_t n_sites;
    pf_calls_view v;                                 /* read_hp: the batch's tags or the caller's */
    const uint64_t *site_off;                        /* [W+1] */
    const uint32_t *site_pos;                        /* [n_sites] */
    const uint32_t *site_cnt;                        /* [n_sites*6] */
    int4 *site_w;                                    /* [n_sites] wM0, wU0, wM1, wU1; PF_LLR_NONE: that tag is not usable */
    uint32_t *n_used;                                /* [R] zeroed by the host */
    long long *llr;                                  /* [R] zeroed by the host */
    uint8_t *verdict;                                /* [R] 255 from the host */
    uint32_t *win_n;                                 /* [W*8] */
};

#define TC_LIST PF_TAGCHECK_THREADS                  /* list entries: one per read of a round */
/* dynamic LDS: the tile, the list (lo, end, sum: 8 B; tag, count: 4 B), eight counters and the list's length */
#define TC_LDS(T) (20u * (T) + 32u * TC_LIST + 48u)

// the verdict of a scored read from its sum and count (the header's table)
__device__ inline uint32_t tc_verdict(const tagcheck_args &a, uint32_t h, long long S, uint32_t n) {
    if (!n) return 255u;
    uint32_t d = 2u;
    if (n >= a.min_calls) {
        if (S > 0 && S >= a.min_llr) d = 0u;
        else if (S < 0 && -S >= a.min_llr) d = 1u;
    }
    return d == 2u ? 2u : d == h ? 0u : 1u;
}

// one wave: the sum and the count of the calls [s, e) of a read tagged h that
// lie in the LDS tile (s is the first call at or right of the tile's first
// position); every lane returns both
__device__ inline void tc_read_sum(const tagcheck_args &a, const uint32_t *s_pos, const int32_t *s_w, uint32_t n, uint32_t p_hi,
                                   uint64_t s, uint64_t e, uint32_t h, uint32_t lane, long long *sum, uint32_t *cnt) {
    long long acc = 0;
    uint32_t cn = 0;
    for (uint64_t c0 = s; c0 < e; c0 += 64) {
        const uint64_t c = c0 + lane;
        const bool valid = c < e;
        const uint32_t p = valid ? a.v.call_pos[c] : 0u;
        const uint32_t cat = valid ? a.v.call_cat[c] : 2u;
        if (valid && p <= p_hi && cat < 2u) {         // p >= the tile's first position: the slice is sorted and starts there
            uint32_t k = 0;
            for (uint32_t hi = n; k < hi;) {
                const uint32_t mid = k + (hi - k) / 2;
                if (s_pos[mid] < p) k = mid + 1; else hi = mid;
            }
            if (k < n && s_pos[k] == p) {
                const int32_t w = s_w[(2u * h + cat) * a.T + k];
                if (w != PF_LLR_NONE) {
                    acc += w;
                    cn++;
                }
            }
        }
        if (__ballot(valid && p > p_hi)) break;       // past the tile's last position
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t al = (uint32_t)__shfl_xor((int)(uint32_t)acc, d);
        const uint32_t ah = (uint32_t)__shfl_xor((int)(uint32_t)((unsigned long long)acc >> 32), d);
        acc += (long long)(((unsigned long long)ah << 32) | al);
        cn += (uint32_t)__shfl_xor((int)cn, d);
    }
    *sum = acc;
    *cnt = cn;
}

}  // namespace

__global__ __launch_bounds__(256) void pf_tagcheck_weights(tagcheck_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_sites) return;
    const uint2 *c = reinterpret_cast<const uint2 *>(a.site_cnt + 6 * i);
    const uint2 h1 = c[0], h2 = c[1];
    int32_t w[4];
    loo_weights(h1.x, h1.y, h2.x, h2.y, a.min_cov, w);
    a.site_w[i] = make_int4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(PF_TAGCHECK_THREADS) void pf_tagcheck_score(tagcheck_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];
    const uint32_t w = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t T = a.T;
    if (w >= a.W) return;
    uint32_t *s_pos = s_mem;                                                     // [T]
    int32_t *s_w = reinterpret_cast<int32_t *>(s_mem + T);                       // [4][T]: wM0, wU0, wM1, wU1
    uint64_t *s_lo = reinterpret_cast<uint64_t *>(s_mem + 5u * T);               // the list: first call in the tile,
    uint64_t *s_e = s_lo + TC_LIST;                                              // the slice's end,
    long long *s_sum = reinterpret_cast<long long *>(s_e + TC_LIST);             // the wave's sum
    uint32_t *s_tag = reinterpret_cast<uint32_t *>(s_sum + TC_LIST);             // the read's tag
    uint32_t *s_cn = s_tag + TC_LIST;                                            // and the wave's count
    uint32_t *s_n = s_cn + TC_LIST;                                              // [8] the window's counters
    uint32_t *s_len = s_n + 8;                                                   // the list's length
    if (tid < 9u) s_n[tid] = 0u;                                                 // s_n[8] is s_len
    const uint64_t s0 = a.site_off[w], s1 = a.site_off[w + 1];
    const uint32_t r0 = a.v.win_read_off[w], r1 = a.v.win_read_off[w + 1];
    const uint64_t n_tiles = s1 > s0 ? (s1 - s0 + T - 1) / T : 1;                // a window without sites: one empty tile
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t b0 = s0 + t * T;
        const uint32_t n = b0 < s1 ? (uint32_t)(s1 - b0 < T ? s1 - b0 : T) : 0u;
        __syncthreads();                              // the previous tile's readers are done
        for (uint32_t i = tid; i < n; i += PF_TAGCHECK_THREADS) {
            const int4 ww = a.site_w[b0 + i];
            s_pos[i] = a.site_pos[b0 + i];
            s_w[i] = ww.x;
            s_w[T + i] = ww.y;
            s_w[2u * T + i] = ww.z;
            s_w[3u * T + i] = ww.w;
        }
        __syncthreads();
        const uint32_t p_lo = n ? s_pos[0] : 0u, p_hi = n ? s_pos[n - 1u] : 0u;
        const bool last = t + 1 == n_tiles;
        for (uint32_t g = r0; g < r1; g += PF_TAGCHECK_THREADS) {
            // A: this lane's read
            const uint32_t r = g + tid;
            const bool have = r >= g && r < r1;
            const uint32_t hp = have ? a.v.read_hp[r] : 255u;
            const bool scored = hp < 2u;
            uint64_t lo = 0, c1 = 0;
            if (scored && n) {
                lo = a.v.read_call_off[r];
                c1 = a.v.read_call_end[r];
            }
            // a slice that ends left of the tile or starts right of it needs no search
            if (lo < c1 && (a.v.call_pos[c1 - 1] < p_lo || a.v.call_pos[lo] > p_hi)) lo = c1;
            for (uint64_t hi = c1; lo < hi;) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (a.v.call_pos[mid] < p_lo) lo = mid + 1; else hi = mid;
            }
            const bool hit = lo < c1 && a.v.call_pos[lo] <= p_hi;
            const uint64_t b_hit = __ballot(hit);
            uint32_t base = 0;
            if (b_hit && lane == 0u) base = atomicAdd(s_len, (uint32_t)__popcll(b_hit));
            const uint32_t slot = (uint32_t)__shfl((int)base, 0) + (uint32_t)__popcll(b_hit & ((1ull << lane) - 1ull));
            if (hit) {                                // at most one entry per lane of the workgroup: slot < TC_LIST
                s_lo[slot] = lo;
                s_e[slot] = c1;
                s_tag[slot] = hp;
            }
            __syncthreads();
            // B: the hits, dealt to the waves
            const uint32_t len = *s_len;
            for (uint32_t j = wave; j < len; j += PF_TAGCHECK_WAVES) {
                long long acc;
                uint32_t cn;
                tc_read_sum(a, s_pos, s_w, n, p_hi, s_lo[j], s_e[j], s_tag[j], lane, &acc, &cn);
                if (lane == 0u) {
                    s_sum[j] = acc;
                    s_cn[j] = cn;
                }
            }
            __syncthreads();
            // C: the read's row: its lane alone reads and writes it
            long long my_s = 0;
            uint32_t my_n = 0;
            if (hit) {
                my_s = s_sum[slot];
                my_n = s_cn[slot];
            }
            if (tid == 0u) *s_len = 0u;
            if (scored && (last || my_n)) {
                my_s += a.llr[r];
                my_n += a.n_used[r];
            }
            if (last) {
                const uint32_t v = scored ? tc_verdict(a, hp, my_s, my_n) : 255u;
                if (scored) {
                    a.verdict[r] = (uint8_t)v;
                    a.llr[r] = my_s;
                    a.n_used[r] = my_n;
                }
#pragma unroll
                for (uint32_t h = 0; h < 2u; h++) {
                    const bool mine = scored && hp == h;
                    const uint64_t b_r = __ballot(mine), b_sc = __ballot(mine && my_n >= 1u), b_ok = __ballot(mine && v == 0u),
                                   b_fl = __ballot(mine && v == 1u);
                    if (lane == 0u && b_r) {
                        atomicAdd(&s_n[4u * h], (uint32_t)__popcll(b_r));
                        if (b_sc) atomicAdd(&s_n[4u * h + 1u], (uint32_t)__popcll(b_sc));
                        if (b_ok) atomicAdd(&s_n[4u * h + 2u], (uint32_t)__popcll(b_ok));
                        if (b_fl) atomicAdd(&s_n[4u * h + 3u], (uint32_t)__popcll(b_fl));
                    }
                }
            } else if (scored && my_n) {
                a.llr[r] = my_s;
                a.n_used[r] = my_n;
            }
            __syncthreads();                          // the list is free again
        }
    }
    __syncthreads();
    if (tid < 8u) a.win_n[8ull * w + tid] = s_n[tid];
}

// ---- host side
extern "C" void pf_tagcheck_site_weights(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2, uint32_t min_cov, int32_t w[4],
                                         uint8_t usable[2]) {
    if (!w || !usable) return;
    // the header's range: a count above 65,535 is no pileup count
    if (m1 > 0xFFFFu) m1 = 0xFFFFu;
    if (u1 > 0xFFFFu) u1 = 0xFFFFu;
    if (m2 > 0xFFFFu) m2 = 0xFFFFu;
    if (u2 > 0xFFFFu) u2 = 0xFFFFu;
    loo_weights(m1, u1, m2, u2, min_cov, w);
    for (int h = 0; h < 2; h++) {
        usable[h] = w[2 * h] != PF_LLR_NONE;
        if (!usable[h]) w[2 * h] = w[2 * h + 1] = 0;
    }
}

extern "C" void pf_tagcheck_free(pf_tagcheck_t *p) {
    if (!p) return;
    free(const_cast<uint32_t *>(p->win_read_off));
    free(const_cast<uint32_t *>(p->n_used));
    free(const_cast<int64_t *>(p->llr));
    free(const_cast<uint8_t *>(p->verdict));
    free(const_cast<uint8_t *>(p->hp));
    free(const_cast<uint32_t *>(p->win_n));
    free(p);
}

extern "C" int pf_batch_tagcheck(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, const pf_assign_cfg_t *cfg,
                                 pf_tagcheck_t **out) {
    if (!ctx || !db || !out || !cfg) return PF_ERR_ARG;
    *out = nullptr;
    const uint32_t T = pf_env_pow2("PF_TAGCHECK_TILE", 64, PF_TAGCHECK_TILE, PF_TAGCHECK_TILE);
    if (!T) return PF_ERR_ARG;
    pf_dev_batch d;
    const int vrc = pf_batch_calls_view(ctx, db, &d);
    if (vrc) return vrc;
    const uint32_t W = d.W, R = d.R;
    if (read_hp && n_hp != R) return PF_ERR_ARG;

    pf_tagcheck_t *res = (pf_tagcheck_t *)calloc(1, sizeof(pf_tagcheck_t));
    if (!res) return PF_ERR_NOMEM;
    std::unique_ptr<pf_tagcheck_t, void (*)(pf_tagcheck_t *)> own(res, pf_tagcheck_free);  // freed on every return but the last
    res->n_windows = W;
    res->n_reads = R;
    uint32_t *h_wro = (uint32_t *)calloc((size_t)W + 1, 4), *h_nu = (uint32_t *)calloc((size_t)R + 1, 4);
    uint32_t *h_wn = (uint32_t *)calloc(8ull * W + 1, 4);
    int64_t *h_llr = (int64_t *)calloc((size_t)R + 1, 8);
    uint8_t *h_v = (uint8_t *)calloc((size_t)R + 1, 1), *h_hp = (uint8_t *)calloc((size_t)R + 1, 1);
    res->win_read_off = h_wro; res->n_used = h_nu; res->win_n = h_wn; res->llr = h_llr; res->verdict = h_v; res->hp = h_hp;
    if (!h_wro || !h_nu || !h_wn || !h_llr || !h_v || !h_hp) return PF_ERR_NOMEM;
    pf_pile_dev pd;
    memset(&pd, 0, sizeof pd);
    std::unique_ptr<pf_pile_dev, void (*)(pf_pile_dev *)> pd_own(&pd, pf_pile_dev_free);
    std::vector<uint64_t> h_so;
    pf_call call(pf_ctx_stream(ctx));
    hipStream_t st = call.st;
    // the site table under this call's tags (the view above has run the load stage)
    const int prc = pf_batch_pileup_dev(ctx, db, read_hp, n_hp, &pd);
    if (prc) return prc;

    // the tile the kernel gets: no larger than the largest window's sites
    uint32_t T_run = 64;
    if (pd.n_sites) {
        h_so.resize((size_t)W + 1);
        if (hipMemcpyAsync(h_so.data(), pd.win_off, 8ull * ((size_t)W + 1), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PF_ERR_HIP;
        uint64_t most = 0;
        for (uint32_t w = 0; w < W; w++) most = h_so[w + 1] - h_so[w] > most ? h_so[w + 1] - h_so[w] : most;
        while (T_run < T && T_run < most) T_run *= 2;
    }

    tagcheck_args a;
    memset(&a, 0, sizeof a);
    a.W = W; a.T = T_run; a.min_cov = cfg->min_cov; a.min_calls = cfg->min_calls;
    a.min_llr = (long long)cfg->min_llr_q16;
    a.n_sites = pd.n_sites;
    a.v = pf_calls_view_of(d);
    const int hrc = call.upload_hp(read_hp, R, a.v);
    if (hrc) return hrc;
    void *p_so = nullptr;
    if ((!pd.n_sites && !(p_so = call.alloc(8ull * ((size_t)W + 1)))) ||
        (pd.n_sites && !(a.site_w = static_cast<int4 *>(call.alloc(16ull * pd.n_sites)))) ||
        !(a.n_used = static_cast<uint32_t *>(call.alloc(4ull * R))) || !(a.llr = static_cast<long long *>(call.alloc(8ull * R))) ||
        !(a.verdict = static_cast<uint8_t *>(call.alloc(R))) || !(a.win_n = static_cast<uint32_t *>(call.alloc(32ull * W))))
        return PF_ERR_NOMEM;
    a.site_off = pd.n_sites ? pd.win_off : static_cast<const uint64_t *>(p_so);
    a.site_pos = pd.pos; a.site_cnt = pd.cnt;
    // a read that is not scored keeps zeros and 255
    if ((p_so && hipMemsetAsync(p_so, 0, 8ull * ((size_t)W + 1), st) != hipSuccess) ||
        hipMemsetAsync(a.n_used, 0, R ? 4ull * R : 8, st) != hipSuccess || hipMemsetAsync(a.llr, 0, R ? 8ull * R : 8, st) != hipSuccess ||
        hipMemsetAsync(a.win_n, 0, W ? 32ull * W : 8, st) != hipSuccess || hipMemsetAsync(a.verdict, 0xFF, R ? R : 8, st) != hipSuccess)
        return PF_ERR_HIP;
    if (!call.mark(0)) return PF_ERR_HIP;
    if (pd.n_sites) {
        const uint64_t nb = (pd.n_sites + 255u) / 256u;
        if (nb > 0x7FFFFFFFull) return PF_ERR_LIMIT;
        hipLaunchKernelGGL(pf_tagcheck_weights, dim3((uint32_t)nb), dim3(256), 0, st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    }
    if (W) {
        hipLaunchKernelGGL(pf_tagcheck_score, dim3(W), dim3(PF_TAGCHECK_THREADS), TC_LDS(T_run), st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    }
    if (!call.mark(1) ||
        (W && hipMemcpyAsync(h_wro, d.win_read_off, 4ull * ((size_t)W + 1), hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (R && (hipMemcpyAsync(h_nu, a.n_used, 4ull * R, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(h_llr, a.llr, 8ull * R, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(h_v, a.verdict, R, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(h_hp, a.v.read_hp, R, hipMemcpyDeviceToHost, st) != hipSuccess)) ||
        (W && hipMemcpyAsync(h_wn, a.win_n, 32ull * W, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_kernels = call.ms(0, 1);
    *out = own.release();
    return PF_OK;
}
