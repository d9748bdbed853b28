// pf_assign.hip -- tags for untagged reads from a window's allele-specific
// methylation (pf_batch_assign; include/pomfret_amd.h has the definition).
//
// The site table is the pileup's: pf_batch_pileup_dev (pf_api.hip) runs the
// pileup kernels under the call's tags and leaves the per-window site CSR (pos,
// cnt) in HBM.  Two kernels follow, all in integers.
//
// pf_assign_weights, one thread per site: the two Laplace-smoothed log-odds of
// an informative site from six evaluations of the Q16 log2 (sixteen squarings
// of a 32-bit mantissa each, no table), stored as one int2 beside the site.  A
// site that is not informative gets ASSIGN_NONE in the first weight -- a value
// no weight takes (|w| < 2^22) -- so that an informative site whose weights are
// both 0 stays distinct from it.
//
// pf_assign_score, one workgroup per window.  The window's sites go through
// LDS in tiles of T (position and the weight pair, 12 B per site; one tile for
// every region hapmeth meets).  Per tile the waves take the window's reads 64
// at a time, one per lane, read index -> (wave, lane) fixed: a candidate (tag
// 254) whose sorted call slice misses the tile's position range needs no
// search, the others binary-search the slice for the tile's first position;
// the wave then strides over each hitting read's calls up to the tile's last
// position, every lane binary-searching its call's position in the LDS tile,
// and reduces the int64 sum and the count once per read.  A read's running sum
// lives in its own row of the output between tiles, read and written by the
// one lane that owns the read: no atomics.  After the last tile that lane
// applies the decision and writes the row; the window's three counters are
// ballot counts added in LDS.  Integer sums: neither the tile nor the
// workgroup size reaches the result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include "pf_device.h"
#include "pf_llr.h"                 // ilog2_q16, site_weights: shared with pf_tagcheck.hip
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

#define ASSIGN_NONE PF_LLR_NONE     /* first weight of a site that is not informative */

struct assign_args {
    uint32_t W, T, min_cov, min_calls;
    long long min_llr;
    uint64_t n_sites;
    pf_calls_view v;                                 /* read_hp: the batch's tags or the caller's */
    const uint64_t *site_off;                        /* [W+1] */
    const uint32_t *site_pos;                        /* [n_sites] */
    const uint32_t *site_cnt;                        /* [n_sites*6] */
    int2 *site_w;                                    /* [n_sites] wM, wU; wM == ASSIGN_NONE: not informative */
    uint32_t *n_used;                                /* [R] */
    long long *llr;                                  /* [R] */
    uint8_t *hp;                                     /* [R] */
    uint32_t *win_n;                                 /* [W*3] */
};

}  // namespace

__global__ __launch_bounds__(256) void pf_assign_weights(assign_args a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_sites) return;
    const uint2 *c = reinterpret_cast<const uint2 *>(a.site_cnt + 6 * i);
    const uint2 h1 = c[0], h2 = c[1];
    int2 w = make_int2(ASSIGN_NONE, 0);
    if (h1.x + h1.y >= a.min_cov && h2.x + h2.y >= a.min_cov) site_weights(h1.x, h1.y, h2.x, h2.y, &w.x, &w.y);
    a.site_w[i] = w;
}

__global__ __launch_bounds__(PF_ASSIGN_THREADS) void pf_assign_score(assign_args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tile[];   // pos [T], wM [T], wU [T]
    __shared__ uint32_t s_n[3];
    const uint32_t w = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t T = a.T;
    if (w >= a.W) return;
    uint32_t *s_pos = s_tile;
    int32_t *s_wm = reinterpret_cast<int32_t *>(s_tile + T), *s_wu = reinterpret_cast<int32_t *>(s_tile + 2u * T);
    if (tid < 3u) s_n[tid] = 0u;
    const uint64_t s0 = a.site_off[w], s1 = a.site_off[w + 1];
    const uint32_t r0 = a.v.win_read_off[w], r1 = a.v.win_read_off[w + 1];
    const uint64_t n_tiles = s1 > s0 ? (s1 - s0 + T - 1) / T : 1;      // a window without sites: one empty tile
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t b0 = s0 + t * T;
        const uint32_t n = b0 < s1 ? (uint32_t)(s1 - b0 < T ? s1 - b0 : T) : 0u;
        __syncthreads();                              // the previous tile's readers are done
        for (uint32_t i = tid; i < n; i += PF_ASSIGN_THREADS) {
            const int2 ww = a.site_w[b0 + i];
            s_pos[i] = a.site_pos[b0 + i];
            s_wm[i] = ww.x;
            s_wu[i] = ww.y;
        }
        __syncthreads();
        const uint32_t p_lo = n ? s_pos[0] : 0u, p_hi = n ? s_pos[n - 1u] : 0u;
        const bool first = t == 0, last = t + 1 == n_tiles;
        for (uint32_t g = r0 + wave * 64u; g < r1; g += PF_ASSIGN_WAVES * 64u) {
            const uint32_t r = g + lane;
            const bool have = r >= g && r < r1;
            const uint32_t hp = have ? a.v.read_hp[r] : 0u;
            const bool cand = have && hp == 254u;
            uint64_t lo = 0, c1 = 0;
            if (cand && n) {
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
            long long my_s = 0;
            uint32_t my_n = 0;
            for (uint64_t m = __ballot(hit); m; m &= m - 1) {
                const int l = __builtin_ctzll(m);
                const uint64_t s = shfl64(lo, l);
                const uint64_t e = shfl64(c1, l);
                long long acc = 0;
                uint32_t cn = 0;
                for (uint64_t c0 = s; c0 < e; c0 += 64) {
                    const uint64_t c = c0 + lane;
                    const bool valid = c < e;
                    const uint32_t p = valid ? a.v.call_pos[c] : 0u;
                    const uint32_t cat = valid ? a.v.call_cat[c] : 2u;
                    if (valid && p <= p_hi && cat < 2u) {     // p >= p_lo: the slice is sorted and starts at the bound
                        uint32_t k = 0;
                        for (uint32_t hi = n; k < hi;) {
                            const uint32_t mid = k + (hi - k) / 2;
                            if (s_pos[mid] < p) k = mid + 1; else hi = mid;
                        }
                        if (k < n && s_pos[k] == p) {
                            const int32_t wm = s_wm[k];
                            if (wm != ASSIGN_NONE) {
                                acc += cat ? s_wu[k] : wm;
                                cn++;
                            }
                        }
                    }
                    if (__ballot(valid && p > p_hi)) break;   // past the tile's last position
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const uint32_t al = (uint32_t)__shfl_xor((int)(uint32_t)acc, d);
                    const uint32_t ah = (uint32_t)__shfl_xor((int)(uint32_t)((unsigned long long)acc >> 32), d);
                    acc += (long long)(((unsigned long long)ah << 32) | al);
                    cn += (uint32_t)__shfl_xor((int)cn, d);
                }
                my_s = lane == (uint32_t)l ? acc : my_s;
                my_n = lane == (uint32_t)l ? cn : my_n;
            }
            // the read's row: its lane alone reads and writes it
            if (cand && !first) {
                my_s += a.llr[r];
                my_n += a.n_used[r];
            }
            if (last) {
                uint32_t tag = hp;
                if (cand && my_n >= a.min_calls) {
                    if (my_s > 0 && my_s >= a.min_llr) tag = 0u;
                    else if (my_s < 0 && -my_s >= a.min_llr) tag = 1u;
                }
                if (have) {
                    a.hp[r] = (uint8_t)tag;
                    a.llr[r] = cand ? my_s : 0ll;
                    a.n_used[r] = cand ? my_n : 0u;
                }
                const uint64_t b_sc = __ballot(cand && my_n >= 1u), b_0 = __ballot(cand && tag == 0u), b_1 = __ballot(cand && tag == 1u);
                if (lane == 0u) {
                    if (b_sc) atomicAdd(&s_n[0], (uint32_t)__popcll(b_sc));
                    if (b_0) atomicAdd(&s_n[1], (uint32_t)__popcll(b_0));
                    if (b_1) atomicAdd(&s_n[2], (uint32_t)__popcll(b_1));
                }
            } else if (cand) {
                a.llr[r] = my_s;
                a.n_used[r] = my_n;
            }
        }
    }
    __syncthreads();
    if (tid < 3u) a.win_n[3ull * w + tid] = s_n[tid];
}

// ---- host side
extern "C" uint32_t pf_ilog2_q16(uint32_t x) { return x ? ilog2_q16(x) : 0u; }

extern "C" void pf_assign_site_weights(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2, int32_t w[2]) {
    if (!w) return;
    // the header's range: a count above 65,535 is no pileup count
    if (m1 > 0xFFFFu) m1 = 0xFFFFu;
    if (u1 > 0xFFFFu) u1 = 0xFFFFu;
    if (m2 > 0xFFFFu) m2 = 0xFFFFu;
    if (u2 > 0xFFFFu) u2 = 0xFFFFu;
    site_weights(m1, u1, m2, u2, &w[0], &w[1]);
}

extern "C" void pf_assign_free(pf_assign_t *p) {
    if (!p) return;
    free(const_cast<uint32_t *>(p->win_read_off));
    free(const_cast<uint32_t *>(p->n_used));
    free(const_cast<int64_t *>(p->llr));
    free(const_cast<uint8_t *>(p->hp));
    free(const_cast<uint32_t *>(p->win_n));
    free(p);
}

extern "C" int pf_batch_assign(pf_ctx_t *ctx, pf_dbatch_t *db, const uint8_t *read_hp, uint32_t n_hp, const pf_assign_cfg_t *cfg,
                               pf_assign_t **out) {
    if (!ctx || !db || !out || !cfg) return PF_ERR_ARG;
    *out = nullptr;
    const uint32_t T = pf_env_pow2("PF_ASSIGN_TILE", 64, PF_ASSIGN_TILE, PF_ASSIGN_TILE);
    if (!T) return PF_ERR_ARG;
    pf_dev_batch d;
    const int vrc = pf_batch_calls_view(ctx, db, &d);
    if (vrc) return vrc;
    const uint32_t W = d.W, R = d.R;
    if (read_hp && n_hp != R) return PF_ERR_ARG;

    pf_assign_t *res = (pf_assign_t *)calloc(1, sizeof(pf_assign_t));
    if (!res) return PF_ERR_NOMEM;
    std::unique_ptr<pf_assign_t, void (*)(pf_assign_t *)> own(res, pf_assign_free);    // freed on every return but the last
    res->n_windows = W;
    res->n_reads = R;
    uint32_t *h_wro = (uint32_t *)calloc((size_t)W + 1, 4), *h_nu = (uint32_t *)calloc((size_t)R + 1, 4);
    uint32_t *h_wn = (uint32_t *)calloc(3ull * W + 1, 4);
    int64_t *h_llr = (int64_t *)calloc((size_t)R + 1, 8);
    uint8_t *h_hp = (uint8_t *)calloc((size_t)R + 1, 1);
    res->win_read_off = h_wro; res->n_used = h_nu; res->win_n = h_wn; res->llr = h_llr; res->hp = h_hp;
    if (!h_wro || !h_nu || !h_wn || !h_llr || !h_hp) return PF_ERR_NOMEM;
    pf_pile_dev pd;
    memset(&pd, 0, sizeof pd);
    std::unique_ptr<pf_pile_dev, void (*)(pf_pile_dev *)> pd_own(&pd, pf_pile_dev_free);
    pf_call call(pf_ctx_stream(ctx));
    hipStream_t st = call.st;
    // the site table under this call's tags (the view above has run the load stage)
    const int prc = pf_batch_pileup_dev(ctx, db, read_hp, n_hp, &pd);
    if (prc) return prc;

    assign_args a;
    memset(&a, 0, sizeof a);
    a.W = W; a.T = T; a.min_cov = cfg->min_cov; a.min_calls = cfg->min_calls;
    a.min_llr = (long long)cfg->min_llr_q16;
    a.n_sites = pd.n_sites;
    a.v = pf_calls_view_of(d);
    const int hrc = call.upload_hp(read_hp, R, a.v);
    if (hrc) return hrc;
    void *p_so = nullptr;
    if ((!pd.n_sites && !(p_so = call.alloc(8ull * ((size_t)W + 1)))) ||
        (pd.n_sites && !(a.site_w = static_cast<int2 *>(call.alloc(8ull * pd.n_sites)))) ||
        !(a.n_used = static_cast<uint32_t *>(call.alloc(4ull * R))) || !(a.llr = static_cast<long long *>(call.alloc(8ull * R))) ||
        !(a.hp = static_cast<uint8_t *>(call.alloc(R))) || !(a.win_n = static_cast<uint32_t *>(call.alloc(12ull * W))))
        return PF_ERR_NOMEM;
    a.site_off = pd.n_sites ? pd.win_off : static_cast<const uint64_t *>(p_so);
    a.site_pos = pd.pos; a.site_cnt = pd.cnt;
    // a read outside every window keeps its tag and zeros
    if ((p_so && hipMemsetAsync(p_so, 0, 8ull * ((size_t)W + 1), st) != hipSuccess) ||
        hipMemsetAsync(a.n_used, 0, R ? 4ull * R : 8, st) != hipSuccess || hipMemsetAsync(a.llr, 0, R ? 8ull * R : 8, st) != hipSuccess ||
        hipMemsetAsync(a.win_n, 0, W ? 12ull * W : 8, st) != hipSuccess ||
        (R && hipMemcpyAsync(a.hp, a.v.read_hp, R, hipMemcpyDeviceToDevice, st) != hipSuccess))
        return PF_ERR_HIP;
    if (!call.mark(0)) return PF_ERR_HIP;
    if (pd.n_sites) {
        const uint64_t nb = (pd.n_sites + 255u) / 256u;
        if (nb > 0x7FFFFFFFull) return PF_ERR_LIMIT;
        hipLaunchKernelGGL(pf_assign_weights, dim3((uint32_t)nb), dim3(256), 0, st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    }
    if (W) {
        hipLaunchKernelGGL(pf_assign_score, dim3(W), dim3(PF_ASSIGN_THREADS), 12u * T, st, a);
        if (hipGetLastError() != hipSuccess) return PF_ERR_HIP;
    }
    if (!call.mark(1) ||
        (W && hipMemcpyAsync(h_wro, d.win_read_off, 4ull * ((size_t)W + 1), hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (R && (hipMemcpyAsync(h_nu, a.n_used, 4ull * R, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(h_llr, a.llr, 8ull * R, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipMemcpyAsync(h_hp, a.hp, R, hipMemcpyDeviceToHost, st) != hipSuccess)) ||
        (W && hipMemcpyAsync(h_wn, a.win_n, 12ull * W, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return PF_ERR_HIP;
    res->ms_kernels = call.ms(0, 1);
    *out = own.release();
    return PF_OK;
}
