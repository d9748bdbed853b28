// pf_llr.h -- the integer log-odds shared by pf_assign.hip, pf_tagcheck.hip and
// pf_dmr_hmm.hip (include/pomfret_amd.h has the definitions): the Q16 log2, the
// two weights of pf_batch_assign's informative site, the four leave-one-out
// weights of pf_batch_tagcheck's and the evidence of pf_dmr_hmm_regions'.  Host
// and device compute the same.
#ifndef PF_LLR_H
#define PF_LLR_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PF_LLR_NONE INT32_MIN       /* no weight: a value no weight takes (|w| < 2^22) */

// L(x) of the header, x >= 1
__host__ __device__ inline uint32_t ilog2_q16(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t e = 31u - (uint32_t)__clz((int)x);
#else
    const uint32_t e = 31u - (uint32_t)__builtin_clz(x);
#endif
    uint64_t y = (uint64_t)x << (31u - e);           // [2^31, 2^32)
    uint32_t f = 0;
    for (int i = 0; i < 16; i++) {
        y = (y * y) >> 31;                           // [2^31, 2^33)
        f <<= 1;
        if (y >= 0x100000000ull) { y >>= 1; f |= 1u; }
    }
    return (e << 16) | f;
}

__host__ __device__ inline void site_weights(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2, int32_t *wm, int32_t *wu) {
    const int32_t d = (int32_t)ilog2_q16(m2 + u2 + 2u) - (int32_t)ilog2_q16(m1 + u1 + 2u);
    *wm = (int32_t)ilog2_q16(m1 + 1u) - (int32_t)ilog2_q16(m2 + 1u) + d;
    *wu = (int32_t)ilog2_q16(u1 + 1u) - (int32_t)ilog2_q16(u2 + 1u) + d;
}

// pf_batch_tagcheck's site: w[2*h + c] is the weight of an entry of category c
// on a read tagged h, scored against the counts without that entry.  A tag
// whose entries are not usable at this site gets PF_LLR_NONE in both weights;
// a usable tag's weight for a category nobody of that tag has is 0 (no read
// can look it up, and L(0) is not evaluated).
__host__ __device__ inline void loo_weights(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2, uint32_t min_cov, int32_t w[4]) {
    const uint32_t n1 = m1 + u1, n2 = m2 + u2;
    w[0] = w[1] = w[2] = w[3] = PF_LLR_NONE;
    if (n1 >= 1u && n1 - 1u >= min_cov && n2 >= min_cov) {          // one entry of haplotype 1 taken out
        const int32_t d = (int32_t)ilog2_q16(n2 + 2u) - (int32_t)ilog2_q16(n1 + 1u);
        w[0] = m1 ? (int32_t)ilog2_q16(m1) - (int32_t)ilog2_q16(m2 + 1u) + d : 0;
        w[1] = u1 ? (int32_t)ilog2_q16(u1) - (int32_t)ilog2_q16(u2 + 1u) + d : 0;
    }
    if (n2 >= 1u && n2 - 1u >= min_cov && n1 >= min_cov) {          // one entry of haplotype 2 taken out
        const int32_t d = (int32_t)ilog2_q16(n2 + 1u) - (int32_t)ilog2_q16(n1 + 2u);
        w[2] = m2 ? (int32_t)ilog2_q16(m1 + 1u) - (int32_t)ilog2_q16(m2) + d : 0;
        w[3] = u2 ? (int32_t)ilog2_q16(u1 + 1u) - (int32_t)ilog2_q16(u2) + d : 0;
    }
}

// pf_dmr_hmm_regions' evidence e of an informative site (counts at most 65,535
// each, so every product stays below 2^39): the Laplace-smoothed log-likelihood
// ratio of "two levels" against "one level" in Q16 bits, clamped to [0, 2^28],
// with the sign of m1*n2 - m2*n1.
__host__ __device__ inline int64_t hmm_evidence(uint32_t m1, uint32_t u1, uint32_t m2, uint32_t u2) {
    const uint32_t n1 = m1 + u1, n2 = m2 + u2, m = m1 + m2, u = u1 + u2, n = n1 + n2;
    const int64_t l1 = (int64_t)ilog2_q16(n1 + 2u), l2 = (int64_t)ilog2_q16(n2 + 2u), l = (int64_t)ilog2_q16(n + 2u);
    const int64_t sep = (int64_t)m1 * ((int64_t)ilog2_q16(m1 + 1u) - l1) + (int64_t)u1 * ((int64_t)ilog2_q16(u1 + 1u) - l1) +
                        (int64_t)m2 * ((int64_t)ilog2_q16(m2 + 1u) - l2) + (int64_t)u2 * ((int64_t)ilog2_q16(u2 + 1u) - l2);
    const int64_t pool = (int64_t)m * ((int64_t)ilog2_q16(m + 1u) - l) + (int64_t)u * ((int64_t)ilog2_q16(u + 1u) - l);
    int64_t g = sep - pool;
    if (g < 0) g = 0;
    if (g > ((int64_t)1 << 28)) g = (int64_t)1 << 28;
    const int64_t d = (int64_t)m1 * n2 - (int64_t)m2 * n1;
    return d > 0 ? g : (d < 0 ? -g : 0);
}

#endif
