// pf_site.h -- the per-site rules of the region calls, shared by pf_dmr.hip and
// pf_regions.hip (include/pomfret_amd.h has the definitions): which site is
// informative and which direction it carries.  Host and device compute the same.
#ifndef PF_SITE_H
#define PF_SITE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

// n1 = m1 + u1, n2 = m2 + u2: both haplotypes covered
__host__ __device__ __forceinline__ bool site_informative(uint32_t n1, uint32_t n2, uint32_t min_cov) {
    return !(n1 < min_cov || n2 < min_cov);
}

// the sign code of an informative site (counts at most 65,535 each): 1 for +1,
// 2 for -1, 0 for no direction; d and t in 64 bits
__host__ __device__ __forceinline__ uint32_t site_sign(uint32_t m1, uint32_t n1, uint32_t m2, uint32_t n2,
                                                       uint32_t min_delta_pct) {
    const int64_t d = ((int64_t)m1 * n2 - (int64_t)m2 * n1) * 100;
    const int64_t t = (int64_t)min_delta_pct * n1 * n2;
    return d >= t ? 1u : (-d >= t ? 2u : 0u);
}

#endif
