// pf_reads.h -- the read-slice scan the per-window consumers of a batch's
// calls share (pf_pileup.hip, pf_perm.hip, pf_rank.hip), as device helpers, and
// the view of the batch that every consumer's arguments embed (those three,
// pf_assign.hip and pf_tagcheck.hip) with the host function that fills it.
//
// A window's (or tile's) reads are taken one per lane.  A read's calls are the
// slice [read_call_off[r], read_call_end[r]) of call_pos / call_cat, sorted by
// position.  slice_seek drops a slice that ends left of a position range or
// starts right of it and binary-searches the others for the range's first
// position.  The wave then takes the hitting lanes in turn -- shfl64
// broadcasts the lane's (lo, end) -- and strides over the calls 64 at a time
// until one passes the range's end: slice_count counts the meth and unmeth
// entries.  block_compact gives the flagged lanes of a workgroup consecutive
// slots in thread order.  pf_assign_score and pf_tagcheck_score keep their own
// seek and their sum over an LDS tile of sites: built from these pieces they
// measured 2 to 5 % slower (profiles/read_scan/README.md).
#ifndef PF_READS_H
#define PF_READS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pf_device.h"

// the view of pf_dev_batch; the tags are the batch's until a call overrides them (pf_call::upload_hp)
static inline pf_calls_view pf_calls_view_of(const pf_dev_batch &d) {
    pf_calls_view v;
    v.win_start = d.win_start; v.win_end = d.win_end; v.win_read_off = d.win_read_off;
    v.read_hp = d.read_hp;
    v.read_call_off = d.read_call_off; v.read_call_end = d.read_call_end;
    v.call_pos = d.call_pos; v.call_cat = d.call_cat;
    return v;
}

// the set lanes of bal below this one
__device__ __forceinline__ uint32_t lane_prefix(uint64_t bal) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// lane l's x in every lane
__device__ __forceinline__ uint64_t shfl64(uint64_t x, int l) {
    return ((uint64_t)(uint32_t)__shfl((int)(x >> 32), l) << 32) | (uint32_t)__shfl((int)x, l);
}

// the wave's sum in every lane
__device__ __forceinline__ uint32_t wave_sum32(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d);
    return x;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t x, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += shfl_xor64(x, d);
    return x;
}

// The lane's read against the position range [first, last): lo becomes the
// first call of the sorted slice [lo, c1) at or right of first -- c1 without a
// search where the slice ends left of the range or starts right of it -- and
// the result says whether that call lies in the range.  P: the positions' type.
template <typename P>
__device__ __forceinline__ bool slice_seek(const uint32_t *call_pos, uint64_t &lo, uint64_t c1, P first, P last) {
    if (lo < c1 && (call_pos[c1 - 1] < first || call_pos[lo] >= last)) lo = c1;
    for (uint64_t hi = c1; lo < hi;) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (call_pos[mid] < first) lo = mid + 1; else hi = mid;
    }
    return lo < c1 && call_pos[lo] < last;
}

// One wave, (s, e, end) the same in every lane: the meth and unmeth entries of
// the calls [s, e) left of end, two ballots per 64 calls.  s is slice_seek's
// bound, so no call lies left of the range.
__device__ __forceinline__ void slice_count(const pf_calls_view &v, uint64_t s, uint64_t e, uint32_t end, uint32_t lane,
                                            uint32_t &cm, uint32_t &cu) {
    cm = 0; cu = 0;
    for (uint64_t c0 = s; c0 < e; c0 += 64) {
        const uint64_t c = c0 + lane;
        const bool valid = c < e;
        const uint32_t p = valid ? v.call_pos[c] : 0u;
        const uint32_t cat = valid ? v.call_cat[c] : 2u;
        const bool in = valid && p < end;
        cm += (uint32_t)__popcll(__ballot(in && cat == 0u));
        cu += (uint32_t)__popcll(__ballot(in && cat == 1u));
        if (__ballot(valid && !in)) break;            // past the range's end
    }
}

// The flagged threads of a workgroup of nw waves in thread order: the result is
// the thread's slot among them (meaningful where flag is set), tot their number.
// wsum holds one word per wave.  There is a barrier inside: every thread of the
// workgroup calls this, and the caller puts a barrier between one call's reads
// of wsum and the next call.
__device__ __forceinline__ uint32_t block_compact(bool flag, uint32_t *wsum, uint32_t nw, uint32_t lane, uint32_t wave,
                                                  uint32_t &tot) {
    const uint64_t bal = __ballot(flag);
    if (lane == 0u) wsum[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0;
    tot = 0;
    for (uint32_t k = 0; k < nw; k++) {
        const uint32_t s = wsum[k];
        before += k < wave ? s : 0u;
        tot += s;
    }
    return before + lane_prefix(bal);
}

// One round of a window's reads, workgroup-wide, one read per thread: read
// g + tid of the reads [.., r1) against the window [ws, we).  hp is the read's
// tag (2 where the thread has no read); hit says that a read tagged 0 or 1 has
// a call in the window, and then my_m / my_u are its meth / unmeth entries
// there.  No barrier; whole waves call it.
__device__ __forceinline__ void window_read_counts(const pf_calls_view &v, uint32_t g, uint32_t r1, uint32_t ws, uint32_t we,
                                                   uint32_t tid, uint32_t &hp, bool &hit, uint32_t &my_m, uint32_t &my_u) {
    const uint32_t r = g + tid, lane = tid & 63u;
    uint64_t lo = 0, c1 = 0;
    hp = 2u;
    if (r >= g && r < r1) {
        lo = v.read_call_off[r];
        c1 = v.read_call_end[r];
        hp = v.read_hp[r];
    }
    if (hp > 1u) lo = c1;                             // untagged, HP >= 3: not a read of the test
    hit = slice_seek(v.call_pos, lo, c1, ws, we);
    my_m = 0; my_u = 0;
    for (uint64_t m = __ballot(hit); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        uint32_t cm, cu;                              // wave-uniform
        slice_count(v, shfl64(lo, l), shfl64(c1, l), we, lane, cm, cu);
        my_m = lane == (uint32_t)l ? cm : my_m;
        my_u = lane == (uint32_t)l ? cu : my_u;
    }
}

#endif
