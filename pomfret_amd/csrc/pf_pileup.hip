// pf_pileup.hip -- per-haplotype CpG methylation pileup (pf_batch_pileup).
//
// The second consumer of a batch's decoded 5mC calls: every call entry of a
// window's reads inside [win_start, win_end) with cat 0 (meth) or 1 (unmeth)
// adds one to cnt[pos][h][cat], h = 0 / 1 for read_hp 0 / 1 and 2 for every
// other tag.  A position with a non-zero counter is a site of the window.
//
// One workgroup per (window, tile of T positions).  The tile's counters live
// in LDS, three u32 per position (one per h: meth in the low, unmeth in the
// high 16 bits; a window holds at most 65,535 reads, so a count only passes
// 65,535 when reads carry duplicate entries at one position -- the add that
// finds its field full sets the status bit and the call fails with
// PF_ERR_LIMIT).  The waves take the window's reads in turn, 64 at a time, by
// the shared read-slice scan of pf_reads.h against the tile's range (most reads
// of a window miss a given tile); what is the pileup's own is the stride over
// each hitting read's calls: coalesced loads and LDS atomics into the tile's
// counters, and no call touches an HBM atomic.  The tile is
// then scanned in position order, ballot / mbcnt prefix counts compacting the
// non-zero positions.  Two passes make the output exactly sized and deterministic:
// pf_pile_count leaves each item's site count, pf_pile_scan the prefix sums
// (item and window offsets), pf_pile_emit rebuilds the non-empty tiles and
// writes their sites where the sums say.  Integer sums: neither atomic order
// nor launch geometry reaches the output.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pf_device.h"
#include "pf_reads.h"

namespace {

template <bool EMIT>
__device__ __forceinline__ void pile_item(const pf_pile_args &a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tile[];   // [3][T]
    __shared__ uint32_t wsum[PF_PILE_WAVES];
    const pf_calls_view &v = a.v;
    const uint32_t item = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t T = a.T;
    if (item >= a.n_items) return;
    uint64_t out0 = 0, out1 = 0;
    if (EMIT) {
        out0 = a.item_off[item];
        out1 = a.item_off[item + 1];
        if (out1 == out0) return;                    // no site: nothing to rebuild
    }
    // the item's window: the last w with tile_off[w] <= item (empty windows share their successor's offset)
    uint32_t w = 0;
    for (uint32_t hi = a.W; hi - w > 1;) {
        const uint32_t mid = w + (hi - w) / 2;
        if (a.tile_off[mid] <= item) w = mid; else hi = mid;
    }
    const uint64_t ws = v.win_start[w], we = v.win_end[w];
    const uint64_t t0 = ws + (uint64_t)(item - a.tile_off[w]) * T;
    const uint64_t t1 = t0 + T < we ? t0 + T : we;
    const uint32_t span = t1 > t0 ? (uint32_t)(t1 - t0) : 0u;          // <= T
    for (uint32_t h = 0; h < 3; h++)
        for (uint32_t i = tid; i < span; i += PF_PILE_THREADS) tile[h * T + i] = 0u;
    __syncthreads();

    const uint32_t r0 = v.win_read_off[w], r1 = v.win_read_off[w + 1];
    bool wrapped = false;
    for (uint32_t g = r0 + wave * 64u; g < r1; g += PF_PILE_WAVES * 64u) {
        // 64 reads at once, one per lane: the lower bound of t0 in the read's
        // sorted slice, and whether the call there lies in the tile
        const uint32_t r = g + lane;
        uint64_t lo = 0, c1 = 0;
        uint32_t h = 2u;
        if (r >= g && r < r1) {
            lo = v.read_call_off[r];
            c1 = v.read_call_end[r];
            const uint32_t hp = v.read_hp[r];
            h = hp < 2u ? hp : 2u;
        }
        const bool hit = slice_seek(v.call_pos, lo, c1, t0, t1);
        // the wave strides over each hitting read's calls from the bound to
        // the tile's end: coalesced loads, LDS atomics
        for (uint64_t m = __ballot(hit); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const uint64_t s = shfl64(lo, l), e = shfl64(c1, l);
            const uint32_t hh = (uint32_t)__shfl((int)h, l);
            for (uint64_t c = s + lane; c < e; c += 64) {
                const uint64_t p = v.call_pos[c];
                const uint32_t cat = v.call_cat[c];  // with the position: one round trip per step
                if (p >= t1) break;
                if (p < t0 || cat > 1u) continue;    // p < t0: never in a sorted slice
                const uint32_t old = atomicAdd(&tile[hh * T + (uint32_t)(p - t0)], cat ? 0x10000u : 1u);
                wrapped |= ((old >> (16u * cat)) & 0xFFFFu) == 0xFFFFu;
            }
        }
    }
    if (wrapped) atomicOr(a.status, 1u);
    __syncthreads();

    // the tile in position order: each round takes PF_PILE_THREADS positions
    uint32_t run = 0;
    for (uint32_t base = 0; base < span; base += PF_PILE_THREADS) {
        const uint32_t i = base + tid;
        uint32_t v0 = 0, v1 = 0, v2 = 0;
        if (i < span) { v0 = tile[i]; v1 = tile[T + i]; v2 = tile[2 * T + i]; }
        const bool nz = (v0 | v1 | v2) != 0u;
        uint32_t tot;
        const uint32_t slot = block_compact(nz, wsum, PF_PILE_WAVES, lane, wave, tot);
        if (EMIT && nz) {
            const uint64_t o = out0 + run + slot;
            if (o < out1) {                          // holds: both passes count the same calls
                a.out_pos[o] = (uint32_t)t0 + i;
                uint2 *q = reinterpret_cast<uint2 *>(a.out_cnt + 6 * o);
                q[0] = make_uint2(v0 & 0xFFFFu, v0 >> 16);
                q[1] = make_uint2(v1 & 0xFFFFu, v1 >> 16);
                q[2] = make_uint2(v2 & 0xFFFFu, v2 >> 16);
            }
        }
        run += tot;
        __syncthreads();
    }
    if (!EMIT && tid == 0) a.item_cnt[item] = run;
}

}  // namespace

__global__ __launch_bounds__(PF_PILE_THREADS) void pf_pile_count(pf_pile_args a) { pile_item<false>(a); }
__global__ __launch_bounds__(PF_PILE_THREADS) void pf_pile_emit(pf_pile_args a) { pile_item<true>(a); }

// item_off = exclusive prefix sums of item_cnt (item_off[n_items] the total),
// win_off[w] = item_off[tile_off[w]]: one workgroup, each thread a contiguous
// run of items
__global__ __launch_bounds__(PF_PILE_SCAN_THREADS) void pf_pile_scan(pf_pile_args a) {
    __shared__ uint64_t part[PF_PILE_SCAN_THREADS];
    const uint32_t tid = threadIdx.x, n = a.n_items;
    const uint32_t chunk = (n + PF_PILE_SCAN_THREADS - 1) / PF_PILE_SCAN_THREADS;
    const uint64_t b0 = (uint64_t)tid * chunk;
    const uint32_t i0 = (uint32_t)(b0 < n ? b0 : n), i1 = (uint32_t)(b0 + chunk < n ? b0 + chunk : n);
    uint64_t s = 0;
    for (uint32_t i = i0; i < i1; i++) s += a.item_cnt[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t d = 1; d < PF_PILE_SCAN_THREADS; d <<= 1) {
        const uint64_t v = tid >= d ? part[tid - d] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint64_t o = part[tid] - s;
    for (uint32_t i = i0; i < i1; i++) {
        a.item_off[i] = o;
        o += a.item_cnt[i];
    }
    if (tid == PF_PILE_SCAN_THREADS - 1) a.item_off[n] = part[tid];
    __threadfence();
    __syncthreads();
    for (uint32_t w = tid; w <= a.W; w += PF_PILE_SCAN_THREADS) a.win_off[w] = a.item_off[a.tile_off[w]];
}
