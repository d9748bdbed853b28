// pf_mdsynth.hip -- MD:Z synthesised on gfx950 from CIGAR, SEQ and the
// reference (DESIGN.md "MD synthesis"), for BAMs whose records carry no MD
// tag: the -u pre-pass's K4 (pf_haptag.hip) then reads the synthesised bytes
// exactly as it reads a tag.
//
// One wavefront per read, as K4 is laid out, and two passes over the same
// walk: pf_k4_mdlen writes each read's byte count, the host's exclusive scan
// turns the counts into md_off (the host needs the counts anyway: they size
// K4's scratch), pf_k4_mdfill writes the bytes.
//
// The walk: CIGAR ops 64 a step, with wave prefix sums for each op's
// reference start, query start and "match coordinate" (the number of M/=/X
// bases before it).  The M/=/X and D ops of a step are then visited in order
// (a ballot mask, the op's values taken by readlane):
//   M/=/X: bases 64 a step; every lane compares its SEQ and reference
//     nibbles, a ballot gives the mismatch mask.  A step without a mismatch
//     costs nothing more.  Otherwise each mismatch lane's preceding run is its
//     match coordinate minus that of the previous event (the previous set bit
//     of the mask, or the wave-uniform coordinate carried from earlier steps
//     and ops), its bytes are digits(run) + 1, and a wave scan of the byte
//     counts places them;
//   D: digits(run) + 1 + l bytes, the letters written by all lanes.
// The run that closes the string is the total match coordinate minus the
// carried one.  No LDS, no scratch; plain vector stores.
#include <hip/hip_runtime.h>
#include "pf_ingest.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>
#include "../../include/pomfret_amd.h"

#define MD_WAVES 4

struct pf_md_dev {
    uint32_t n_reads;
    const uint32_t *start;
    const uint64_t *cigar_off;
    const uint32_t *cigar;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    const uint8_t *seq;
    const uint8_t *ref;          // packed nibbles, high nibble first
    uint64_t ref_len;
    uint32_t *md_len;            // pf_k4_mdlen: [n_reads]
    const uint64_t *md_off;      // pf_k4_mdfill: [n_reads + 1]
    uint8_t *md;
    uint32_t *err;               // bit 0: an M/=/X/D op past the contig's end; bit 1: MD of 2^31 bytes or more
};

static __device__ __forceinline__ uint32_t md_uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
static __device__ __forceinline__ uint32_t md_rdl(uint32_t x, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)l);
}
static __device__ __forceinline__ uint64_t md_rdl64(uint64_t x, uint32_t l) {
    return (uint64_t)md_rdl((uint32_t)(x >> 32), l) << 32 | md_rdl((uint32_t)x, l);
}
static __device__ __forceinline__ uint64_t md_lt(uint32_t lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }
static __device__ __forceinline__ uint32_t md_shr_add(uint32_t x, const int ctrl) {
    uint32_t y;
    switch (ctrl) {
    case 1: y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true); break;
    case 2: y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true); break;
    case 4: y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true); break;
    case 8: y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true); break;
    case 15: y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false); break;
    default: y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false); break;
    }
    return x + y;
}
// inclusive wave prefix sum (row_shr within 16-lane rows, row_bcast carries), as K4's
static __device__ __forceinline__ uint32_t md_scan(uint32_t x) {
    x = md_shr_add(x, 1);
    x = md_shr_add(x, 2);
    x = md_shr_add(x, 4);
    x = md_shr_add(x, 8);
    x = md_shr_add(x, 15);
    x = md_shr_add(x, 31);
    return x;
}
static __device__ __forceinline__ uint32_t md_nib(const uint8_t *p, uint64_t i) {
    return (p[i >> 1] >> ((~(uint32_t)i & 1u) << 2)) & 0xfu;
}
// "=ACMGRSVTWYHKDBN"[c]
static __device__ __forceinline__ uint8_t md_letter(uint32_t c) {
    const uint64_t t = c < 8 ? 0x565352474D43413Dull : 0x4E42444B48595754ull;
    return (uint8_t)(t >> ((c & 7u) << 3));
}
static __device__ __forceinline__ uint32_t md_digits(uint32_t u) {
    return 1u + (u >= 10u) + (u >= 100u) + (u >= 1000u) + (u >= 10000u) + (u >= 100000u) + (u >= 1000000u) +
           (u >= 10000000u) + (u >= 100000000u) + (u >= 1000000000u);
}
// every store of the fill pass stays inside the read's slice [0, cap)
static __device__ __forceinline__ void md_put(uint8_t *out, uint64_t cap, uint64_t i, uint8_t v) {
    if (i < cap) out[i] = v;
}
static __device__ __forceinline__ void md_put_dec(uint8_t *out, uint64_t cap, uint64_t at, uint32_t u, uint32_t nd) {
    for (uint32_t i = nd; i-- > 0;) {
        md_put(out, cap, at + i, (uint8_t)('0' + u % 10u));
        u /= 10u;
    }
}

template <bool FILL>
static __device__ __forceinline__ void md_walk(const pf_md_dev &d) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = md_uni(blockIdx.x * MD_WAVES + (threadIdx.x >> 6));
    if (r >= d.n_reads) return;
    const uint64_t c0 = d.cigar_off[r];
    const uint32_t ncig = md_uni((uint32_t)(d.cigar_off[r + 1] - c0));
    const uint32_t *cig = d.cigar + c0;
    const uint8_t *seq = d.seq + d.seq_off[r];
    const uint32_t lq = md_uni(d.seq_len[r]);
    const uint64_t start = md_uni(d.start[r]);
    uint8_t *out = nullptr;
    uint64_t cap = 0;
    if (FILL) {
        const uint64_t m0 = d.md_off[r];
        out = d.md + m0;
        cap = d.md_off[r + 1] - m0;
    }
    uint64_t o = 0;              // bytes so far
    uint32_t base = 0;           // match coordinate after the previous event
    uint64_t cr = 0, cq = 0;     // reference / query bases before this step's ops
    uint32_t cm = 0;             // M/=/X bases before them
    for (uint32_t b = 0; b < ncig; b += 64) {
        const uint32_t c = b + lane;
        const uint32_t w = c < ncig ? cig[c] : 0xFu;
        const uint32_t op = w & 0xf, l = w >> 4;
        const bool isM = op == 0 || op == 7 || op == 8;
        const uint32_t rl = (isM || op == 2 || op == 3) ? l : 0u;
        const uint32_t ql = (isM || op == 1 || op == 4) ? l : 0u;
        const uint32_t ml = isM ? l : 0u;
        // 64 lengths below 2^28 sum past 32 bits: low and high halves apart
        const uint64_t sr = ((uint64_t)md_scan(rl >> 16) << 16) + md_scan(rl & 0xffffu);
        const uint64_t sq = ((uint64_t)md_scan(ql >> 16) << 16) + md_scan(ql & 0xffffu);
        const uint32_t sm = md_scan(ml);
        const uint64_t xr = cr + sr - rl, xq = cq + sq - ql;
        const uint32_t xm = cm + sm - ml;
        uint64_t act = __ballot((isM && l > 0) || op == 2);
        while (act) {
            const uint32_t k = md_uni((uint32_t)__ffsll((long long)act) - 1u);
            act &= act - 1;
            const uint32_t kw = md_rdl(w, k), kop = kw & 0xf, kl = kw >> 4;
            const uint64_t x = start + md_rdl64(xr, k), y = md_rdl64(xq, k);
            const uint32_t m = md_rdl(xm, k);
            if (x + kl > d.ref_len) {
                if (lane == 0) { atomicOr(d.err, 1u); if (!FILL) d.md_len[r] = 0; }
                return;
            }
            if (kop == 2) {
                const uint32_t u = m - base, nd = md_digits(u);
                if (FILL) {
                    if (lane == 0) {
                        md_put_dec(out, cap, o, u, nd);
                        md_put(out, cap, o + nd, (uint8_t)'^');
                    }
                    for (uint32_t j = lane; j < kl; j += 64)
                        md_put(out, cap, o + nd + 1 + j, md_letter(md_nib(d.ref, x + j)));
                }
                o += (uint64_t)nd + 1 + kl;
                base = m;
                continue;
            }
            for (uint32_t j0 = 0; j0 < kl; j0 += 64) {
                const uint32_t j = j0 + lane;
                bool mis = false;
                uint32_t c2 = 0;
                if (j < kl) {
                    const uint64_t qi = y + j;
                    const uint32_t c1 = qi < lq ? md_nib(seq, qi) : 15u;
                    c2 = md_nib(d.ref, x + j);
                    mis = !(c1 == 0 || (c1 == c2 && c1 != 15u));
                }
                const uint64_t mm = __ballot(mis);
                if (!mm) continue;
                const uint64_t below = mm & md_lt(lane);
                const uint32_t after_prev = below ? m + j0 + 64u - (uint32_t)__clzll((long long)below) : base;
                const uint32_t u = m + j - after_prev, nd = md_digits(u);
                const uint32_t nb = mis ? nd + 1u : 0u;
                const uint32_t sc = md_scan(nb);
                if (FILL && mis) {
                    const uint64_t at = o + sc - nb;
                    md_put_dec(out, cap, at, u, nd);
                    md_put(out, cap, at + nd, md_letter(c2));
                }
                o += md_rdl(sc, 63);
                base = m + j0 + 64u - (uint32_t)__clzll((long long)mm);
            }
        }
        cr += md_rdl64(sr, 63);
        cq += md_rdl64(sq, 63);
        cm += md_rdl(sm, 63);
    }
    const uint32_t u = cm - base, nd = md_digits(u);
    if (FILL) {
        if (lane == 0) md_put_dec(out, cap, o, u, nd);
    } else if (lane == 0) {
        o += nd;
        if (o >> 31) { atomicOr(d.err, 2u); o = 0; }
        d.md_len[r] = (uint32_t)o;
    }
}

__global__ __launch_bounds__(64 * MD_WAVES) void pf_k4_mdlen(pf_md_dev d) { md_walk<false>(d); }
__global__ __launch_bounds__(64 * MD_WAVES) void pf_k4_mdfill(pf_md_dev d) { md_walk<true>(d); }

// ------------------------------------------------------------------------
// host side
extern "C" int pf_ctx_device(const pf_ctx *c);
extern "C" hipStream_t pf_ctx_stream(const pf_ctx *c);

namespace {

// per context: the contig reference it holds on the device (the device fetch
// uploads a contig's nibbles once and keeps them until the context moves to
// another contig) and the synthesis counters
struct MdCtx {
    const uint8_t *h_nib = nullptr;   // host nibbles the device copy was made from
    uint64_t len = 0;
    uint8_t *d_ref = nullptr;
    pf_md_stats_t st = {0, 0, 0, 0.0, 0.0};
};
std::mutex g_md_mu;
std::map<const pf_ctx_t *, MdCtx> g_md;

template <typename T>
hipError_t md_up(std::vector<void *> &al, T **dst, const T *src, size_t n, size_t pad = 0) {
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n + pad, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    al.push_back(p);
    *dst = (T *)p;
    if (n && src) e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

}  // namespace

#define MCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "[E::pomfret_amd] %s: %s\n", #x, hipGetErrorString(e_)); rc = PF_ERR_HIP; goto done; } } while (0)

// The two kernels over reads whose arrays are on the device (in: start,
// cigar_off, cigar, seq_off, seq_len, seq): md_len[N] on the host, *d_md_off
// [N + 1] and *d_md on the device, both appended to `al` (the caller frees).
// Returns with the stream drained.
int pf_mdsynth_dev(pf_ctx_t *ctx, hipStream_t st, uint32_t N, const pf_k4_reads_dev &in, const uint8_t *d_ref,
                   uint64_t ref_len, std::vector<uint32_t> &md_len, std::vector<uint64_t> &md_off,
                   std::vector<void *> &al, uint64_t **d_md_off, uint8_t **d_md) {
    int rc = PF_OK;
    md_len.assign(N, 0);
    md_off.assign((size_t)N + 1, 0);
    if (ref_len >> 32) return PF_ERR_LIMIT;
    pf_md_dev d;
    memset(&d, 0, sizeof d);
    uint32_t *d_len = nullptr, *d_err = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    uint32_t err = 0;
    float ms_len = 0.f, ms_fill = 0.f;
    const dim3 grid((N + MD_WAVES - 1) / MD_WAVES), block(64 * MD_WAVES);
    d.n_reads = N;
    d.start = in.start; d.cigar_off = in.cigar_off; d.cigar = in.cigar;
    d.seq_off = in.seq_off; d.seq_len = in.seq_len; d.seq = in.seq;
    d.ref = d_ref; d.ref_len = ref_len;
    MCHK(hipMalloc((void **)&d_len, std::max<size_t>(N, 1) * 4));
    MCHK(hipMalloc((void **)&d_err, 4));
    MCHK(hipMemsetAsync(d_err, 0, 4, st));
    for (int i = 0; i < 3; i++) MCHK(hipEventCreate(&ev[i]));
    d.md_len = d_len; d.err = d_err;
    MCHK(hipEventRecord(ev[0], st));
    if (N) {
        hipLaunchKernelGGL(pf_k4_mdlen, grid, block, 0, st, d);
        MCHK(hipGetLastError());
    }
    MCHK(hipEventRecord(ev[1], st));
    if (N) MCHK(hipMemcpyAsync(md_len.data(), d_len, 4ull * N, hipMemcpyDeviceToHost, st));
    MCHK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    if (err) { rc = (err & 1u) ? PF_ERR_ARG : PF_ERR_LIMIT; goto done; }
    for (uint32_t r = 0; r < N; r++) md_off[r + 1] = md_off[r] + md_len[r];
    {
        void *p = nullptr;
        MCHK(hipMalloc(&p, ((size_t)N + 1) * 8));
        al.push_back(p);
        *d_md_off = (uint64_t *)p;
        MCHK(hipMalloc(&p, md_off[N] + 16));
        al.push_back(p);
        *d_md = (uint8_t *)p;
    }
    MCHK(hipMemcpyAsync(*d_md_off, md_off.data(), ((size_t)N + 1) * 8, hipMemcpyHostToDevice, st));
    d.md_off = *d_md_off; d.md = *d_md;
    if (N) {
        hipLaunchKernelGGL(pf_k4_mdfill, grid, block, 0, st, d);
        MCHK(hipGetLastError());
    }
    MCHK(hipEventRecord(ev[2], st));
    MCHK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    MCHK(hipStreamSynchronize(st));
    if (err) { rc = PF_ERR_INTERNAL; goto done; }
    if (hipEventElapsedTime(&ms_len, ev[0], ev[1]) != hipSuccess ||
        hipEventElapsedTime(&ms_fill, ev[1], ev[2]) != hipSuccess) {
        (void)hipGetLastError();
        ms_len = ms_fill = 0.f;
    }
    {
        std::lock_guard<std::mutex> lk(g_md_mu);
        pf_md_stats_t &s = g_md[ctx].st;
        s.n_reads += N; s.md_bytes += md_off[N]; s.ms_len += ms_len; s.ms_fill += ms_fill;
    }
done:
    for (int i = 0; i < 3; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (d_len) (void)hipFree(d_len);
    if (d_err) (void)hipFree(d_err);
    return rc;
}

// The context's device copy of a contig's reference: uploaded once, kept until
// the context asks for another contig (or pf_ref_free / pf_ctx_destroy).
int pf_mdsynth_ref_dev(pf_ctx_t *ctx, const uint8_t *nib, uint64_t len, const uint8_t **d_ref) {
    if (!ctx || !nib || !d_ref) return PF_ERR_ARG;
    if (len >> 32) return PF_ERR_LIMIT;
    std::lock_guard<std::mutex> lk(g_md_mu);
    MdCtx &m = g_md[ctx];
    if (m.d_ref && m.h_nib == nib && m.len == len) { *d_ref = m.d_ref; return PF_OK; }
    if (hipSetDevice(pf_ctx_device(ctx)) != hipSuccess) return PF_ERR_HIP;
    if (m.d_ref) { (void)hipFree(m.d_ref); m.d_ref = nullptr; m.h_nib = nullptr; }
    const size_t bytes = (size_t)((len + 1) / 2);
    void *p = nullptr;
    if (hipMalloc(&p, bytes + 16) != hipSuccess) { (void)hipGetLastError(); return PF_ERR_NOMEM; }
    if (bytes && hipMemcpy(p, nib, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return PF_ERR_HIP; }
    m.d_ref = (uint8_t *)p; m.h_nib = nib; m.len = len;
    m.st.ref_upload_bytes += bytes;
    *d_ref = m.d_ref;
    return PF_OK;
}

static void md_ctx_drop(const pf_ctx_t *ctx, MdCtx &m) {
    if (!m.d_ref) return;
    (void)hipSetDevice(pf_ctx_device(ctx));
    (void)hipFree(m.d_ref);
    m.d_ref = nullptr; m.h_nib = nullptr; m.len = 0;
}

// pf_ctx_destroy: the context's device reference and counters go
extern "C" void pf_mdsynth_ctx_release(const pf_ctx_t *ctx) {
    std::lock_guard<std::mutex> lk(g_md_mu);
    auto it = g_md.find(ctx);
    if (it == g_md.end()) return;
    md_ctx_drop(ctx, it->second);
    g_md.erase(it);
}

// pf_ref_free: no context keeps a device copy of host nibbles that are gone
extern "C" void pf_mdsynth_forget(const uint8_t *nib) {
    std::lock_guard<std::mutex> lk(g_md_mu);
    for (auto &kv : g_md)
        if (kv.second.h_nib == nib) md_ctx_drop(kv.first, kv.second);
}

extern "C" int pf_ctx_md_stats(const pf_ctx_t *ctx, pf_md_stats_t *out) {
    if (!ctx || !out) return PF_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_md_mu);
    auto it = g_md.find(ctx);
    if (it == g_md.end()) memset(out, 0, sizeof *out);
    else *out = it->second.st;
    return PF_OK;
}

// the batch's arrays on the device (no MD) and the reference beside them
static int md_upload_batch(const pf_read_aln_batch_t *Rb, const uint8_t *ref_nib, uint64_t ref_len,
                           std::vector<void *> &al, pf_k4_reads_dev *dv, uint8_t **d_ref) {
    int rc = PF_OK;
    const uint32_t N = Rb->n_reads;
    const uint64_t ncig = Rb->cigar_off[N], nseq = Rb->seq_off[N];
    memset(dv, 0, sizeof *dv);
    MCHK(md_up(al, (uint32_t **)&dv->start, Rb->start, N));
    MCHK(md_up(al, (uint32_t **)&dv->end, Rb->end, N));
    MCHK(md_up(al, (uint64_t **)&dv->cigar_off, Rb->cigar_off, (size_t)N + 1));
    MCHK(md_up(al, (uint32_t **)&dv->cigar, Rb->cigar, ncig));
    MCHK(md_up(al, (uint64_t **)&dv->seq_off, Rb->seq_off, (size_t)N + 1));
    MCHK(md_up(al, (uint32_t **)&dv->seq_len, Rb->seq_len, N));
    MCHK(md_up(al, (uint8_t **)&dv->seq, Rb->seq, nseq, 16));
    MCHK(md_up(al, d_ref, ref_nib, (size_t)((ref_len + 1) / 2), 16));
done:
    return rc;
}

extern "C" int pf_md_synth(pf_ctx_t *ctx, const pf_read_aln_batch_t *Rb, const uint8_t *ref_nib, uint64_t ref_len,
                           uint64_t **md_off, uint8_t **md) {
    if (!ctx || !Rb || !md_off || !md || (!ref_nib && ref_len)) return PF_ERR_ARG;
    *md_off = nullptr;
    *md = nullptr;
    if (ref_len >> 32) return PF_ERR_LIMIT;
    const uint32_t N = Rb->n_reads;
    uint64_t *off = (uint64_t *)malloc(((size_t)N + 1) * 8);
    if (!off) return PF_ERR_NOMEM;
    off[0] = 0;
    if (N == 0) {
        *md = (uint8_t *)malloc(1);
        if (!*md) { free(off); return PF_ERR_NOMEM; }
        *md_off = off;
        return PF_OK;
    }
    int rc = PF_OK;
    std::vector<void *> al;
    std::vector<uint32_t> mdl;
    std::vector<uint64_t> mo;
    pf_k4_reads_dev dv;
    uint8_t *d_ref = nullptr, *d_md = nullptr, *buf = nullptr;
    uint64_t *d_mo = nullptr;
    hipStream_t st = pf_ctx_stream(ctx);
    MCHK(hipSetDevice(pf_ctx_device(ctx)));
    rc = md_upload_batch(Rb, ref_nib, ref_len, al, &dv, &d_ref);
    if (!rc) rc = pf_mdsynth_dev(ctx, st, N, dv, d_ref, ref_len, mdl, mo, al, &d_mo, &d_md);
    if (rc) goto done;
    buf = (uint8_t *)malloc(std::max<uint64_t>(mo[N], 1));
    if (!buf) { rc = PF_ERR_NOMEM; goto done; }
    if (mo[N]) MCHK(hipMemcpy(buf, d_md, mo[N], hipMemcpyDeviceToHost));
    memcpy(off, mo.data(), ((size_t)N + 1) * 8);
done:
    for (void *p : al) (void)hipFree(p);
    if (rc) { free(off); free(buf); return rc; }
    *md_off = off;
    *md = buf;
    return PF_OK;
}

extern "C" int pf_haptag_reads_ref(pf_ctx_t *ctx, const pf_known_vars_t *K, const pf_read_aln_batch_t *Rb,
                                   const uint8_t *ref_nib, uint64_t ref_len, uint8_t *hp_out) {
    if (!ctx || !K || !Rb || !hp_out || (!ref_nib && ref_len)) return PF_ERR_ARG;
    if (ref_len >> 32) return PF_ERR_LIMIT;
    const uint32_t N = Rb->n_reads;
    if (N == 0) return PF_OK;
    int rc = PF_OK;
    std::vector<void *> al;
    std::vector<uint32_t> mdl, nins(N), ncig(N);
    std::vector<uint64_t> mo;
    pf_k4_reads_dev dv;
    uint8_t *d_ref = nullptr, *d_md = nullptr;
    uint64_t *d_mo = nullptr;
    hipStream_t st = pf_ctx_stream(ctx);
    for (uint32_t r = 0; r < N; r++) {
        uint32_t n = 0;
        for (uint64_t c = Rb->cigar_off[r]; c < Rb->cigar_off[r + 1]; c++) n += (Rb->cigar[c] & 0xf) == 1;
        nins[r] = n;
        ncig[r] = (uint32_t)(Rb->cigar_off[r + 1] - Rb->cigar_off[r]);
    }
    MCHK(hipSetDevice(pf_ctx_device(ctx)));
    rc = md_upload_batch(Rb, ref_nib, ref_len, al, &dv, &d_ref);
    if (!rc) rc = pf_mdsynth_dev(ctx, st, N, dv, d_ref, ref_len, mdl, mo, al, &d_mo, &d_md);
    if (!rc) {
        dv.md_off = d_mo;
        dv.md = d_md;
        pf_k4_reads_host h{Rb->start, Rb->end, nins.data(), ncig.data(), mdl.data()};
        rc = pf_haptag_core(ctx, K, N, h, nullptr, &dv, hp_out);
    }
done:
    for (void *p : al) (void)hipFree(p);
    return rc;
}
