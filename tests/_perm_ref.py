"""The permutation test's literal reference (include/pomfret_amd.h,
pf_batch_permtest), shared by the permutation tests: Python ints carry the
128-bit products.  Test infrastructure, no GPU."""
import numpy as np

MAX_READS = 4096                                 # PF_PERM_MAX_READS


def mix(x):  # x: int, uint32 semantics
    x &= 0xFFFFFFFF; x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF
    x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF; return x ^ (x >> 16)


def perm_ref(ws, we, m, u, hp, n_perm, seed):      # participating reads only, read order
    n, n1 = len(m), sum(h == 0 for h in hp); Mt, Nt = sum(m), sum(m) + sum(u)
    def stat(lab):
        M0 = sum(a for a, l in zip(m, lab) if l == 0); N0 = sum(a + b for a, b, l in zip(m, u, lab) if l == 0)
        return abs(M0 * Nt - Mt * N0), N0 * (Nt - N0)
    A0, D0 = stat(hp)
    if n1 in (0, n) or D0 == 0: return 0, 1
    base = mix(seed ^ mix(ws ^ mix(we))); hits = 0
    for b in range(n_perm):
        kb = mix(base + b); order = sorted(range(n), key=lambda i: (mix(kb ^ i), i))
        lab = [1] * n
        for i in order[:n1]: lab[i] = 0
        A, D = stat(lab); hits += D > 0 and A * D0 >= A0 * D
    return hits, 0


def participating(batch, w, hp=None):
    """(m, u, tags) of window w's participating reads of a WindowBatch, in
    read order: tag 0 or 1 and at least one cat 0 / 1 entry inside the window."""
    hp = np.asarray(batch.read_hp if hp is None else hp, np.uint8)
    ws, we = int(batch.win_start[w]), int(batch.win_end[w])
    m, u, tags = [], [], []
    for r in range(int(batch.win_read_off[w]), int(batch.win_read_off[w + 1])):
        if hp[r] > 1:
            continue
        c0, c1 = int(batch.read_call_off[r]), int(batch.read_call_off[r + 1])
        p, c = np.asarray(batch.call_pos[c0:c1], np.int64), np.asarray(batch.call_cat[c0:c1])
        inside = (p >= ws) & (p < we)
        mm, uu = int((inside & (c == 0)).sum()), int((inside & (c == 1)).sum())
        if mm + uu:
            m.append(mm); u.append(uu); tags.append(int(hp[r]))
    return m, u, tags


def perm_ref_batch(batch, n_perm, seed, hp=None):
    """DeviceBatch.permtest's arrays for a WindowBatch, from perm_ref."""
    W = batch.n_windows
    out = dict(n_reads=np.zeros((W, 2), np.uint32), sum=np.zeros((W, 4), np.uint64), hits=np.zeros(W, np.uint32),
               status=np.zeros(W, np.uint32))
    for w in range(W):
        m, u, tags = participating(batch, w, hp)
        out["n_reads"][w] = [tags.count(0), tags.count(1)]
        out["sum"][w] = [sum(a for a, t in zip(m, tags) if t == k) if j == 0 else sum(b for b, t in zip(u, tags) if t == k)
                         for k in (0, 1) for j in (0, 1)]
        if len(m) > MAX_READS:
            out["status"][w] = 2
            continue
        out["hits"][w], out["status"][w] = perm_ref(int(batch.win_start[w]), int(batch.win_end[w]), m, u, tags, n_perm, seed)
    return out


def same(got, ref, tag=""):
    for k in ("n_reads", "sum", "hits", "status"):
        assert np.array_equal(np.asarray(got[k], np.uint64), np.asarray(ref[k], np.uint64)), \
            f"{tag}: {k} {np.asarray(got[k]).tolist()[:8]} vs {np.asarray(ref[k]).tolist()[:8]}"
