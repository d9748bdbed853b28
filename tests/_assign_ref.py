"""The tag assignment's literal reference (include/pomfret_amd.h,
pf_batch_assign), shared by the assign tests: plain Python ints, one loop per
window.  Test infrastructure, no GPU."""
import numpy as np

HEADER = "#qname\tchrom\tstart\tend\tn_calls\tllr\thp\n"


def ilog2_q16(x):
    """L(x), x >= 1: the header's algorithm, not libm."""
    e = x.bit_length() - 1
    y = x << (31 - e)
    f = 0
    for _ in range(16):
        y = (y * y) >> 31
        f <<= 1
        if y >= 1 << 32:
            y >>= 1
            f |= 1
    return (e << 16) | f


def weights(m1, u1, m2, u2):
    """(wM, wU) of an informative site."""
    n1, n2 = m1 + u1, m2 + u2
    L = ilog2_q16
    return (L(m1 + 1) - L(n1 + 2) - L(m2 + 1) + L(n2 + 2), L(u1 + 1) - L(n1 + 2) - L(u2 + 1) + L(n2 + 2))


def assign_ref_batch(batch, min_cov, min_calls, min_llr_q16, hp=None):
    """DeviceBatch.assign's arrays for a WindowBatch."""
    hp = np.asarray(batch.read_hp if hp is None else hp, np.uint8)
    W, R = batch.n_windows, batch.n_reads
    assert hp.size == R
    pos, cat, off = np.asarray(batch.call_pos).tolist(), np.asarray(batch.call_cat).tolist(), np.asarray(batch.read_call_off).tolist()
    n_used, llr, new = [0] * R, [0] * R, hp.tolist()
    win_n = np.zeros((W, 3), np.uint32)
    for w in range(W):
        ws, we = int(batch.win_start[w]), int(batch.win_end[w])
        r0, r1 = int(batch.win_read_off[w]), int(batch.win_read_off[w + 1])
        cnt = {}                                         # pos -> [m1, u1, m2, u2]
        for r in range(r0, r1):
            if hp[r] > 1:
                continue
            for c in range(off[r], off[r + 1]):
                if ws <= pos[c] < we and cat[c] < 2:
                    cnt.setdefault(pos[c], [0, 0, 0, 0])[2 * int(hp[r]) + cat[c]] += 1
        wt = {p: weights(*c) for p, c in cnt.items() if c[0] + c[1] >= min_cov and c[2] + c[3] >= min_cov}
        for r in range(r0, r1):
            if hp[r] != 254:
                continue
            S = n = 0
            for c in range(off[r], off[r + 1]):
                if ws <= pos[c] < we and cat[c] < 2 and pos[c] in wt:
                    S += wt[pos[c]][cat[c]]
                    n += 1
            n_used[r], llr[r] = n, S
            if n >= min_calls and S >= min_llr_q16 and S > 0:
                new[r] = 0
            elif n >= min_calls and -S >= min_llr_q16 and S < 0:
                new[r] = 1
            win_n[w] += [n >= 1, new[r] == 0, new[r] == 1]
    return dict(win_read_off=np.asarray(batch.win_read_off, np.uint32), n_used=np.asarray(n_used, np.uint32),
                llr=np.asarray(llr, np.int64), hp=np.asarray(new, np.uint8), win_n=win_n)


def same(got, ref, tag=""):
    for k in ("win_read_off", "n_used", "llr", "hp", "win_n"):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and np.array_equal(g.astype(np.int64), r.astype(np.int64)), \
            f"{tag}: {k} differs at {np.flatnonzero(g.ravel() != r.ravel())[:8].tolist() if g.shape == r.shape else g.shape}"


def assign_lines(res, chrom, win_start, win_end, qname_of_read):
    """pf_write_assign's lines (no header) of an assign dict."""
    out = []
    for w in range(len(win_start)):
        for r in range(int(res["win_read_off"][w]), int(res["win_read_off"][w + 1])):
            if int(res["n_used"][r]) >= 1:
                h = int(res["hp"][r])
                out.append("%s\t%s\t%d\t%d\t%d\t%.4f\t%s\n" % (qname_of_read[r], chrom, win_start[w], win_end[w],
                                                              int(res["n_used"][r]), int(res["llr"][r]) / 65536.0,
                                                              "1" if h == 0 else "2" if h == 1 else "."))
    return out
