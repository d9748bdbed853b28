"""The rank test's literal reference (include/pomfret_amd.h, pf_batch_ranktest),
shared by the rank tests: Python ints, every pair compared by
cross-multiplication, ties counted with fractions.Fraction.  Past 300 counted
reads the same definition runs as a numpy int64 cross-multiplication (the
products there stay far below 2^63).  Test infrastructure, no GPU."""
import math
from collections import Counter
from fractions import Fraction

import numpy as np

from tests._perm_ref import participating

MAX_READS = 4096                                 # PF_RANK_MAX_READS
KEYS = ("n_reads", "n_short", "cls", "sum", "u2", "ties", "status")
HEAD = ("#chrom\tstart\tend\treads_h1\treads_h2\tshort_h1\tshort_h2\tallmeth_h1\tallunmeth_h1\tmixed_h1\tallmeth_h2"
        "\tallunmeth_h2\tmixed_h2\tauc\tz\trank_p\trank_q\n")


def rank_ref(m, u, tags, min_calls):
    """One window from its participating reads (m_i, u_i, tag_i), read order:
    dict(n_reads [2], n_short [2], cls [2][3], sum [4], u2, ties, status)."""
    n_short, n_reads, cls, sm = [0, 0], [0, 0], [[0, 0, 0], [0, 0, 0]], [0, 0, 0, 0]
    cm, cn, ct = [], [], []
    for a, b, t in zip(m, u, tags):
        assert t in (0, 1) and a + b >= 1
        if a + b < min_calls:
            n_short[t] += 1
            continue
        n_reads[t] += 1
        cls[t][0 if b == 0 else 1 if a == 0 else 2] += 1
        sm[2 * t] += a
        sm[2 * t + 1] += b
        cm.append(int(a)); cn.append(int(a + b)); ct.append(t)
    out = dict(n_reads=n_reads, n_short=n_short, cls=cls, sum=sm, u2=0, ties=0, status=0)
    if len(cm) > MAX_READS:
        out["status"] = 2
    elif n_reads[0] == 0 or n_reads[1] == 0:
        out["status"] = 1
    elif len(cm) > 300:
        M, N, T = np.array(cm, np.int64), np.array(cn, np.int64), np.array(ct)
        assert int(M.max()) * int(N.max()) < 2 ** 62
        lhs, rhs = M[:, None] * N[None, :], M[None, :] * N[:, None]      # f_i > f_j iff lhs > rhs
        cross = (T[:, None] == 0) & (T[None, :] == 1)
        eq = lhs == rhs
        e = eq.sum(axis=1).astype(object)
        out["u2"] = 2 * int(((lhs > rhs) & cross).sum()) + int((eq & cross).sum())
        out["ties"] = int(sum(int(x) * int(x) - 1 for x in e))
    else:
        G = E = 0
        for i in range(len(cm)):
            for j in range(len(cm)):
                if ct[i] == 0 and ct[j] == 1:
                    G += cm[i] * cn[j] > cm[j] * cn[i]
                    E += cm[i] * cn[j] == cm[j] * cn[i]
        out["u2"] = 2 * G + E
        out["ties"] = sum(t ** 3 - t for t in Counter(Fraction(a, b) for a, b in zip(cm, cn)).values())
    return out


def rank_ref_batch(batch, min_calls, hp=None):
    """DeviceBatch.ranktest's arrays for a WindowBatch, from rank_ref."""
    W = batch.n_windows
    out = dict(n_reads=np.zeros((W, 2), np.uint32), n_short=np.zeros((W, 2), np.uint32), cls=np.zeros((W, 2, 3), np.uint32),
               sum=np.zeros((W, 4), np.uint64), u2=np.zeros(W, np.uint64), ties=np.zeros(W, np.uint64),
               status=np.zeros(W, np.uint32))
    for w in range(W):
        r = rank_ref(*participating(batch, w, hp), min_calls)
        for k in KEYS:
            out[k][w] = r[k]
    return out


def same(got, ref, tag=""):
    for k in KEYS:
        g, r = np.asarray(got[k], np.uint64), np.asarray(ref[k], np.uint64)
        assert g.shape == r.shape and np.array_equal(g, r), f"{tag}: {k} {g.tolist()[:8]} vs {r.tolist()[:8]}"


def rank_p_ref(u2, n1, n2, ties):
    """pf_rank_p's steps as a Python loop would take them: (auc, z, p)."""
    a = float(n1) * float(n2)
    n = float(n1) + float(n2)
    u = float(u2)
    auc = u / (2.0 * a)
    var = (a / 12.0) * ((n + 1.0) - float(ties) / (n * (n - 1.0)))
    if var <= 0.0:
        return auc, 0.0, 1.0
    d = max(abs(u - a) / 2.0 - 0.5, 0.0)
    z = d / math.sqrt(var)
    return auc, z, min(1.0, math.erfc(z / math.sqrt(2.0)))


def bh_ref(p, tested):
    """pf_bh_adjust_p as a Python loop: sorted by (p, index), a group of equal p
    shares its last member's rank, the running minimum from the top, capped."""
    q = [float("nan")] * len(p)
    v = sorted((float(p[i]), i) for i in range(len(p)) if tested[i])
    m, b, run = len(v), len(v), None
    while b > 0:
        a = b - 1
        while a > 0 and v[a - 1][0] == v[b - 1][0]:
            a -= 1
        x = (v[a][0] * float(m)) / float(b)
        run = x if run is None or x < run else run
        for j in range(a, b):
            q[v[j][1]] = run if run < 1.0 else 1.0
        b = a
    return q


def rank_text(recs, bh):
    """{prefix}.hapmeth.rank.tsv from records (chrom, start, end and rank_ref's
    dict): the p-values by pomfret_amd.rank_p, the library's host function,
    which tests/test_ranktest.py pins to scipy; the q-values by bh_ref."""
    from pomfret_amd import rank_p
    tested = [int(r["status"]) == 0 for r in recs]
    st = [rank_p(int(r["u2"]), int(r["n_reads"][0]), int(r["n_reads"][1]), int(r["ties"])) if t else None
          for r, t in zip(recs, tested)]
    q = bh_ref([s[2] if s else 1.0 for s in st], tested)
    lines = []
    for r, s, qq in zip(recs, st, q):
        ints = [int(r["start"]), int(r["end"]), *np.asarray(r["n_reads"]).ravel().tolist(),
                *np.asarray(r["n_short"]).ravel().tolist(), *np.asarray(r["cls"]).ravel().tolist()]
        tail = "\t.\t.\t.\t." if s is None else "\t%.4f\t%.3f\t%.6g\t%s" % (s[0], s[1], s[2], "%.6g" % qq if bh else ".")
        lines.append(r["chrom"] + "".join("\t%d" % x for x in ints) + tail + "\n")
    return HEAD + "".join(lines)
