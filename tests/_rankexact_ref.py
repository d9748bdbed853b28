"""The exact rank test's literal reference (include/pomfret_amd.h,
pf_batch_rankexact), shared by the exact rank tests, in Python integers.
brute() is the definition: every subset of the counted reads of haplotype 1's
size, u2 of each by comparing all pairs across the split.  dp() is the counting
identity the kernel uses: u2(A) = sum of r_i over A - |A|^2 with r_i = 2 * #{f_j
< f_i} + #{f_j == f_i}, counted as subset sums for the smaller class.
tests/test_rankexact.py pins dp to brute; the device tests compare with dp.
Test infrastructure, no GPU."""
import itertools
from math import comb

import numpy as np

from tests._perm_ref import participating
from tests._rank_ref import bh_ref, rank_ref, rank_text

MAX_READS = 64                                   # PF_RANK_EXACT_MAX_READS
KEYS = ("n_reads", "n_short", "u2", "total", "le", "ge", "two", "status")
HEAD_EXTRA = "\texact_p\tbest_p\tbest_q"


def _cmp(a, b):
    """The order of two fractions (m, n) by cross-multiplication: -1, 0, 1."""
    x, y = a[0] * b[1], b[0] * a[1]
    return (x > y) - (x < y)


def _u2(f, inside):
    """u2(A) of the definition, A the reads with inside[i]."""
    g = e = 0
    for i in range(len(f)):
        for j in range(len(f)):
            if inside[i] and not inside[j]:
                c = _cmp(f[i], f[j])
                g += c > 0
                e += c == 0
    return 2 * g + e


def _counts(dist, u0, a12):
    """(total, le, ge, two) of {u2 value: subsets} against the observed u0."""
    total = sum(dist.values())
    le = sum(c for v, c in dist.items() if v <= u0)
    ge = sum(c for v, c in dist.items() if v >= u0)
    two = sum(c for v, c in dist.items() if abs(v - a12) >= abs(u0 - a12))
    return total, le, ge, two


def brute(f, tags):
    """f: the counted reads' (m_i, n_i), tags: 0 / 1.  (u2(A0), total, le, ge,
    two) by enumeration."""
    n, n1 = len(f), tags.count(0)
    u0 = _u2(f, [t == 0 for t in tags])
    dist = {}
    for A in itertools.combinations(range(n), n1):
        inside = [False] * n
        for i in A:
            inside[i] = True
        v = _u2(f, inside)
        dist[v] = dist.get(v, 0) + 1
    return (u0,) + _counts(dist, u0, n1 * (n - n1))


def dp(f, tags):
    """The same five integers by the subset-sum identity, for the smaller class."""
    n, n1 = len(f), tags.count(0)
    n2 = n - n1
    r = [2 * sum(_cmp(f[j], f[i]) < 0 for j in range(n)) + sum(_cmp(f[j], f[i]) == 0 for j in range(n)) for i in range(n)]
    small = 0 if n1 <= n2 else 1
    k = min(n1, n2)
    ways = [dict() for _ in range(k + 1)]
    ways[0][0] = 1
    for i in range(n):
        for c in range(min(i + 1, k), 0, -1):
            for s, cnt in ways[c - 1].items():
                ways[c][s + r[i]] = ways[c].get(s + r[i], 0) + cnt
    v0 = sum(x for x, t in zip(r, tags) if t == small) - k * k
    dist = {s - k * k: c for s, c in ways[k].items()}
    assert all(0 <= v <= 2 * n1 * n2 for v in dist)
    total, le, ge, two = _counts(dist, v0, n1 * n2)
    if small == 1:                               # u2(A) = 2 n1 n2 - v(complement)
        return 2 * n1 * n2 - v0, total, ge, le, two
    return v0, total, le, ge, two


def rankexact_ref(m, u, tags, min_calls, max_reads=MAX_READS):
    """One window from its participating reads, as rank_ref takes them:
    dict(n_reads [2], n_short [2], u2, total, le, ge, two, status).  n_reads,
    n_short and u2 are rank_ref's."""
    base = rank_ref(m, u, tags, min_calls)
    f = [(int(a), int(a + b)) for a, b in zip(m, u) if a + b >= min_calls]
    t = [int(x) for (a, b, x) in zip(m, u, tags) if a + b >= min_calls]
    out = dict(n_reads=base["n_reads"], n_short=base["n_short"], u2=base["u2"], total=0, le=0, ge=0, two=0, status=0)
    if len(f) > max_reads:
        out["status"] = 2
    elif 0 in base["n_reads"]:
        out["status"] = 1
    else:
        u0, out["total"], out["le"], out["ge"], out["two"] = dp(f, t)
        assert u0 == base["u2"] and out["total"] == comb(len(f), base["n_reads"][0])
    return out


def rankexact_ref_batch(batch, min_calls, max_reads=MAX_READS, hp=None):
    """DeviceBatch.rankexact's arrays for a WindowBatch."""
    W = batch.n_windows
    out = dict(n_reads=np.zeros((W, 2), np.uint32), n_short=np.zeros((W, 2), np.uint32), status=np.zeros(W, np.uint32))
    out.update({k: np.zeros(W, np.uint64) for k in ("u2", "total", "le", "ge", "two")})
    for w in range(W):
        r = rankexact_ref(*participating(batch, w, hp), min_calls, max_reads)
        for k in KEYS:
            out[k][w] = r[k]
    return out


def same(got, ref, tag=""):
    for k in KEYS:
        g, r = np.asarray(got[k], np.uint64), np.asarray(ref[k], np.uint64)
        assert g.shape == r.shape and np.array_equal(g, r), f"{tag}: {k} {g.tolist()[:8]} vs {r.tolist()[:8]}"


def rank_exact_text(recs, bh):
    """{prefix}.hapmeth.rank.tsv under --dmr-rank-exact: rank_text's lines
    (records as there) and exact_p, best_p, best_q from each record's two,
    total and exact_status.  exact_p is two / total of two doubles."""
    from pomfret_amd import rank_p
    base = rank_text(recs, bh).splitlines()
    exact = [float(r["two"]) / float(r["total"]) if int(r["exact_status"]) == 0 else None for r in recs]
    best = [x if x is not None else rank_p(int(r["u2"]), int(r["n_reads"][0]), int(r["n_reads"][1]), int(r["ties"]))[2]
            if int(r["status"]) == 0 else None for r, x in zip(recs, exact)]
    q = bh_ref([1.0 if b is None else b for b in best], [b is not None for b in best])
    lines = [base[0] + HEAD_EXTRA]
    for line, x, b, qq in zip(base[1:], exact, best, q):
        lines.append(line + "\t" + ("." if x is None else "%.6g" % x) + "\t" + ("." if b is None else "%.6g" % b) + "\t" +
                     ("." if b is None or not bh else "%.6g" % qq))
    return "".join(x + "\n" for x in lines)
