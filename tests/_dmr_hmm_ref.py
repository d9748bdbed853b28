"""The hidden Markov model's literal reference (include/pomfret_amd.h,
pf_dmr_hmm_regions), shared by the HMM tests: plain Python ints, one loop per
chain, the tie rules as the header writes them.  Test infrastructure, no GPU."""
import bisect

import numpy as np

from tests._assign_ref import ilog2_q16 as L

CLAMP = 1 << 28
KEYS = ("start", "end", "n_sites", "sign", "sum", "open")


def evidence(m1, u1, m2, u2):
    """e of an informative site."""
    n1, n2 = m1 + u1, m2 + u2
    m, u, n = m1 + m2, u1 + u2, n1 + n2
    sep = (m1 * (L(m1 + 1) - L(n1 + 2)) + u1 * (L(u1 + 1) - L(n1 + 2)) +
           m2 * (L(m2 + 1) - L(n2 + 2)) + u2 * (L(u2 + 1) - L(n2 + 2)))
    pool = m * (L(m + 1) - L(n + 2)) + u * (L(u + 1) - L(n + 2))
    g = min(max(sep - pool, 0), CLAMP)
    d = m1 * n2 - m2 * n1
    return g if d > 0 else (-g if d < 0 else 0)


def _viterbi(es, site_cost, switch):
    """The states of one chain's sites."""
    em = [(0, e - site_cost, -e - site_cost) for e in es]
    V = [list(em[0])]
    bp = [None]
    for i in range(1, len(es)):
        v, b = [], []
        for s in range(3):
            cand = [V[-1][r] - (switch if r != s else 0) for r in range(3)]
            best = max(cand)
            b.append(s if cand[s] == best else cand.index(best))
            v.append(em[i][s] + best)
        V.append(v)
        bp.append(b)
    x = [0] * len(es)
    x[-1] = V[-1].index(max(V[-1]))
    for i in range(len(es) - 1, 0, -1):
        x[i - 1] = bp[i][x[i]]
    return x


def kept(run, cfg):
    """min_sites and the pooled-delta rule."""
    M1, U1, M2, U2 = run["sum"]
    N1, N2 = M1 + U1, M2 + U2
    return run["n_sites"] >= cfg.min_sites and run["sign"] * (M1 * N2 - M2 * N1) * 100 >= cfg.min_delta_pct * N1 * N2


def hmm_ref(pos, cnt, cfg, hcfg, breaks=()):
    """Context.dmr_hmm_regions(..., sites=True) for the sites (pos [n], cnt
    [n, 6] or [n, 3, 2]): the kept runs as arrays, n_informative, n_chains,
    state, evidence; plus "all", every run before the two filters."""
    site_cost, switch = int(round(hcfg.site_cost * 65536)), int(round(hcfg.switch * 65536))
    brk = sorted(int(x) for x in breaks)
    pos = np.asarray(pos).tolist()
    cnt = np.asarray(cnt).reshape(-1, 6).tolist()
    n = len(pos)
    state, evid = [255] * n, [0] * n
    chains, cur = [], None                                   # lists of site indices
    for i in range(n):
        m1, u1, m2, u2 = cnt[i][:4]
        if m1 + u1 < cfg.min_cov or m2 + u2 < cfg.min_cov:
            continue
        evid[i] = evidence(m1, u1, m2, u2)
        joined = False
        if cur is not None and pos[i] - pos[cur[-1]] <= cfg.max_gap:
            k = bisect.bisect_right(brk, pos[cur[-1]])       # the first break above the previous site
            joined = not (k < len(brk) and brk[k] <= pos[i])
        if joined:
            cur.append(i)
        else:
            cur = [i]
            chains.append(cur)
    runs = []
    for ch in chains:
        xs = _viterbi([evid[i] for i in ch], site_cost, switch)
        run = None
        for i, x in zip(ch, xs):
            state[i] = x
            if run is not None and x != run["x"]:
                runs.append(run)
                run = None
            if x == 0:
                continue
            if run is None:
                run = dict(x=x, start=pos[i], end=pos[i] + 1, n_sites=0, sign=1 if x == 1 else -1, sum=[0, 0, 0, 0], open=0)
            run["end"] = pos[i] + 1
            run["n_sites"] += 1
            run["sum"] = [a + b for a, b in zip(run["sum"], cnt[i][:4])]
        if run is not None:
            runs.append(run)
    keep = [r for r in runs if kept(r, cfg)]
    k = len(keep)
    return dict(start=np.array([r["start"] for r in keep], np.uint32), end=np.array([r["end"] for r in keep], np.uint32),
                n_sites=np.array([r["n_sites"] for r in keep], np.uint32), sign=np.array([r["sign"] for r in keep], np.int32),
                sum=np.array([r["sum"] for r in keep], np.uint64).reshape(k, 4), open=np.zeros(k, np.uint32),
                n_informative=sum(len(c) for c in chains), n_chains=len(chains), state=np.array(state, np.uint8),
                evidence=np.array(evid, np.int64), all=runs, kept=keep)


def same(got, ref, what=""):
    for k in KEYS + ("state", "evidence"):
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and np.array_equal(g, r), (what, k, g[:8], r[:8])
    assert got["n_informative"] == ref["n_informative"] and got["n_chains"] == ref["n_chains"], what
