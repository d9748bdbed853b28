"""The literal references of the given-regions feature (include/pomfret_amd.h:
pf_region_sums, pf_bh_adjust, pf_write_regions), shared by the region tests:
plain Python ints and floats, one loop over regions and sites.  Test
infrastructure, no GPU."""
import functools
import math

import numpy as np

from tests._dmr_hmm_ref import evidence

FIELDS = ("n_cpg", "n_sites", "n_pos", "n_neg", "sum", "evidence")
INT32_MAX = 2 ** 31 - 1
MAX_TEST_SPAN = 1_000_000
HEADER = ("#chrom\tstart\tend\tname\tn_cpg\tn_sites\tn_h1gt\tn_h2gt\tdir\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta"
          "\tpooled_p\tllr_bits\tblock")
PERM_COLUMNS = "\treads_h1\treads_h2\tperm_p\tperm_q"


@functools.lru_cache(maxsize=None)
def _site(m1, u1, m2, u2, min_cov, min_delta_pct):
    """None for a transparent site, else (sign, e)."""
    n1, n2 = m1 + u1, m2 + u2
    if n1 < min_cov or n2 < min_cov:
        return None
    d, t = (m1 * n2 - m2 * n1) * 100, min_delta_pct * n1 * n2
    return (1 if d >= t else (-1 if -d >= t else 0)), evidence(m1, u1, m2, u2)


def region_ref(pos, cnt, cfg, starts, ends):
    """Context.region_sums for the sites (pos [n], cnt [n, 6] or [n, 3, 2]) and
    the regions [starts[i], ends[i]): every region walks every site."""
    pos = np.asarray(pos).tolist()
    cnt = np.asarray(cnt).reshape(-1, 6).tolist()
    sites = [_site(c[0], c[1], c[2], c[3], cfg.min_cov, cfg.min_delta_pct) for c in cnt]
    out = []
    for s, e in zip(np.asarray(starts).tolist(), np.asarray(ends).tolist()):
        r = dict(n_cpg=0, n_sites=0, n_pos=0, n_neg=0, sum=[0, 0, 0, 0], evidence=0)
        for i, p in enumerate(pos):
            if not s <= p < e:
                continue
            r["n_cpg"] += 1
            if sites[i] is None:
                continue
            sign, ev = sites[i]
            r["n_sites"] += 1
            r["n_pos"] += sign == 1
            r["n_neg"] += sign == -1
            r["sum"] = [a + b for a, b in zip(r["sum"], cnt[i][:4])]
            r["evidence"] += ev
        out.append(r)
    return arrays(out, sum(x is not None for x in sites))


def arrays(recs, n_informative):
    n = len(recs)
    return dict(n_cpg=np.array([r["n_cpg"] for r in recs], np.uint32), n_sites=np.array([r["n_sites"] for r in recs], np.uint32),
                n_pos=np.array([r["n_pos"] for r in recs], np.uint32), n_neg=np.array([r["n_neg"] for r in recs], np.uint32),
                sum=np.array([r["sum"] for r in recs], np.uint64).reshape(n, 4),
                evidence=np.array([r["evidence"] for r in recs], np.int64), n_informative=n_informative)


def add(a, b):
    """The records of the same regions over two disjoint site ranges, added."""
    return dict({k: a[k] + b[k] for k in FIELDS}, n_informative=a["n_informative"] + b["n_informative"])


def same(got, ref, what=""):
    for k in FIELDS:
        assert np.array_equal(got[k], ref[k]), (what, k, got[k][:8], ref[k][:8])
    assert got["n_informative"] == ref["n_informative"], what


def bh_ref(hits, tested, n_perm):
    """pf_bh_adjust: the operations of the header, in its order, in doubles."""
    idx = [i for i, t in enumerate(tested) if t]
    m = len(idx)
    val = {}
    for j in idx:
        p = (hits[j] + 1.0) / (n_perm + 1.0)
        rank = sum(1 for k in idx if hits[k] <= hits[j])
        val[j] = (p * float(m)) / float(rank)
    q = [math.nan] * len(hits)
    for i in idx:
        q[i] = min(1.0, min(val[j] for j in idx if hits[j] >= hits[i]))
    return q


def block_of(start, end, breaks):
    return "split" if any(start < x < end for x in breaks) else "ok"


def pooled_p(s):
    from pomfret_amd import fisher_exact
    return None if max(s) > INT32_MAX else fisher_exact(*s)[3]


def eligible(rec, cfg, max_p, breaks=()):
    """Whether the second pass takes the region (rec: start, end, n_sites, sum)."""
    p = pooled_p(rec["sum"])
    return (block_of(rec["start"], rec["end"], breaks) == "ok" and rec["n_sites"] >= cfg.min_sites and p is not None and
            p <= max_p and 0 < rec["end"] - rec["start"] <= MAX_TEST_SPAN)


def regions_text(recs, perm=None, n_perm=0, breaks=None):
    """{prefix}.hapmeth.regions.bed.  recs: dicts of chrom, start, end, name and
    the FIELDS, in file order.  perm: None, or per record None (not eligible)
    or (reads_h1, reads_h2, hits, status); perm_q is over all records.  breaks:
    {chrom: positions}."""
    lines = [HEADER + (PERM_COLUMNS if perm is not None else "") + "\n"]
    q = None
    if perm is not None:
        tested = [t is not None and t[3] == 0 for t in perm]
        q = bh_ref([t[2] if t is not None else 0 for t in perm], tested, n_perm)
    for k, r in enumerate(recs):
        M1, U1, M2, U2 = (int(x) for x in r["sum"])
        N1, N2 = M1 + U1, M2 + U2
        lhs, rhs = M1 * N2, M2 * N1
        delta = (M1 / N1 if N1 else 0.0) - (M2 / N2 if N2 else 0.0)
        p = pooled_p((M1, U1, M2, U2))
        line = "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%.4f\t%s\t%.3f\t%s" % (
            r["chrom"], r["start"], r["end"], r["name"], r["n_cpg"], r["n_sites"], r["n_pos"], r["n_neg"],
            "h1>h2" if lhs > rhs else ("h1<h2" if lhs < rhs else "."), M1, U1, M2, U2, delta,
            "." if p is None else "%.6g" % p, int(r["evidence"]) / 65536.0,
            block_of(r["start"], r["end"], (breaks or {}).get(r["chrom"], ())))
        if perm is not None:
            t = perm[k]
            if t is None:
                line += "\t.\t.\t.\t."
            elif t[3] != 0:
                line += "\t%d\t%d\t.\t." % (t[0], t[1])
            else:
                line += "\t%d\t%d\t%.6g\t%.6g" % (t[0], t[1], (t[2] + 1.0) / (n_perm + 1.0), q[k])
        lines.append(line + "\n")
    return "".join(lines)
