"""The rank kernel (pf_batch_ranktest) beside the permutation kernel at 999
permutations on the same batches: profiles/rank/README.md's numbers.

tools/dmr_perm_prof.py's protocol and batches: record-level synth_aln batches
at 60x (seed 7) of 16 and 256 windows of 50,000 bases, and a calls-level batch
of about --cut windows of 1,000 bases cut from the largest one (the shape
--dmr produces).  Per repeat the rank test for each workgroup size, narrow
(the kernel's choice) and forced wide (PF_RANK_WIDE=1), and the permutation
test at its default workgroup; event-timed, in one process.  3 warm-up
repeats, 15 timed; median [min-max].

--null N also prints, from the CPU reference alone, the rate of p < 0.05 over
N null regions of 30 + 30 reads of 5-40 calls (DESIGN.md §3 Permutation test's
null regions).

usage: python tools/rank_prof.py [--windows 16,256] [--threads 64,256,1024] [--cut 1000] [--perm 999] [--null 300]
                                 [--lib libpomfret_amd_variant.so]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEYS = ("n_reads", "n_short", "cls", "sum", "u2", "ties", "status")


def stat(v):
    return "%.3f [%.3f-%.3f]" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def time_batch(db, name, extra, threads, n_perm, min_calls, warmup, steps):
    ker = {(t, w): [] for t in threads for w in (0, 1)}
    perm_ms = []
    first = None
    for it in range(warmup + steps):
        for t in threads:
            for w in (0, 1):
                os.environ["PF_RANK_THREADS"] = str(t)
                os.environ["PF_RANK_WIDE"] = str(w)
                res = db.ranktest(min_calls)
                if first is not None:                # neither the workgroup nor the product width reaches the result
                    assert all(np.array_equal(res[k], first[k]) for k in KEYS)
                first = first or res
                if it >= warmup:
                    ker[(t, w)].append(res["ms"])
        pm = db.permtest(n_perm, seed=1)
        if it >= warmup:
            perm_ms.append(pm["ms"])
    os.environ.pop("PF_RANK_THREADS", None)
    os.environ.pop("PF_RANK_WIDE", None)
    n = first["n_reads"].sum(axis=1)
    print(json.dumps(dict(batch=name, **extra, windows=int(n.size), tested=int((first["status"] == 0).sum()),
                          untested=int((first["status"] == 1).sum()), over_limit=int((first["status"] == 2).sum()),
                          counted_reads_per_window="%d [%d-%d]" % (int(np.median(n)), int(n.min()), int(n.max())),
                          short_reads=int(first["n_short"].sum()),
                          rank_ms={"%d threads, %s" % (t, "wide" if w else "narrow"): stat(v) for (t, w), v in ker.items()},
                          perm_ms={"%d perms, 256 threads" % n_perm: stat(perm_ms)})), flush=True)


def null_rate(n_cases, seed=1):
    """The rate of p < 0.05 on null regions, from the literal reference and pf_rank_p (no GPU)."""
    from pomfret_amd import rank_p
    from tests._rank_ref import rank_ref
    rng = np.random.default_rng(seed)
    ps = []
    for _ in range(n_cases):
        n = rng.integers(5, 41, 60)
        level = rng.random()                          # one level for both haplotypes: the null
        m = rng.binomial(n, level)
        r = rank_ref(m.tolist(), (n - m).tolist(), [0] * 30 + [1] * 30, 3)
        ps.append(rank_p(r["u2"], 30, 30, r["ties"])[2])
    ps = np.array(ps)
    print(json.dumps(dict(null_cases=n_cases, p_below_0_05="%.1f %%" % (100.0 * float((ps < 0.05).mean())),
                          mean_p="%.3f" % float(ps.mean()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--threads", default="64,256,1024")
    ap.add_argument("--cut", type=int, default=1000)
    ap.add_argument("--perm", type=int, default=999)
    ap.add_argument("--min-calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--null", type=int, default=0)
    ap.add_argument("--lib", default=None, help="another build of the library, a .so in pomfret_amd/ (an unroll variant)")
    a = ap.parse_args()
    if a.lib:
        import pomfret_amd._lib as L
        L.LIB_PATH = os.path.join(os.path.dirname(L.LIB_PATH), a.lib)
    if a.null:
        null_rate(a.null)
    sizes = [int(x) for x in a.windows.split(",") if x]
    if not sizes:
        return
    from dmr_perm_prof import cut_batch
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    threads = [int(x) for x in a.threads.split(",")]
    cfg = Config.from_coverage(60, given=True)
    ctx = Context(0)
    for n in sizes:
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        time_batch(db, "50 kb windows", dict(records=int(aln.n_recs)), threads, a.perm, a.min_calls, a.warmup, a.steps)
        if a.cut and n == max(sizes):
            cb = cut_batch(db, aln, a.cut)
            db.free()
            db = ctx.upload(cfg, cb)
            time_batch(db, "1 kb windows", dict(reads=int(cb.n_reads), calls=int(cb.call_pos.size)), threads, a.perm,
                       a.min_calls, a.warmup, a.steps)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
