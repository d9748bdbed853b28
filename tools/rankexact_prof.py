"""The exact rank kernel (pf_batch_rankexact) beside the rank kernel
(pf_batch_ranktest) on the same batches: profiles/rank_exact/README.md's
numbers.

tools/rank_prof.py's protocol and batches: record-level synth_aln batches at
60x (seed 7) of 16 and 256 windows of 50,000 bases (every window holds more
than 64 counted reads: the kernel's cost where it only declines), a calls-level
batch of about --cut windows of 1,000 bases cut from the largest one (the shape
--dmr produces), and one made for this kernel: --worst windows of 32 + 32
counted reads without ties, the largest table there is.  Per repeat the exact
test for each workgroup size with the kernel's own placement, once more at the
largest workgroup with every table in the slab (PF_RANKX_HBM=1), and the rank
test; event-timed, in one process.  3 warm-up repeats, 15 timed; median
[min-max].

usage: python tools/rankexact_prof.py [--windows 16,256] [--threads 64,256,1024] [--cut 1000] [--worst 512]
                                      [--max-reads 64] [--lib libpomfret_amd_variant.so]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEYS = ("n_reads", "n_short", "u2", "total", "le", "ge", "two", "status")


def stat(v):
    return "%.3f [%.3f-%.3f]" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def cells(n, k):
    """The table of n counted reads, k in the smaller class, in cells of 8 bytes."""
    return sum(2 * c * (n - c) + 1 for c in range(k + 1))


def time_batch(db, name, extra, threads, min_calls, max_reads, warmup, steps):
    ker = {(t, h): [] for t in threads for h in (0,)}
    ker[(max(threads), 1)] = []
    rank_ms = []
    first = None
    for it in range(warmup + steps):
        for t, h in ker:
            os.environ["PF_RANKX_THREADS"] = str(t)
            os.environ["PF_RANKX_HBM"] = str(h)
            res = db.rankexact(min_calls, max_reads)
            if first is not None:                    # neither the workgroup nor the placement reaches the result
                assert all(np.array_equal(res[k], first[k]) for k in KEYS)
            first = first or res
            if it >= warmup:
                ker[(t, h)].append(res["ms"])
        rk = db.ranktest(min_calls)
        assert np.array_equal(rk["u2"], first["u2"]) and np.array_equal(rk["n_reads"], first["n_reads"])
        if it >= warmup:
            rank_ms.append(rk["ms"])
    os.environ.pop("PF_RANKX_THREADS", None)
    os.environ.pop("PF_RANKX_HBM", None)
    n = first["n_reads"].sum(axis=1)
    tested = first["status"] == 0
    size = np.array([cells(int(a + b), int(min(a, b))) for a, b in first["n_reads"][tested]])
    print(json.dumps(dict(batch=name, **extra, windows=int(n.size), tested=int(tested.sum()),
                          untested=int((first["status"] == 1).sum()), over_limit=int((first["status"] == 2).sum()),
                          counted_reads_per_window="%d [%d-%d]" % (int(np.median(n)), int(n.min()), int(n.max())),
                          tables_in_lds=int((size <= 8113).sum()), tables_in_slab=int((size > 8113).sum()),
                          table_updates=int(sum(int(a + b) * int(s) for (a, b), s in zip(first["n_reads"][tested], size))),
                          exact_ms={"%d threads, %s" % (t, "all in the slab" if h else "own placement"): stat(v)
                                    for (t, h), v in ker.items()},
                          rank_ms={"256 threads": stat(rank_ms)})), flush=True)


def worst_batch(n_windows, seed=3232):
    """Calls-level: every window 32 + 32 reads of 70 calls with distinct meth counts."""
    from pomfret_amd.abi import WindowBatch
    rng = np.random.default_rng(seed)
    ws, we, wro, hp, co, cp, cc = [], [], [0], [], [0], [], []
    for w in range(n_windows):
        s = 1000 * w
        ws.append(s)
        we.append(s + 1000)
        m = rng.permutation(71)[:64]
        tags = rng.permutation([0] * 32 + [1] * 32)
        for a, t in zip(m.tolist(), tags.tolist()):
            hp.append(t)
            cp.extend(range(s + 10, s + 10 + 70))
            cc.extend([0] * a + [1] * (70 - a))
            co.append(len(cp))
        wro.append(len(hp))
    R = len(hp)
    return WindowBatch(win_start=ws, win_end=we, win_read_off=wro, read_start=np.zeros(R), read_end=np.ones(R), read_hp=hp,
                       read_call_off=co, call_pos=cp, call_cat=cc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--threads", default="64,256,1024")
    ap.add_argument("--cut", type=int, default=1000)
    ap.add_argument("--worst", type=int, default=512)
    ap.add_argument("--min-calls", type=int, default=3)
    ap.add_argument("--max-reads", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--lib", default=None, help="another build of the library, a .so in pomfret_amd/")
    a = ap.parse_args()
    if a.lib:
        import pomfret_amd._lib as L
        L.LIB_PATH = os.path.join(os.path.dirname(L.LIB_PATH), a.lib)
    from dmr_perm_prof import cut_batch
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    threads = [int(x) for x in a.threads.split(",")]
    sizes = [int(x) for x in a.windows.split(",") if x]
    cfg = Config.from_coverage(60, given=True)
    ctx = Context(0)
    args = (threads, a.min_calls, a.max_reads, a.warmup, a.steps)
    for n in sizes:
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        time_batch(db, "50 kb windows", dict(records=int(aln.n_recs)), *args)
        if a.cut and n == max(sizes):
            cb = cut_batch(db, aln, a.cut)
            db.free()
            db = ctx.upload(cfg, cb)
            time_batch(db, "1 kb windows", dict(reads=int(cb.n_reads), calls=int(cb.call_pos.size)), *args)
        db.free()
    if a.worst:
        wb = worst_batch(a.worst)
        db = ctx.upload(cfg, wb)
        time_batch(db, "32 + 32 reads", dict(reads=int(wb.n_reads), calls=int(wb.call_pos.size)), *args)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
