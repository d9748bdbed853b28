"""The permutation kernel (pf_batch_permtest) beside the pileup kernels of the
same batch: profiles/dmr_perm/README.md's numbers.

tools/dmr_prof.py's protocol: record-level synth_aln batches at 60x (seed 7) of
16 and 256 windows of 50,000 bases; per repeat the pileup (its kernels' ms) and
the permutation test (its kernel's ms) for each n_perm and each workgroup size
in turn.  3 warm-up repeats, 15 timed; median [min-max].

The shape --dmr produces is many short windows with a few dozen reads each:
--cut N also times a calls-level batch of about N windows of 1,000 bases cut
from the first windows of the largest batch.  Each 1 kb window holds the reads
of its 50 kb window that have a call inside it, whole (as the second pass of
hapmeth --dmr-perm fetches them), the calls as the device loader decoded them.

usage: python tools/dmr_perm_prof.py [--windows 16,256] [--perms 99,999,9999] [--threads 64,256,1024] [--cut 1000]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(v):
    return "%.3f [%.3f-%.3f]" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def cut_batch(db, aln, n_cut, width=1000):
    """A calls-level WindowBatch of about n_cut windows of `width` bases from
    the first windows of the record-level batch db (uploaded from aln)."""
    from pomfret_amd.abi import WindowBatch
    off, pos, cat, _, _ = db.debug_calls()
    rec = db.read_recs()
    off = off.astype(np.int64)
    hp = aln.hp[rec]
    win = np.searchsorted(aln.win_rec_off.astype(np.int64), rec, side="right") - 1
    has = off[1:] > off[:-1]
    lo = np.where(has, pos[np.minimum(off[:-1], max(pos.size - 1, 0))], 0).astype(np.int64)
    hi = np.where(has, pos[np.maximum(off[1:] - 1, 0)], 0).astype(np.int64)
    ws, we, wro, rhp, slices = [], [], [0], [], []
    for w in range(aln.n_windows):
        if len(ws) >= n_cut:
            break
        reads = np.flatnonzero((win == w) & has)
        for s in range(int(aln.win_start[w]), int(aln.win_end[w]), width):
            e = min(s + width, int(aln.win_end[w]))
            for r in reads[(lo[reads] < e) & (hi[reads] >= s)]:
                if np.any((pos[off[r]:off[r + 1]] >= s) & (pos[off[r]:off[r + 1]] < e)):
                    rhp.append(hp[r])
                    slices.append((off[r], off[r + 1]))
            ws.append(s)
            we.append(e)
            wro.append(len(rhp))
    co = np.concatenate([[0], np.cumsum([b - a for a, b in slices])]).astype(np.uint64)
    cp = np.concatenate([pos[a:b] for a, b in slices]) if slices else np.zeros(0, np.uint32)
    cc = np.concatenate([cat[a:b] for a, b in slices]) if slices else np.zeros(0, np.uint8)
    R = len(rhp)
    return WindowBatch(win_start=ws, win_end=we, win_read_off=wro, read_start=np.zeros(R), read_end=np.ones(R),
                       read_hp=rhp, read_call_off=co, call_pos=cp, call_cat=cc)


def time_batch(db, name, extra, perms, threads, warmup, steps):
    pile_ms = []
    ker = {(p, t): [] for p in perms for t in threads}
    first = {}
    for it in range(warmup + steps):
        pile = db.pileup()
        if it >= warmup:
            pile_ms.append(pile["ms"])
        for p in perms:
            for t in threads:
                os.environ["PF_PERM_THREADS"] = str(t)
                res = db.permtest(p, seed=1)
                if p in first:                       # the result does not depend on the workgroup
                    assert all(np.array_equal(res[k], first[p][k]) for k in ("hits", "status", "n_reads", "sum"))
                first.setdefault(p, res)
                if it >= warmup:
                    ker[(p, t)].append(res["ms"])
    os.environ.pop("PF_PERM_THREADS", None)
    r = first[perms[0]]
    n = r["n_reads"].sum(axis=1)
    print(json.dumps(dict(batch=name, **extra, windows=int(n.size), tested=int((r["status"] == 0).sum()),
                          untested=int((r["status"] == 1).sum()), over_limit=int((r["status"] == 2).sum()),
                          reads_per_window="%d [%d-%d]" % (int(np.median(n)), int(n.min()), int(n.max())),
                          calls_in_range=int(r["sum"].sum()), pileup_ms=stat(pile_ms),
                          perm_ms={"%d perms, %d threads" % k: stat(v) for k, v in ker.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--perms", default="99,999,9999")
    ap.add_argument("--threads", default="64,256,1024")
    ap.add_argument("--cut", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--lib", default=None, help="another build of the library, a .so in pomfret_amd/")
    a = ap.parse_args()
    if a.lib:
        import pomfret_amd._lib as L
        L.LIB_PATH = os.path.join(os.path.dirname(L.LIB_PATH), a.lib)
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    perms = [int(x) for x in a.perms.split(",")]
    threads = [int(x) for x in a.threads.split(",")]
    cfg = Config.from_coverage(60, given=True)
    ctx = Context(0)
    sizes = [int(x) for x in a.windows.split(",")]
    for n in sizes:
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        time_batch(db, "50 kb windows", dict(records=int(aln.n_recs)), perms, threads, a.warmup, a.steps)
        if a.cut and n == max(sizes):
            cb = cut_batch(db, aln, a.cut)
            db.free()
            db = ctx.upload(cfg, cb)
            time_batch(db, "1 kb windows", dict(reads=int(cb.n_reads), calls=int(cb.call_pos.size)), perms, threads,
                       a.warmup, a.steps)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
