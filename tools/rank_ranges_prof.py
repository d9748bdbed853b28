"""The range kernel (pf_batch_rankranges: pf_rank_ranges) on
tile-shaped batches: profiles/rank_ranges/README.md's numbers.

tools/rank_prof.py's protocol and batches: record-level synth_aln batches at
60x (seed 7) of 16 and 256 windows of 50,000 bases.  Every window is cut into
tiles of T bases, the ranges of one call.  Per repeat, for each T: the call at
each workgroup size (PF_RANK_THREADS) with the LDS array sized to the batch,
the call at 64 threads with the fixed 32 KB array
(PF_RANKR_LDS_FIXED=1), and the pileup of the same batch for context;
event-timed, in one process.  3 warm-up repeats, 15 timed; median [min-max].

The baseline is pf_rank_test on a calls-level batch of about --cut windows of
1,000 bases cut from the first windows of the largest batch
(tools/dmr_perm_prof.py's cut_batch: one window per tile, every read with a
call in the tile, its whole slice), beside the range call on the same tiles
alone (the other windows get no range).  --lib names another build of the
library (make variant V=name VFLAGS=...).

usage: python tools/rank_ranges_prof.py [--windows 16,256] [--tiles 1000,5000] [--threads 64,256,1024] [--cut 1000]
                                        [--lib libpomfret_amd_name.so]
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


def tiles_of(ws, we, T, n_windows=None):
    """(off, starts, ends): window w in tiles of T bases; windows from n_windows on get none."""
    off, s, e = [0], [], []
    for w, (a, b) in enumerate(zip(ws.tolist(), we.tolist())):
        if n_windows is None or w < n_windows:
            for x in range(a, b, T):
                s.append(x)
                e.append(min(x + T, b))
        off.append(len(s))
    return np.array(off, np.uint64), np.array(s, np.uint32), np.array(e, np.uint32)


def time_ranges(db, aln, name, tiles, threads, min_calls, warmup, steps, n_windows=None):
    for T in tiles:
        rng = tiles_of(aln.win_start, aln.win_end, T, n_windows)
        ker = {t: [] for t in threads}
        fixed, pile_ms = [], []
        first = None
        for it in range(warmup + steps):
            for t in threads:
                os.environ["PF_RANK_THREADS"] = str(t)
                res = db.rankranges(*rng, min_calls=min_calls)
                if first is not None:                    # the workgroup size does not reach the result
                    assert all(np.array_equal(res[k], first[k]) for k in KEYS)
                first = first or res
                if it >= warmup:
                    ker[t].append(res["ms"])
            os.environ["PF_RANK_THREADS"] = "64"             # the size at which the first record was taken
            os.environ["PF_RANKR_LDS_FIXED"] = "1"
            res = db.rankranges(*rng, min_calls=min_calls)
            os.environ.pop("PF_RANKR_LDS_FIXED", None)
            os.environ.pop("PF_RANK_THREADS", None)
            assert all(np.array_equal(res[k], first[k]) for k in KEYS)
            pile = db.pileup()
            if it >= warmup:
                fixed.append(res["ms"])
                pile_ms.append(pile["ms"])
        n = first["n_reads"].sum(axis=1)
        print(json.dumps(dict(batch=name, tile=T, ranges=int(n.size), tested=int((first["status"] == 0).sum()),
                              counted_reads_per_range="%d [%d-%d]" % (int(np.median(n)), int(n.min()), int(n.max())),
                              ranges_ms={"%d threads" % t: stat(v) for t, v in ker.items()},
                              ranges_ms_fixed_32k_lds=stat(fixed), pileup_ms=stat(pile_ms))), flush=True)


def time_baseline(db, name, threads, min_calls, warmup, steps):
    ker = {t: [] for t in threads}
    first = None
    for it in range(warmup + steps):
        for t in threads:
            os.environ["PF_RANK_THREADS"] = str(t)
            res = db.ranktest(min_calls)
            first = first or res
            if it >= warmup:
                ker[t].append(res["ms"])
    os.environ.pop("PF_RANK_THREADS", None)
    n = first["n_reads"].sum(axis=1)
    print(json.dumps(dict(batch=name, windows=int(n.size), tested=int((first["status"] == 0).sum()),
                          counted_reads_per_window="%d [%d-%d]" % (int(np.median(n)), int(n.min()), int(n.max())),
                          rank_test_ms={"%d threads" % t: stat(v) for t, v in ker.items()})), flush=True)
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--tiles", default="1000,5000")
    ap.add_argument("--threads", default="64,256,1024")
    ap.add_argument("--cut", type=int, default=1000)
    ap.add_argument("--min-calls", type=int, default=3)
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
    sizes = [int(x) for x in a.windows.split(",") if x]
    tiles = [int(x) for x in a.tiles.split(",") if x]
    threads = [int(x) for x in a.threads.split(",")]
    cfg = Config.from_coverage(60, given=True)
    ctx = Context(0)
    for n in sizes:
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        time_ranges(db, aln, "%d windows of 50 kb, %d records" % (n, int(aln.n_recs)), tiles, threads, a.min_calls, a.warmup,
                    a.steps)
        if a.cut and n == max(sizes):
            cb = cut_batch(db, aln, a.cut)
            k = int(np.searchsorted(aln.win_start, int(cb.win_start[-1]), side="right"))     # the windows the cut took
            time_ranges(db, aln, "the first %d of them alone" % k, [1000], threads, a.min_calls, a.warmup, a.steps, k)
            same = db.rankranges(*tiles_of(aln.win_start, aln.win_end, 1000, k), min_calls=a.min_calls)
            db.free()
            db = ctx.upload(cfg, cb)
            base = time_baseline(db, "their tiles as %d windows of 1 kb (calls level, %d reads, %d calls)"
                                 % (cb.n_windows, int(cb.n_reads), int(cb.call_pos.size)), threads, a.min_calls, a.warmup,
                                 a.steps)
            print(json.dumps(dict(both_routes_same_integers=all(np.array_equal(base[key], same[key]) for key in KEYS))),
                  flush=True)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
