"""The assign kernels (pf_batch_assign) beside the pileup kernels of the same
batch: profiles/assign/README.md's numbers.

tools/dmr_perm_prof.py's protocol and batches: record-level synth_aln at 60x
(seed 7) of 16 and 256 windows of 50,000 bases, and (--cut N) the calls-level
batch of about N windows of 1,000 bases cut from the largest one, the shape the
second pass of hapmeth --assign produces.  Per repeat the pileup (its kernels'
ms) and the assignment (its two kernels' ms; the site table's pileup kernels
are outside them) for each tile in turn.  3 warm-up repeats, 15 timed; median
[min-max].

usage: python tools/assign_prof.py [--windows 16,256] [--tiles 4096,64] [--cut 1000] [--min-cov 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.dmr_perm_prof import cut_batch, stat  # noqa: E402


def time_batch(db, name, extra, tiles, cfg, warmup, steps):
    pile_ms, ker, first = [], {t: [] for t in tiles}, None
    for it in range(warmup + steps):
        pile = db.pileup()
        if it >= warmup:
            pile_ms.append(pile["ms"])
        for t in tiles:
            os.environ["PF_ASSIGN_TILE"] = str(t)
            res = db.assign(cfg)
            if first is not None:                    # the result does not depend on the tile
                assert all(np.array_equal(res[k], first[k]) for k in ("n_used", "llr", "hp", "win_n"))
            first = first or res
            if it >= warmup:
                ker[t].append(res["ms"])
    os.environ.pop("PF_ASSIGN_TILE", None)
    sites = np.diff(pile["win_off"].astype(np.int64))
    c = pile["cnt"].astype(np.int64)
    inf = int(((c[:, 0].sum(axis=1) >= cfg.min_cov) & (c[:, 1].sum(axis=1) >= cfg.min_cov)).sum())
    reads = np.diff(first["win_read_off"].astype(np.int64))
    print(json.dumps(dict(batch=name, **extra, windows=int(reads.size),
                          reads_per_window="%d [%d-%d]" % (int(np.median(reads)), int(reads.min()), int(reads.max())),
                          sites_per_window="%d [%d-%d]" % (int(np.median(sites)), int(sites.min()), int(sites.max())),
                          informative_sites=inf, scored=int(first["win_n"][:, 0].sum()),
                          assigned=int(first["win_n"][:, 1:].sum()),
                          entries_used=int(first["n_used"].sum()), pileup_ms=stat(pile_ms),
                          assign_ms={"tile %d" % t: stat(v) for t, v in ker.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--tiles", default="4096,64")
    ap.add_argument("--cut", type=int, default=1000)
    ap.add_argument("--min-cov", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--lib", default=None, help="another build of the library, a .so in pomfret_amd/")
    a = ap.parse_args()
    if a.lib:
        import pomfret_amd._lib as L
        L.LIB_PATH = os.path.join(os.path.dirname(L.LIB_PATH), a.lib)
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.abi import AssignConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    tiles = [int(x) for x in a.tiles.split(",")]
    acfg = AssignConfig(min_cov=a.min_cov)
    cfg = Config.from_coverage(60, given=True)
    ctx = Context(0)
    sizes = [int(x) for x in a.windows.split(",")]
    for n in sizes:
        print(f"[assign_prof] {n} windows: generating", file=sys.stderr, flush=True)
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        time_batch(db, "50 kb windows", dict(records=int(aln.n_recs)), tiles, acfg, a.warmup, a.steps)
        if a.cut and n == max(sizes):
            cb = cut_batch(db, aln, a.cut)
            db.free()
            db = ctx.upload(cfg, cb)
            time_batch(db, "1 kb windows", dict(reads=int(cb.n_reads), calls=int(cb.call_pos.size)), tiles, acfg,
                       a.warmup, a.steps)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
