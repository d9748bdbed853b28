"""The given-regions kernels (pf_region_sums) beside the region kernels
(pf_dmr_regions) of the same batch: profiles/regions/README.md's numbers.

Record-level synth_aln batches at 60x (seed 7) of 16 and 256 windows; per
repeat the pileup, then pf_dmr_regions on its CSR (default parameters), then
pf_region_sums on the same CSR for each region list and block in turn: its
kernels' ms and the host time of the upload (28 B per site and 8 B per region).
The lists: N regions drawn at random over the sites' span, 200 to 20,000 bases
long (heavily overlapping at 100,000), and N regions that tile the span
(disjoint).  3 warm-up repeats, 15 timed; median [min-max].  Every block's
records are compared with the first block's in every repeat.

usage: python tools/regions_prof.py [--windows 16,256] [--regions 1000,100000] [--blocks 1024,256,512]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(v):
    return "%.3f [%.3f-%.3f]" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def lists(pos, n, rng):
    lo, hi = int(pos.min()), int(pos.max()) + 1
    s = rng.integers(lo, hi, n)
    random = (s, np.minimum(s + rng.integers(200, 20_000, n), 2 ** 32 - 1))
    edges = np.linspace(lo, hi, n + 1).astype(np.int64)
    return dict(random=random, tiled=(edges[:-1], edges[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--regions", default="1000,100000")
    ap.add_argument("--blocks", default="1024,256,512")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--lib", default=None, help="another build of the library, a .so in pomfret_amd/")
    a = ap.parse_args()
    if a.lib:
        import pomfret_amd._lib as L
        L.LIB_PATH = os.path.join(os.path.dirname(L.LIB_PATH), a.lib)
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.abi import DmrConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    blocks = [int(x) for x in a.blocks.split(",")]
    cfg, dcfg = Config.from_coverage(60, given=True), DmrConfig()
    ctx = Context(0)
    for n in [int(x) for x in a.windows.split(",")]:
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        pile = db.pileup()
        rng = np.random.default_rng(9)
        cases = {(k, kind): v for k in [int(x) for x in a.regions.split(",")] for kind, v in lists(pile["pos"], k, rng).items()}
        pile_ms, dmr_ms, dmr_up = [], [], []
        ker = {(c, b): [] for c in cases for b in blocks}
        up = {(c, b): [] for c in cases for b in blocks}
        info = {}
        for it in range(a.warmup + a.steps):
            pile = db.pileup()
            d = ctx.dmr_regions(pile, dcfg)
            res = {(c, b): ctx.region_sums(pile, dcfg, *cases[c], block=b) for c in cases for b in blocks}
            for c in cases:
                for b in blocks[1:]:
                    assert all(np.array_equal(res[(c, b)][k], res[(c, blocks[0])][k])
                               for k in ("n_cpg", "n_sites", "n_pos", "n_neg", "sum", "evidence"))
                info[c] = dict(mean_cpg=float(res[(c, blocks[0])]["n_cpg"].mean()), n_informative=res[(c, blocks[0])]["n_informative"])
            if it >= a.warmup:
                pile_ms.append(pile["ms"])
                dmr_ms.append(d["ms"])
                dmr_up.append(d["ms_upload"])
                for key, r in res.items():
                    ker[key].append(r["ms"])
                    up[key].append(r["ms_upload"])
        print(json.dumps(dict(windows=n, records=int(aln.n_recs), sites=int(pile["pos"].size), pileup_ms=stat(pile_ms),
                              dmr_ms=stat(dmr_ms), dmr_upload_ms=stat(dmr_up),
                              region_sums=[dict(regions=c[0], kind=c[1], block=b, ms=stat(ker[(c, b)]), upload_ms=stat(up[(c, b)]),
                                                upload_share="%.2f" % (float(np.median(up[(c, b)])) /
                                                                       (float(np.median(up[(c, b)])) + float(np.median(ker[(c, b)])))),
                                                **info[c]) for c in cases for b in blocks])), flush=True)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
