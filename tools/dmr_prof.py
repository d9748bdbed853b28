"""The region kernels (pf_dmr_regions) beside the pileup kernels of the same
run: profiles/dmr/README.md's numbers.

Record-level synth_aln batches at 60x (seed 7) of 16 and 256 windows; per
repeat the pileup (its kernels' ms), then the region call on its CSR for each
block size in turn (its kernels' ms and the host time of the 28 B/site upload).
3 warm-up repeats, 15 timed; median [min-max].

usage: python tools/dmr_prof.py [--lib libpomfret_amd_variant.so] [--blocks 256,512,1024] [--windows 16,256]
                                [--dmr min_cov,min_delta_pct,max_gap,min_sites]

The synthetic reads carry no allele-specific methylation, so the default
parameters find no run on them and the emit pass is not launched; --dmr
3,50,1000,1 finds runs (and times all three kernels).

Blocks above the build's PF_DMR_BLOCK need a variant build:
    make -C pomfret_amd/csrc variant V=dmr4096 VFLAGS=-DPF_DMR_BLOCK=4096"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pomfret_amd._lib as L  # noqa: E402


def stat(v):
    return "%.3f [%.3f-%.3f]" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--blocks", default="256,512,1024")
    ap.add_argument("--windows", default="16,256")
    ap.add_argument("--dmr", default="5,40,500,5")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.join(os.path.dirname(L.LIB_PATH), a.lib)
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.abi import DmrConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    blocks = [int(x) for x in a.blocks.split(",")]
    cfg, dcfg = Config.from_coverage(60, given=True), DmrConfig(*[int(x) for x in a.dmr.split(",")])
    ctx = Context(0)
    for n in [int(x) for x in a.windows.split(",")]:
        aln = make_aln_batch(AlnSpec(n_windows=n, coverage=60, seed=7), workers=min(16, n))
        db = ctx.upload_aln(cfg, aln, LoadConfig())
        pile_ms, ker, up = [], {b: [] for b in blocks}, {b: [] for b in blocks}
        first = None
        for it in range(a.warmup + a.steps):
            pile = db.pileup()
            res = {b: ctx.dmr_regions(pile, dcfg, block=b) for b in blocks}
            for b in blocks[1:]:
                assert all(np.array_equal(res[b][k], res[blocks[0]][k]) for k in ("start", "end", "n_sites", "sum", "open"))
            if it >= a.warmup:
                pile_ms.append(pile["ms"])
                for b in blocks:
                    ker[b].append(res[b]["ms"])
                    up[b].append(res[b]["ms_upload"])
            first = res[blocks[0]]
        kept = int((first["n_sites"] >= dcfg.min_sites).sum())
        print(json.dumps(dict(dmr=a.dmr, windows=n, records=int(aln.n_recs), sites=int(pile["pos"].size),
                              informative=first["n_informative"], runs_returned=int(first["start"].size),
                              regions=kept, longest=int(first["n_sites"].max()) if first["start"].size else 0,
                              pileup_ms=stat(pile_ms),
                              dmr_ms={b: stat(ker[b]) for b in blocks}, upload_ms={b: stat(up[b]) for b in blocks})),
              flush=True)
        db.free()
    ctx.close()


if __name__ == "__main__":
    main()
