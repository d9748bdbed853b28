"""Generates tests/golden/k3_paths_budget_sweep.json: the greedy path
(DeviceBatch.k3_paths) of every problem at every point of
tests._cases.k3_budget_sweep, recorded on a GPU with the library of the commit
before K3's placement refactor.  A pin of k3_run's path decision (NOT an
oracle output): regenerate it only with a change that means to move problems
between paths."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pomfret_amd import Context  # noqa: E402
from tests._cases import k3_budget_sweep  # noqa: E402

SWEEP_ENV = ("PF_K3_LDS", "PF_K3_LDS_FB", "PF_K3_CACHE", "PF_K3_GCNT")

if __name__ == "__main__":
    ctx = Context(0)
    out, seen = {}, set()
    for tag, cfg, batch, env in k3_budget_sweep():
        for k in SWEEP_ENV:                      # the library reads them at upload
            os.environ.pop(k, None)
        os.environ.update(env)
        db = ctx.upload(cfg, batch)
        db.run()
        out[tag] = db.k3_paths().tolist()
        seen |= {p for row in out[tag] for p in row}
        db.free()
    ctx.close()
    missing = {1, 2, 3, 4, 6} - seen
    assert not missing, f"the sweep never takes path(s) {sorted(missing)}: add budget points"
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "k3_paths_budget_sweep.json"), "w") as f:
        f.write("{\n" + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in out.items()) + "\n}\n")
    print("wrote", len(out), "points; codes seen", sorted(seen))
