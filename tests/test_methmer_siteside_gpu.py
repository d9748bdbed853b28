"""The methylation characters of a read by a search from the site side
(k2_stage_calls + k2_chars_site, pf_kernels.hip) against the oracle on small
hand-built windows: every read's methmer keys in both directions, the site
arrays, then the window results.

A read of up to 512 calls is staged in its wave's LDS buffer, one word (pos <<
2) | cat per call in call order, and every site of the read's range takes the
lower bound of its position over those words; a read of 513 calls reads its
calls from HBM (k2_chars).  The windows are those of
tests/test_methmer_pair_gpu.py: 30 tagged reads left of the gap, two carrier
reads that call every site position methylated / unmethylated (with
cov_for_selection = 1 exactly these positions are sites) and the case's own
reads, whose calls off the sites are methylated or category 2, so they create
no site.  Each case asserts from the oracle's own site arrays (`_model`) that
its input contains the situation it names.

"A read whose range holds PF_K12_CAP sites" cannot reach the search: a read
stays in the fused kernel only when its bound, (#sites in [F, L]) + 3k + 4, is
<= PF_K12_CAP, and its range is smaller than the bound
(tests/test_methmer_pair_gpu.py has the arithmetic).  test_cap has the read
whose bound is exactly PF_K12_CAP, the largest the search sees, and the read
with one site more, which takes the fallback kernel, at the default of 512 and
at a PF_K12_CAP lowered by the environment.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_methmer_pair_gpu import BASE, _batch, _cfg, _grid, _model, _window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
CFG = _cfg(K, 5000)
SEG = 524_288                                     # positions per bitmap segment of K12's fast path


def _compare(oracle_lib, ctx, cfg, b, tag):
    """Site arrays, methmers of every read in both directions and the window results against the
    oracle; returns the K12 paths and the chunk items of the run."""
    db = ctx.upload(cfg, b)
    try:
        ro = b.win_read_off
        for d in (0, 1):
            n, st, keys = db.debug_methmers(d)
            k0 = 0
            for w in range(b.n_windows):
                for o, g, what in zip(oracle_lib.window_sites(cfg, b, w, d), db.debug_sites(w, d, cap=1 << 12),
                                      ("sites", "starts", "lens")):
                    assert np.array_equal(o, g), f"{tag} w{w} d{d} {what}"
                on, ost, okeys = oracle_lib.window_methmers(cfg, b, w, d)
                gn = n[ro[w]:ro[w + 1]]
                assert np.array_equal(on, gn), f"{tag} w{w} d{d} mmr_n {np.argwhere(on != gn)[:3].tolist()}"
                assert np.array_equal(ost, st[ro[w]:ro[w + 1]]), f"{tag} w{w} d{d} mmr_start"
                gk = keys[k0:k0 + len(okeys)]
                assert np.array_equal(okeys, gk), f"{tag} w{w} d{d} keys {np.argwhere(okeys != gk)[:3].tolist()}"
                k0 += len(okeys)
            assert k0 == len(keys), f"{tag} d{d} key count"
        ref = oracle_lib.methphase(cfg, b, n_threads=4)
        out = db.run()
        for name in ("decision", "dir_table", "dir_join", "dir_which_way", "win_n_sites", "win_n_reads", "read_hp"):
            assert np.array_equal(getattr(ref, name), getattr(out, name)), f"{tag}: {name}"
        np.testing.assert_allclose(out.dir_fisher_p, ref.dir_fisher_p, rtol=1e-6, atol=0, err_msg=tag)
        np.testing.assert_allclose(out.dir_score, ref.dir_score, rtol=1e-6, atol=0, err_msg=tag)
        return db.k12_paths().copy(), db.k12_chunk_items()
    finally:
        db.free()


def _union(x):
    """Size of the union of a read's two real-index ranges (what the characters are built over), 0: none."""
    q = [d["q"] for d in x["dirs"] if d]
    return max(b for _, b in q) - min(a for a, _ in q) if q else 0


# ---------------------------------------------------------------------------
# the cases: name -> (windows, check(models)); a window is (sites, reads)
CALL_COUNTS = (1, 63, 64, 65, 511, 512, 513)


def _case_call_counts():
    """Reads of 1 .. 513 calls on a grid 10 apart, call i at BASE + 10 i.  Sites: the first call, the
    last call of every read and the two calls on each side of every 64-call slot boundary."""
    idx = sorted({0} | {n - 1 for n in CALL_COUNTS} | {64 * m - 1 for m in range(1, 9)} | {64 * m for m in range(1, 9)})
    sites = [BASE + 10 * i for i in idx]
    reads = []
    for n in CALL_COUNTS:
        for flip in (0, 1):
            reads.append([(BASE + 10 * i, (i + flip) & 1 if i in idx else 0) for i in range(n)])

    def check(ms):
        m = ms[0]
        assert list(m["sp"]) == sites
        R = m["reads"][32:]
        assert [x["ncalls"] for x in R[::2]] == list(CALL_COUNTS)
        for x in R:
            n = x["ncalls"]
            on = [i for i in range(n) if x["pos"][i] in m["sp"]]
            assert on[0] == 0 and on[-1] == n - 1
            for e in range(64, n, 64):
                assert e - 1 in on and e in on
    return [(sites, reads)], check


def _case_site_kinds():
    """At site X = sites[5] a read has: no call; a category-2 call; two calls of categories (0, 1),
    (1, 2), (0, 2); a call one position below and one above and none on it.  Every read also calls the
    sites around X."""
    sites = _grid(12)
    X = sites[5]
    around = [(sites[3], 0), (sites[4], 1), (sites[6], 0), (sites[7], 1)]
    at_x = [[], [(X, 2)], [(X, 0), (X, 1)], [(X, 1), (X, 2)], [(X, 0), (X, 2)], [(X - 1, 0), (X + 1, 0)],
            [(X - 1, 0), (X, 1), (X + 1, 0)]]
    reads = [sorted(around + a) for a in at_x]

    def check(ms):
        m = ms[0]
        assert list(m["sp"]) == sites
        for x in m["reads"][32:]:
            assert x["dirs"][0] and x["dirs"][0]["xl"] <= 5 < x["dirs"][0]["xr"]
    return [(sites, reads)], check


def _case_range_sizes():
    """Reads whose characters span 1, 64 and 65 sites (one round of 64 lanes, its last lane, the
    first lane of a second round), among every span from 1 to 70."""
    sites = _grid(80, step=20)
    reads = []
    for n in range(1, 72):
        for i0 in (0, 7):
            reads.append([(sites[i], (i + n) & 1) for i in range(i0, i0 + n)] + [(sites[i0 + n - 1] + 5, 0)])

    def check(ms):
        sizes = {_union(x) for x in ms[0]["reads"][32:]}
        assert {1, 64, 65} <= sizes, sorted(sizes)
    return [(sites, reads)], check


def _case_one_direction():
    """A read with sites in range in direction 0 only (its calls lie right of the last direction-1
    start): k2_pair turns it down and it takes the two k2_core calls."""
    sites = _grid(12)
    reads = [[(sites[-1] - 50, 0), (sites[-1], 0)], [(sites[-1] - 50, 0), (sites[-1], 1)],
             [(sites[2], 0), (sites[4], 1), (sites[9], 0)]]

    def check(ms):
        R = ms[0]["reads"][32:]
        for x in R[:2]:
            assert x["dirs"][0] is not None and x["dirs"][1] is None
        assert R[2]["dirs"][0] and R[2]["dirs"][1]
    return [(sites, reads)], check


def _case_two_segments():
    """A window whose calls span more than 524,288 positions (two bitmap segments): reads on both
    sides of the segment boundary and one across it."""
    sites = _grid(12) + [BASE + SEG - 10, BASE + SEG + 40, BASE + 600_000, BASE + 600_100]
    reads = [[(sites[2], 0), (sites[4], 1), (sites[9], 0)],
             [(sites[11], 1), (sites[12], 0), (sites[13], 1)],
             [(sites[13], 0), (sites[14], 1), (sites[15], 0)],
             [(sites[0] - 7, 0), (sites[5], 1), (sites[5], 2), (sites[14], 0), (sites[15] + 3, 0)]]

    def check(ms):
        assert list(ms[0]["sp"]) == sites
    return [(sites, reads)], check


CASES = {"call_counts": _case_call_counts, "site_kinds": _case_site_kinds, "range_sizes": _case_range_sizes,
         "one_direction": _case_one_direction, "two_segments": _case_two_segments}


def _run_case(oracle_lib, ctx, name):
    windows, check = CASES[name]()
    b = _batch([_window(s, r) for s, r in windows])
    check([_model(oracle_lib, CFG, b, w) for w in range(b.n_windows)])
    return _compare(oracle_lib, ctx, CFG, b, name)


@pytest.mark.parametrize("name", list(CASES))
def test_case(oracle_lib, gpu_ctx, name):
    paths, items = _run_case(oracle_lib, gpu_ctx, name)
    assert items == 0                                   # no window of these is heavy: K12's own methmer phase
    assert paths[0] == (2 if name == "two_segments" else 1)


def _cap_batch(oracle_lib, cap):
    """Reads over cnt sites of a grid for cnt around cap - (3k + 4): the bound of the middle one is
    exactly cap."""
    c0 = cap - (3 * K + 4)
    sites = _grid(c0 + 8, step=20)
    reads = [[(sites[i], (i + cnt) & 1) for i in range(2, 2 + cnt)] for cnt in (c0 - 1, c0, c0 + 1, c0 + 2)]
    b = _batch([_window(sites, reads)])
    m = _model(oracle_lib, CFG, b, 0)
    bounds = []
    for x in m["reads"][32:]:
        cnt = int(np.searchsorted(m["sp"], x["L"], "right") - np.searchsorted(m["sp"], x["F"], "left"))
        bounds.append(cnt + 3 * K + 4)
    assert bounds == [cap - 1, cap, cap + 1, cap + 2]
    return b


@pytest.mark.parametrize("cap", [512, 100, 77])
def test_cap(oracle_lib, gpu_ctx, monkeypatch, cap):
    """The read whose bound is PF_K12_CAP (the most sites the search sees for one read) and the read
    with one site more (the fallback kernel), at the default and with PF_K12_CAP lowered."""
    if cap != 512:
        monkeypatch.setenv("PF_K12_CAP", str(cap))
    _compare(oracle_lib, gpu_ctx, CFG, _cap_batch(oracle_lib, cap), f"cap{cap}")


def _child():
    """Every case, and the lowered cap, in this process's environment; prints one line per case."""
    import oracle
    from pomfret_amd import Context
    oracle.build()
    ctx = Context(0)
    for name in CASES:
        paths, items = _run_case(oracle, ctx, name)
        print("CASE", name, int(paths[0]), items, flush=True)
    os.environ["PF_K12_CAP"] = "100"
    _, items = _compare(oracle, ctx, CFG, _cap_batch(oracle, 100), "cap100")
    print("CASE", "cap100", 1, items, flush=True)
    ctx.close()


def test_through_chunks():
    """The same cases with PF_K12C_MINR=1, which hands every window's methmer phase to
    pf_k12_chunks, in a fresh process: the chunk route was taken (K12 handed items over) and the
    two-segment window took two segments."""
    env = dict(os.environ, PYTHONPATH=ROOT, PF_K12C_MINR="1")
    env.pop("PF_K12_CAP", None)
    r = subprocess.run([sys.executable, "-c", "from tests.test_methmer_siteside_gpu import _child; _child()"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = {ln.split()[1]: (int(ln.split()[2]), int(ln.split()[3])) for ln in r.stdout.splitlines() if ln.startswith("CASE")}
    assert set(got) == set(CASES) | {"cap100"}
    for name, (path, items) in got.items():
        assert items >= 1, name
        assert path == (2 if name == "two_segments" else 1), name
