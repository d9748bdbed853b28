"""The allele-specific region kernels (pf_dmr_regions) against one literal
sequential reference, on CSRs built here (no BAM).  Every case runs with 64
sites per workgroup and with the default block, and the two results are
compared with each other and with the reference: all integers, all exact.
"""
import bisect
import os
import subprocess
import sys

import numpy as np
import pytest

from pomfret_amd.abi import DmrConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("start", "end", "n_sites", "sign", "sum", "open")

P = (10, 0, 0, 10)       # informative, h1 > h2
M = (0, 10, 10, 0)       # informative, h1 < h2
Z = (5, 5, 5, 5)         # informative, no direction
U = (1, 0, 0, 1)         # below min_cov: transparent


def _dmr_ref(pos, cnt, cfg, breaks=()):
    """The runs of the sites (pos [n], cnt [n, 6] or [n, 3, 2]) as the header
    states them: one loop over the sites holding the current run.  Returns the
    dict of Context.dmr_regions plus "all", every run before the min_sites
    filter."""
    brk = sorted(int(x) for x in breaks)
    runs, cur, prev, n_inf = [], None, None, 0
    for p, c in zip(np.asarray(pos).tolist(), np.asarray(cnt).reshape(-1, 6).tolist()):
        m1, u1, m2, u2 = c[:4]
        n1, n2 = m1 + u1, m2 + u2
        if n1 < cfg.min_cov or n2 < cfg.min_cov:
            continue
        n_inf += 1
        d, t = (m1 * n2 - m2 * n1) * 100, cfg.min_delta_pct * n1 * n2
        sign = 1 if d >= t else (-1 if -d >= t else 0)
        joined = False
        if prev is not None and sign != 0 and prev[1] == sign and p - prev[0] <= cfg.max_gap:
            i = bisect.bisect_right(brk, prev[0])            # the first break above the previous site
            joined = not (i < len(brk) and brk[i] <= p)
        if not joined:
            if cur is not None:
                runs.append(cur)
            cur = None
            if sign != 0:
                cur = dict(start=p, end=p + 1, n_sites=0, sign=sign, sum=[0, 0, 0, 0], open=1 if n_inf == 1 else 0)
        if cur is not None:
            cur["end"] = p + 1
            cur["n_sites"] += 1
            cur["sum"] = [a + b for a, b in zip(cur["sum"], (m1, u1, m2, u2))]
        prev = (p, sign)
    if cur is not None:
        cur["open"] |= 2
        runs.append(cur)
    kept = [r for r in runs if r["n_sites"] >= cfg.min_sites or r["open"]]
    return dict(_arrays(kept), n_informative=n_inf, all=runs)


def _arrays(runs):
    n = len(runs)
    return dict(start=np.array([r["start"] for r in runs], np.uint32), end=np.array([r["end"] for r in runs], np.uint32),
                n_sites=np.array([r["n_sites"] for r in runs], np.uint32),
                sign=np.array([r["sign"] for r in runs], np.int32),
                sum=np.array([r["sum"] for r in runs], np.uint64).reshape(n, 4),
                open=np.array([r["open"] for r in runs], np.uint32))


def _pile(pos, c4, win_off=None):
    pos = np.asarray(pos, np.uint32)
    cnt = np.zeros((pos.size, 6), np.uint32)
    if pos.size:
        cnt[:, :4] = np.asarray(c4, np.uint32).reshape(-1, 4)
        cnt[:, 4] = 3                                          # the "other" class is ignored
    return dict(win_off=np.array([0, pos.size] if win_off is None else win_off, np.uint64), pos=pos,
                cnt=cnt.reshape(-1, 3, 2))


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k][:8], b[k][:8])
    assert a["n_informative"] == b["n_informative"], what


def _check(ctx, pile, cfg, breaks=None, w0=0, w1=None):
    """Block 64 against the default block against the reference."""
    wo = pile["win_off"].astype(np.int64)
    s0, s1 = int(wo[w0]), int(wo[len(wo) - 1 if w1 is None else w1])
    ref = _dmr_ref(pile["pos"][s0:s1], pile["cnt"].reshape(-1, 6)[s0:s1], cfg, () if breaks is None else breaks)
    small = ctx.dmr_regions(pile, cfg, breaks, w0, w1, block=64)
    deflt = ctx.dmr_regions(pile, cfg, breaks, w0, w1)
    _same(small, deflt, "block 64 against the default block")
    _same(deflt, ref, "device against the reference")
    return ref


CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=500, min_sites=5)


def test_empty_inputs(gpu_ctx):
    r = _check(gpu_ctx, _pile([], []), CFG)
    assert r["start"].size == 0 and r["n_informative"] == 0
    # windows, none of them with a site; an empty window range
    e = _pile([], [], win_off=[0, 0, 0])
    assert _check(gpu_ctx, e, CFG)["start"].size == 0
    assert gpu_ctx.dmr_regions(_pile([7], [P]), CFG, w0=1, w1=1)["start"].size == 0
    # one site; every site below min_cov
    r = _check(gpu_ctx, _pile([7], [P]), CFG)
    assert r["open"].tolist() == [3] and r["n_sites"].tolist() == [1]
    r = _check(gpu_ctx, _pile(np.arange(200) * 3, [U] * 200), CFG)
    assert r["start"].size == 0 and r["n_informative"] == 0


def test_one_run_over_five_blocks(gpu_ctx):
    r = _check(gpu_ctx, _pile(100 + np.arange(300) * 7, [P] * 300), CFG)
    assert r["n_sites"].tolist() == [300] and r["open"].tolist() == [3] and r["sum"][0].tolist() == [3000, 0, 0, 3000]


@pytest.mark.parametrize("last", [63, 64, 65])
def test_run_ends_at_a_block_edge(gpu_ctx, last):
    c4 = [P] * (last + 1) + [M] * (200 - last - 1)
    r = _check(gpu_ctx, _pile(np.arange(200) * 5, c4), CFG)
    assert r["n_sites"].tolist() == [last + 1, 200 - last - 1] and r["open"].tolist() == [1, 2]
    # and with a closed run in front, so the edge run is an interior one
    c4 = [M] * 6 + [Z] + [P] * (last + 1 - 7) + [Z] + [M] * 20
    r = _check(gpu_ctx, _pile(np.arange(len(c4)) * 5, c4), CFG)
    assert r["n_sites"].tolist() == [6, last + 1 - 7, 20] and r["open"].tolist() == [1, 0, 2]


def test_join_across_uninformative_blocks(gpu_ctx):
    # sites 0..39 one run, then three whole 64-blocks (and more) of transparent
    # sites, then the run goes on: its neighbours are 231 bases apart, inside max_gap
    c4 = [P] * 40 + [U] * 230 + [P] * 30 + [M] * 8
    r = _check(gpu_ctx, _pile(np.arange(len(c4)), c4), CFG)
    assert r["n_sites"].tolist() == [70, 8]
    # the same with max_gap one base short
    r = _check(gpu_ctx, _pile(np.arange(len(c4)), c4), DmrConfig(5, 40, 230, 5))
    assert r["n_sites"].tolist() == [40, 30, 8]


def test_alternating_signs(gpu_ctx):
    c4 = [P, M] * 150
    r = _check(gpu_ctx, _pile(np.arange(300) * 2, c4), DmrConfig(5, 40, 500, 1))
    assert r["start"].size == 300 and set(r["n_sites"].tolist()) == {1}
    r = _check(gpu_ctx, _pile(np.arange(300) * 2, c4), CFG)          # only the two open ones come back
    assert r["open"].tolist() == [1, 2]


def test_thresholds(gpu_ctx):
    cfg = DmrConfig(min_cov=5, min_delta_pct=50, max_gap=500, min_sites=1)
    # 7/10 against 2/10 is exactly 50 points: a direction, and it joins
    r = _check(gpu_ctx, _pile([10, 20, 30], [(7, 3, 2, 8)] * 3), cfg)
    assert r["n_sites"].tolist() == [3] and r["sign"].tolist() == [1]
    r = _check(gpu_ctx, _pile([10, 20, 30], [(2, 8, 7, 3)] * 3), cfg)
    assert r["n_sites"].tolist() == [3] and r["sign"].tolist() == [-1]
    # 6/10 against 2/10 is 40 points: informative, no direction, it ends the run
    r = _check(gpu_ctx, _pile([10, 20, 30], [(7, 3, 2, 8), (6, 4, 2, 8), (7, 3, 2, 8)]), cfg)
    assert r["n_sites"].tolist() == [1, 1] and r["n_informative"] == 3
    # min_cov on either haplotype; min_cov - 1 is transparent and the run passes over it
    r = _check(gpu_ctx, _pile([10, 20, 30], [(5, 0, 0, 5), (4, 0, 0, 5), (5, 0, 0, 5)]), cfg)
    assert r["n_sites"].tolist() == [2] and r["n_informative"] == 2
    r = _check(gpu_ctx, _pile([10, 20, 30], [(5, 0, 0, 5), (5, 0, 0, 4), (5, 0, 0, 5)]), cfg)
    assert r["n_sites"].tolist() == [2] and r["n_informative"] == 2


def test_full_counts_need_64_bit_products(gpu_ctx):
    F = 65535
    # second site: m1 * n2 = 65535 * 131070 passes 2^32 and m2 * n1 does not, so 32-bit products give the
    # wrong direction; the first, the second and the last sit exactly on the 50-point threshold
    c4 = [(F, F, 0, F), (F, 0, F, F), (F, F, F, F), (F, 0, 0, F), (F, 0, 0, F), (0, F, F, F)]
    r = _check(gpu_ctx, _pile(np.arange(6) * 10, c4), DmrConfig(5, 50, 500, 1))
    assert r["n_sites"].tolist() == [2, 2, 1] and r["sign"].tolist() == [1, 1, -1]
    assert r["sum"][0].tolist() == [2 * F, F, F, 2 * F]
    big = _pile([1, 2], [(F + 1, 0, 0, 9), P])
    from pomfret_amd import PomfretError
    with pytest.raises(PomfretError, match="limit"):
        gpu_ctx.dmr_regions(big, CFG)


def test_breaks(gpu_ctx):
    pos = 1000 + np.arange(150) * 4
    pile = _pile(pos, [P] * 150)
    assert _check(gpu_ctx, pile, CFG, None)["n_sites"].tolist() == [150]
    # a break at a member's position parts it from its left neighbour
    assert _check(gpu_ctx, pile, CFG, [int(pos[70])])["n_sites"].tolist() == [70, 80]
    # a break between two members; a break at the first site and one past the last change nothing
    assert _check(gpu_ctx, pile, CFG, [int(pos[70]) + 1])["n_sites"].tolist() == [71, 79]
    assert _check(gpu_ctx, pile, CFG, [0, int(pos[0]), int(pos[-1]) + 1, 1 << 31])["n_sites"].tolist() == [150]
    # 1,000 breaks, most of them between sites, two of them equal
    rng = np.random.default_rng(3)
    brk = np.sort(rng.integers(900, 1700, 1000)).tolist()
    r = _check(gpu_ctx, pile, DmrConfig(5, 40, 500, 1), brk)
    assert r["start"].size > 50
    from pomfret_amd import PomfretError
    with pytest.raises(PomfretError):
        gpu_ctx.dmr_regions(pile, CFG, [5, 4])


def test_window_sub_range(gpu_ctx):
    c4 = [P] * 90 + [M] * 90 + [P] * 90
    pile = _pile(np.arange(270) * 3, c4, win_off=[0, 80, 200, 270])
    assert _check(gpu_ctx, pile, CFG)["n_sites"].tolist() == [90, 90, 90]
    r = _check(gpu_ctx, pile, CFG, w0=1, w1=2)
    assert r["n_sites"].tolist() == [10, 90, 20] and r["open"].tolist() == [1, 0, 2]
    r = _check(gpu_ctx, pile, CFG, w0=1, w1=3)
    assert r["n_sites"].tolist() == [10, 90, 90] and r["start"][0] == 80 * 3


def test_non_ascending_range_is_refused(gpu_ctx):
    from pomfret_amd import PomfretError
    pos = np.arange(200) * 3
    pos[130] = pos[129]                                        # equal is not ascending
    for block in (64, 0):
        with pytest.raises(PomfretError, match="argument"):
            gpu_ctx.dmr_regions(_pile(pos, [P] * 200), CFG, block=block)
    # overlapping windows: each ascending inside, not across
    two = _pile(np.concatenate([np.arange(100), 50 + np.arange(100)]), [U] * 200, win_off=[0, 100, 200])
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.dmr_regions(two, CFG)
    assert gpu_ctx.dmr_regions(two, CFG, w0=1, w1=2)["start"].size == 0


def _markov_pile():
    """5,000 sites over 7 windows; the per-site state (h1 > h2, h1 < h2, no
    direction) follows a 3-state Markov chain that stays with probability
    0.985, so runs of 1 to 200 and more occur; one site in six is transparent."""
    rng = np.random.default_rng(20)
    n = 5000
    pos = np.cumsum(rng.integers(1, 60, n)).astype(np.uint32)
    state = np.zeros(n, np.int64)
    for i in range(1, n):
        state[i] = state[i - 1] if rng.random() < 0.985 else rng.integers(0, 3)
    c4 = np.zeros((n, 4), np.uint32)
    for i in range(n):
        n1, n2 = rng.integers(5, 40, 2)
        hi, lo = rng.integers(80, 101) / 100.0, rng.integers(0, 21) / 100.0
        f1, f2 = [(hi, lo), (lo, hi), (0.5, 0.5)][state[i]]
        m1, m2 = int(round(n1 * f1)), int(round(n2 * f2))
        c4[i] = (m1, n1 - m1, m2, n2 - m2)
    c4[rng.random(n) < 1 / 6] = U
    win_off = [0] + sorted(rng.choice(np.arange(1, n), 6, replace=False).tolist()) + [n]
    return _pile(pos, c4, win_off=win_off)


@pytest.fixture(scope="module")
def markov():
    return _markov_pile()


MARKOV_CFGS = [DmrConfig(5, 40, 500, 5), DmrConfig(8, 60, 120, 2), DmrConfig(5, 25, 2000, 20)]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_markov_csr(gpu_ctx, markov, k):
    cfg = MARKOV_CFGS[k]
    brk = [] if k == 0 else np.sort(np.random.default_rng(k).choice(markov["pos"], 12)).tolist()
    ref = _check(gpu_ctx, markov, cfg, brk)
    kept = [r for r in ref["all"] if r["n_sites"] >= cfg.min_sites]
    assert any(r["sign"] > 0 for r in kept) and any(r["sign"] < 0 for r in kept)
    assert max(r["n_sites"] for r in ref["all"]) > 128
    assert ref["open"].any()
    assert len(ref["all"]) > len(kept)                         # min_sites drops something


@pytest.mark.parametrize("k", [0, 1, 2])
def test_stitch_invariance(gpu_ctx, markov, k):
    """Cut at every window boundary, each part through the device, stitched:
    the one-call result after min_sites."""
    from pomfret_amd.pipeline import dmr_stitch
    cfg = MARKOV_CFGS[k]
    brk = [] if k == 0 else np.sort(np.random.default_rng(k).choice(markov["pos"], 12)).tolist()
    W = markov["win_off"].size - 1
    for block in (64, 0):
        parts = [gpu_ctx.dmr_regions(markov, cfg, brk, w, w + 1, block=block) for w in range(W)]
        got = dmr_stitch(parts, cfg, brk)
        one = gpu_ctx.dmr_regions(markov, cfg, brk, block=block)
        keep = one["n_sites"] >= cfg.min_sites
        assert keep.sum() > 3 and not got["open"].any()
        for key in ("start", "end", "n_sites", "sign", "sum"):
            assert np.array_equal(got[key], one[key][keep]), key
        assert got["n_informative"] == one["n_informative"]


def test_block_override_in_the_environment():
    """PF_DMR_BLOCK: 64 and the default give the same records; a value that is
    no power of two in [64, default] is refused.  A fresh process each."""
    code = ("import numpy as np\n"
            "from pomfret_amd import Context, PomfretError\n"
            "from tests.test_dmr_gpu import _pile, P, M, CFG\n"
            "ctx = Context(0)\n"
            "pile = _pile(np.arange(400) * 3, [P] * 150 + [M] * 250)\n"
            "try:\n"
            "    r = ctx.dmr_regions(pile, CFG)\n"
            "    print('RUNS', r['n_sites'].tolist(), r['open'].tolist())\n"
            "except PomfretError as e:\n"
            "    print('REFUSED', e)\n"
            "ctx.close()\n")
    out = {}
    for v in ("64", "", "100", "32", "1048576", "64x"):
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("PF_DMR_BLOCK", None)
        if v:
            env["PF_DMR_BLOCK"] = v
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr
        out[v] = r.stdout.strip().splitlines()[-1]
    assert out["64"] == out[""] == "RUNS [150, 250] [1, 2]"
    for v in ("100", "32", "1048576", "64x"):
        assert out[v].startswith("REFUSED") and "argument" in out[v]
