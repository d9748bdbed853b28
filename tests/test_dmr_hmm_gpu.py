"""The hidden Markov model kernels (pf_dmr_hmm_regions) against the literal
sequential reference (tests/_dmr_hmm_ref.py), on CSRs built here (no BAM).
Every case runs with 64, 256 and 1,024 sites per workgroup; the states, the
evidence, every field of every run, n_informative and n_chains are compared
with the reference as exact equality: all integers.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from pomfret_amd.abi import DmrConfig, HmmConfig

from tests._dmr_hmm_ref import hmm_ref, same
from tests.test_dmr_gpu import M, P, U, Z, _pile
from tests.test_dmr_hmm import planted_pile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = (64, 256, 1024)
CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=500, min_sites=5)
ONE = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=500, min_sites=1)
HMM = HmmConfig()
W = (7, 3, 3, 7)         # informative, weakly h1 > h2: below the site cost's worth on its own


def _check(ctx, pile, cfg=CFG, hcfg=HMM, breaks=None, w0=0, w1=None):
    """Every block against the reference of the range."""
    wo = pile["win_off"].astype(np.int64)
    s0, s1 = int(wo[w0]), int(wo[len(wo) - 1 if w1 is None else w1])
    ref = hmm_ref(pile["pos"][s0:s1], pile["cnt"].reshape(-1, 6)[s0:s1], cfg, hcfg, () if breaks is None else breaks)
    for block in BLOCKS:
        got = ctx.dmr_hmm_regions(pile, cfg, hcfg, breaks, w0, w1, block=block, sites=True)
        same(got, ref, f"block {block}")
        assert not got["open"].any()
    return ref


def _mixed(n, seed):
    """n sites: stretches of P, M, Z, W and U of random lengths, one site in ten replaced by noise."""
    rng = np.random.default_rng(seed)
    c4 = []
    while len(c4) < n:
        c4 += [[P, M, Z, W, U][rng.integers(0, 5)]] * int(rng.integers(1, 30))
    c4 = np.array(c4[:n], np.uint32).reshape(-1, 4)
    noise = rng.random(n) < 0.1
    c4[noise] = rng.integers(0, 14, (int(noise.sum()), 4))
    return _pile(200 + np.cumsum(rng.integers(1, 90, n)), c4)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4097])
def test_sizes(gpu_ctx, n):
    ref = _check(gpu_ctx, _mixed(n, n + 1), ONE)
    assert ref["state"].size == n
    if n >= 63:
        assert ref["n_chains"] >= 1 and len(ref["kept"]) >= 1
    if n >= 129:
        assert {0, 1, 2, 255} <= set(ref["state"].tolist()) and len(ref["kept"]) >= 2


def test_empty_ranges_and_no_informative_site(gpu_ctx):
    r = _check(gpu_ctx, _pile([], [], win_off=[0, 0, 0]))
    assert r["start"].size == 0 and r["n_informative"] == 0 and r["n_chains"] == 0
    got = gpu_ctx.dmr_hmm_regions(_pile([7], [P]), CFG, HMM, w0=1, w1=1, sites=True)
    assert got["start"].size == 0 and got["state"].size == 0 and got["evidence"].size == 0
    r = _check(gpu_ctx, _pile(np.arange(300) * 3, [U] * 300))
    assert r["n_informative"] == 0 and r["n_chains"] == 0 and set(r["state"].tolist()) == {255}
    # without sites=True the two arrays are not returned
    assert "state" not in gpu_ctx.dmr_hmm_regions(_pile([7], [P]), CFG, HMM)


def test_chain_of_one_site(gpu_ctx):
    # 10 / 0 against 0 / 10 is worth more than the site cost: state 1 without any neighbour
    r = _check(gpu_ctx, _pile([7], [P]), ONE)
    assert r["state"].tolist() == [1] and r["n_chains"] == 1 and r["n_sites"].tolist() == [1]
    # three chains of one site each (1,000 apart), and min_sites drops them
    r = _check(gpu_ctx, _pile([7, 1007, 2007], [P, Z, M]), ONE)
    assert r["state"].tolist() == [1, 0, 2] and r["n_chains"] == 3 and r["sign"].tolist() == [1, -1]
    assert _check(gpu_ctx, _pile([7, 1007, 2007], [P, Z, M]), CFG)["start"].size == 0


def _edges_pile(transparent_on_edges):
    """4,300 informative sites whose segments (P, M, Z in turn) begin exactly
    at 4k, 64k and block * k informative sites into the range and next to
    them; every fourth boundary also opens a new chain (a gap of max_gap + 1).
    transparent_on_edges: a transparent site in front of every boundary, so the
    boundaries sit at thread, wave and block edges of the compacted sites but
    not of the range's, and the other way round."""
    edges = sorted({e + d for e in (4, 8, 12, 64, 128, 192, 256, 512, 768, 1024, 2048, 3072, 4096) for d in (-1, 0, 1)})
    c4, pos, p, seg = [], [], 100, 0
    for j in range(4300):
        if j in edges:
            seg += 1
            p += 501 if seg % 4 == 0 else 3
            if transparent_on_edges:
                c4.append(U)
                pos.append(p)
                p += 1
        else:
            p += 3
        c4.append((P, M, Z)[(seg + seg // 3) % 3])
        pos.append(p)
    return _pile(pos, c4), len(edges)


@pytest.mark.parametrize("transparent", [False, True])
def test_chains_and_states_change_at_thread_wave_and_block_edges(gpu_ctx, transparent):
    pile, n_edges = _edges_pile(transparent)
    r = _check(gpu_ctx, pile, ONE)
    assert r["n_informative"] == 4300 and r["n_chains"] == 1 + n_edges // 4
    assert len(r["all"]) > n_edges // 2 and {0, 1, 2} <= set(r["state"].tolist())
    assert (255 in r["state"].tolist()) == transparent


def test_transparent_sites_on_the_ranges_block_edges(gpu_ctx):
    # one long region; the sites at the compaction's thread, wave and block edges are transparent
    c4 = [P] * 2200
    for i in (3, 4, 63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024, 1025, 2047, 2048):
        c4[i] = U
    r = _check(gpu_ctx, _pile(np.arange(2200) * 2, c4))
    assert r["n_sites"].tolist() == [2200 - 15] and r["n_chains"] == 1


def test_max_gap(gpu_ctx):
    c4 = [P] * 12
    pos = np.arange(12) * 10
    pos[6:] += 490                                             # neighbours 5 and 6 are exactly max_gap apart
    r = _check(gpu_ctx, _pile(pos, c4))
    assert r["n_chains"] == 1 and r["n_sites"].tolist() == [12]
    pos[6:] += 1
    r = _check(gpu_ctx, _pile(pos, c4))
    assert r["n_chains"] == 2 and r["n_sites"].tolist() == [6, 6]


def test_breaks(gpu_ctx):
    pos = 1000 + np.arange(150) * 4
    pile = _pile(pos, [P] * 150)
    assert _check(gpu_ctx, pile)["n_sites"].tolist() == [150]
    # a break at a site's position (x == b) parts it from its left neighbour
    r = _check(gpu_ctx, pile, breaks=[int(pos[70])])
    assert r["n_sites"].tolist() == [70, 80] and r["n_chains"] == 2
    # a break between two adjacent sites; one at the first site and one past the last change nothing
    assert _check(gpu_ctx, pile, breaks=[int(pos[70]) + 1])["n_sites"].tolist() == [71, 79]
    assert _check(gpu_ctx, pile, breaks=[0, int(pos[0]), int(pos[-1]) + 1, 1 << 31])["n_chains"] == 1
    rng = np.random.default_rng(3)
    r = _check(gpu_ctx, pile, ONE, breaks=np.sort(rng.integers(900, 1700, 1000)).tolist())
    assert r["n_chains"] > 50
    from pomfret_amd import PomfretError
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.dmr_hmm_regions(pile, CFG, HMM, [5, 4])


def test_all_ties_give_state_zero(gpu_ctx):
    """Every e is 0 and both costs are 0: every path scores 0, and the tie rules
    (stay where you are, else the smallest state) keep state 0 everywhere."""
    pile = _pile(np.arange(700) * 3, [Z] * 700)
    r = _check(gpu_ctx, pile, ONE, HmmConfig(0.0, 0.0))
    assert set(r["state"].tolist()) == {0} and r["start"].size == 0 and r["n_chains"] == 1
    assert not r["evidence"].any()


def test_switch_zero_and_costs_at_64_bits(gpu_ctx):
    pile = _mixed(1500, 77)
    r0 = _check(gpu_ctx, pile, ONE, HmmConfig(2.0, 0.0))
    r8 = _check(gpu_ctx, pile, ONE, HMM)
    assert len(r0["all"]) > len(r8["all"]) > 3                 # a free switch follows every site
    # 64 bits a site and a switch: only full counters (2^28 = 4,096 bits) still make regions
    F = 60000
    c4 = [P] * 100 + [(F, 0, 0, F)] * 70 + [P] * 100 + [(0, F, F, 0)] * 70 + [P] * 10
    r = _check(gpu_ctx, _pile(np.arange(len(c4)) * 3, c4), ONE, HmmConfig(64.0, 64.0))
    assert r["n_sites"].tolist() == [70, 70] and r["sign"].tolist() == [1, -1]
    from pomfret_amd import PomfretError
    for bad in (HmmConfig(64.001, 8.0), HmmConfig(2.0, -0.001)):
        with pytest.raises(PomfretError, match="argument"):
            gpu_ctx.dmr_hmm_regions(pile, CFG, bad)


def test_full_counters_and_the_limit(gpu_ctx):
    F = 65535
    c4 = [(F, 0, 0, F)] * 40 + [(F, F, F, F)] * 30 + [(0, F, F, F)] * 40 + [(F, F, 0, F)] * 40
    r = _check(gpu_ctx, _pile(np.arange(150) * 10, c4), CFG)
    assert r["evidence"][0] == 1 << 28 and r["sum"][0].tolist() == [40 * F, 0, 0, 40 * F] and len(r["kept"]) >= 2
    from pomfret_amd import PomfretError
    for block in BLOCKS + (0,):
        with pytest.raises(PomfretError, match="limit"):
            gpu_ctx.dmr_hmm_regions(_pile([1, 2], [(F + 1, 0, 0, 9), P]), CFG, HMM, block=block)


def test_non_ascending_range_is_refused(gpu_ctx):
    from pomfret_amd import PomfretError
    pos = np.arange(200) * 3
    pos[130] = pos[129]                                        # equal is not ascending
    for block in BLOCKS:
        with pytest.raises(PomfretError, match="argument"):
            gpu_ctx.dmr_hmm_regions(_pile(pos, [P] * 200), CFG, HMM, block=block)
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.dmr_hmm_regions(_pile(np.arange(200)[::-1] * 3, [U] * 200), CFG, HMM)
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.dmr_hmm_regions(_pile(np.arange(200) * 3, [P] * 200), CFG, HMM, block=96)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_pileups_with_planted_regions(gpu_ctx, seed):
    """About 5,000 sites: planted regions of 3 to 300 CpGs among flat stretches, one site in eight
    transparent, a dozen breaks, three parameter sets."""
    rng = np.random.default_rng(100 + seed)
    lens = []
    while sum(lens) < 5000:
        lens += [int(rng.integers(20, 400)), int(rng.integers(3, 300))]
    pos, cnt, planted = planted_pile(seed, tuple(lens + [50]))
    cnt[rng.random(pos.size) < 1 / 8, :4] = U
    pile = dict(win_off=np.array([0, pos.size], np.uint64), pos=pos, cnt=cnt.reshape(-1, 3, 2))
    brk = np.sort(rng.choice(pos, 12)).tolist()
    cfg, hcfg = [(CFG, HMM), (DmrConfig(8, 60, 150, 2), HmmConfig(1.0, 4.0)), (DmrConfig(3, 25, 2000, 20), HmmConfig(3.5, 12.25))][seed - 1]
    r = _check(gpu_ctx, pile, cfg, hcfg, brk)
    assert any(x["sign"] > 0 for x in r["kept"]) and any(x["sign"] < 0 for x in r["kept"])
    assert len(r["all"]) >= len(r["kept"]) >= 5 and r["n_chains"] > 1
    if seed != 2:                                              # at min_cov 8 and max_gap 150 the chains are short
        assert max(x["n_sites"] for x in r["kept"]) > 64


def test_window_sub_range(gpu_ctx):
    pile = _mixed(900, 9)
    pile["win_off"] = np.array([0, 80, 80, 470, 900], np.uint64)
    whole = _check(gpu_ctx, pile, ONE)
    for w0, w1 in ((0, 1), (1, 2), (2, 3), (1, 4), (3, 4)):
        part = _check(gpu_ctx, pile, ONE, w0=w0, w1=w1)
        assert part["state"].size == int(pile["win_off"][w1]) - int(pile["win_off"][w0])
    assert whole["state"].size == 900


def test_block_override_in_the_environment():
    """PF_DMR_BLOCK: 64 and the default give the reference's result; a value
    that is no power of two in [64, 1024] is refused.  A fresh process each."""
    code = ("import numpy as np\n"
            "from pomfret_amd import Context, PomfretError\n"
            "from tests.test_dmr_hmm_gpu import _mixed, ONE, HMM\n"
            "from tests._dmr_hmm_ref import hmm_ref, same\n"
            "ctx = Context(0)\n"
            "pile = _mixed(700, 5)\n"
            "try:\n"
            "    r = ctx.dmr_hmm_regions(pile, ONE, HMM, sites=True)\n"
            "    same(r, hmm_ref(pile['pos'], pile['cnt'], ONE, HMM), 'env')\n"
            "    print('RUNS', r['start'].size)\n"
            "except PomfretError as e:\n"
            "    print('REFUSED', e)\n"
            "ctx.close()\n")
    out = {}
    for v in ("64", "", "100", "64x"):
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("PF_DMR_BLOCK", None)
        if v:
            env["PF_DMR_BLOCK"] = v
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stderr
        out[v] = r.stdout.strip().splitlines()[-1]
    assert out["64"] == out[""] and out[""].startswith("RUNS") and int(out[""].split()[1]) > 3
    for v in ("100", "64x"):
        assert out[v].startswith("REFUSED") and "argument" in out[v]
