"""The given-regions kernels (pf_region_sums) against one literal reference
(tests/_regions_ref.py: every region walks every site), on CSRs built here as
test_dmr_gpu.py builds its own (no BAM).  Every case runs with 64, 256 and 1,024
sites per workgroup against one reference: all integers, all exact.
"""
import functools

import numpy as np
import pytest

from pomfret_amd.abi import DmrConfig

from tests._regions_ref import add, region_ref, same
from tests.test_dmr_gpu import M, P, U, Z, _pile

pytestmark = pytest.mark.gpu

BLOCKS = (64, 256, 1024)
CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=500, min_sites=5)


def _sites(n, seed):
    """n sites 1 to 9 bases apart: the four kinds of test_dmr_gpu.py and random
    counts, a quarter of them below min_cov on one haplotype."""
    rng = np.random.default_rng(seed)
    pos = 100 + np.cumsum(rng.integers(1, 10, n))
    kinds = np.array([P, M, Z, U], np.uint32)
    c4 = kinds[rng.integers(0, 4, n)]
    rnd = rng.random(n) < 0.5
    c4[rnd] = rng.integers(0, 40, (int(rnd.sum()), 4))
    return pos.astype(np.uint32), c4


def _regions(pos, seed):
    """One shuffled list of every kind of region the header allows."""
    n = len(pos)
    reg = [(5, 5), (0, 0), (0, 1), (2 ** 32 - 1, 2 ** 32 - 1), (0, 2 ** 32 - 1)]
    if n:
        first, last = int(pos[0]), int(pos[-1])
        reg += [(0, first), (0, first + 1), (first, first), (last + 1, last + 1000), (last, last + 1), (last + 1, last + 1),
                (0, last + 1), (first, last + 1), (first, last), (first + 1, last + 1)]
        idx = {0, n - 1, n // 2}
        for k in range(4):
            idx |= {4 * k, 4 * k + 1}
        for b in BLOCKS:
            for k in range(1, 5):
                idx |= {b * k - 1, b * k, b * k + 1}
        idx = sorted(i for i in idx if 0 <= i < n)
        for i in idx:                                        # one-site regions, and one base off on either side
            p = int(pos[i])
            reg += [(p, p + 1), (p - 1, p + 1), (p, p + 2), (p + 1, p + 2), (p - 1, p)]
        for i, j in zip(idx[::3], idx[2::3]):                # start and end exactly on a site, and one off
            a, b = int(pos[i]), int(pos[j])
            reg += [(a, b), (a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)]
        mid = n // 2
        for w in (1, 3, 40, 700):                            # nested around the middle site, then overlapping pairs
            lo, hi = max(mid - w, 0), min(mid + w, n - 1)
            reg += [(int(pos[lo]), int(pos[hi]) + 1)]
            reg += [(int(pos[lo]), int(pos[mid]) + 1), (int(pos[max(mid - w // 2, 0)]), int(pos[hi]))]
        reg += reg[5:15] + reg[-3:]                          # duplicated
    rng = np.random.default_rng(seed)
    reg = [reg[i] for i in rng.permutation(len(reg))]
    return np.array([r[0] for r in reg], np.uint32), np.array([r[1] for r in reg], np.uint32)


@functools.lru_cache(maxsize=None)
def _case(n):
    pos, c4 = _sites(n, 7 + n)
    pile = _pile(pos, c4)
    starts, ends = _regions(pos, n)
    return pile, starts, ends, region_ref(pile["pos"], pile["cnt"], CFG, starts, ends)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 4097])
def test_sizes(gpu_ctx, n, block):
    pile, starts, ends, ref = _case(n)
    got = gpu_ctx.region_sums(pile, CFG, starts, ends, block=block)
    same(got, ref, (n, block))
    whole = int(np.flatnonzero((starts == 0) & (ends == 2 ** 32 - 1))[0])
    assert got["n_cpg"][whole] == n and got["n_sites"][whole] == ref["n_informative"]
    assert got["n_cpg"][(starts == ends)].sum() == 0 and got["ms"] >= 0
    if n >= 63:
        assert ref["n_pos"].any() and ref["n_neg"].any() and (ref["n_sites"] > ref["n_pos"] + ref["n_neg"]).any()
        assert (ref["evidence"] > 0).any() and (ref["evidence"] < 0).any() and (ref["n_cpg"] > ref["n_sites"]).any()


def test_no_regions_and_the_default_block(gpu_ctx):
    pile, starts, ends, ref = _case(129)
    got = gpu_ctx.region_sums(pile, CFG)
    assert got["n_cpg"].size == 0 and got["sum"].shape == (0, 4) and got["n_informative"] == ref["n_informative"]
    same(gpu_ctx.region_sums(pile, CFG, starts, ends), ref, "block 0")
    # windows, none of them with a site; an empty window range
    e = _pile([], [], win_off=[0, 0, 0])
    got = gpu_ctx.region_sums(e, CFG, [0, 7], [9, 7])
    assert got["n_cpg"].tolist() == [0, 0] and not got["sum"].any() and got["n_informative"] == 0
    got = gpu_ctx.region_sums(pile, CFG, starts, ends, w0=1, w1=1)
    assert not got["n_cpg"].any() and not got["evidence"].any()


def test_the_cfg_reaches_the_kernels(gpu_ctx):
    pile, starts, ends, ref = _case(129)
    cfg = DmrConfig(min_cov=8, min_delta_pct=70, max_gap=1, min_sites=99)
    other = region_ref(pile["pos"], pile["cnt"], cfg, starts, ends)
    assert other["n_informative"] < ref["n_informative"] and not np.array_equal(other["n_pos"], ref["n_pos"])
    for block in BLOCKS:
        same(gpu_ctx.region_sums(pile, cfg, starts, ends, block=block), other, block)


@pytest.mark.parametrize("block", BLOCKS)
def test_window_sub_range(gpu_ctx, block):
    pos, c4 = _sites(270, 3)
    pile = _pile(pos, c4, win_off=[0, 80, 200, 270])
    starts, ends = _regions(pos, 3)
    cnt = pile["cnt"].reshape(-1, 6)
    for w0, w1, s0, s1 in ((1, 2, 80, 200), (1, 3, 80, 270), (0, 3, 0, 270)):
        ref = region_ref(pos[s0:s1], cnt[s0:s1], CFG, starts, ends)
        same(gpu_ctx.region_sums(pile, CFG, starts, ends, w0=w0, w1=w1, block=block), ref, (w0, w1, block))


@pytest.mark.parametrize("j", [1024, 1000])
def test_additivity(gpu_ctx, j):
    """Sites [0, j) plus sites [j, n) is the whole, field by field, for j on
    and off a block edge."""
    n = 2100
    pos, c4 = _sites(n, 11)
    starts, ends = _regions(pos, 11)
    cut = _pile(pos, c4, win_off=[0, j, n])
    ref = region_ref(cut["pos"], cut["cnt"], CFG, starts, ends)
    cross = (starts <= pos[j - 1]) & (ends > pos[j])          # a site on either side of the cut
    assert cross.sum() > 3
    for block in BLOCKS:
        a = gpu_ctx.region_sums(cut, CFG, starts, ends, w0=0, w1=1, block=block)
        b = gpu_ctx.region_sums(cut, CFG, starts, ends, w0=1, w1=2, block=block)
        assert a["n_cpg"][cross].all() and b["n_cpg"][cross].all()
        same(add(a, b), ref, (j, block))
        same(gpu_ctx.region_sums(cut, CFG, starts, ends, block=block), ref, (j, block, "one call"))


def test_sums_past_32_bits(gpu_ctx):
    n, F = 70_000, 65535
    pos = np.arange(n, dtype=np.uint32) * 2 + 10
    c4 = np.tile(np.array([[F, 0, 3, F]], np.uint32), (n, 1))
    pile = _pile(pos, c4)
    starts = np.array([0, 10, 10 + 2 * 66_000, 11, 0], np.uint32)
    ends = np.array([2 ** 32 - 1, 10 + 2 * 66_000, 10 + 2 * n, 10 + 2 * 69_999, 10], np.uint32)
    ref = region_ref(pile["pos"], pile["cnt"], CFG, starts, ends)
    assert ref["sum"][0].tolist() == [n * F, 0, 3 * n, n * F] and n * F > 2 ** 32 and ref["evidence"][0] > 2 ** 32
    assert ref["sum"][1][0] > 2 ** 32 > ref["sum"][2][0]
    for block in BLOCKS:
        same(gpu_ctx.region_sums(pile, CFG, starts, ends, block=block), ref, block)


def test_errors(gpu_ctx):
    """Error codes of the validating pass and of the argument checks."""
    from pomfret_amd import PomfretError
    pos = np.arange(200) * 3
    ok = _pile(pos, [P] * 200)
    bad = pos.copy()
    bad[130] = bad[129]                                        # equal is not ascending
    for block in BLOCKS + (0,):
        with pytest.raises(PomfretError, match="argument"):
            gpu_ctx.region_sums(_pile(bad, [P] * 200), CFG, [0], [1000], block=block)
        with pytest.raises(PomfretError, match="limit"):
            gpu_ctx.region_sums(_pile(pos, [P] * 150 + [(65536, 0, 0, 9)] + [P] * 49), CFG, [0], [1000], block=block)
    with pytest.raises(PomfretError, match="argument"):        # and without a region to look up
        gpu_ctx.region_sums(_pile(bad, [P] * 200), CFG)
    # overlapping windows: each ascending inside, not across
    two = _pile(np.concatenate([np.arange(100), 50 + np.arange(100)]), [U] * 200, win_off=[0, 100, 200])
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.region_sums(two, CFG, [0], [10])
    assert gpu_ctx.region_sums(two, CFG, [0], [60], w0=1, w1=2)["n_cpg"].tolist() == [10]
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.region_sums(ok, CFG, [0, 9, 0], [5, 8, 7])     # start > end
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.region_sums(_pile([], []), CFG, [9], [8])      # ... also where no site is
    for block in (1, 32, 100, 2048, 1 << 20):
        with pytest.raises(PomfretError, match="argument"):
            gpu_ctx.region_sums(ok, CFG, [0], [5], block=block)
    with pytest.raises(PomfretError, match="argument"):
        gpu_ctx.region_sums(ok, DmrConfig(5, 101, 500, 5), [0], [5])
    assert gpu_ctx.region_sums(ok, CFG, [0], [31])["n_cpg"].tolist() == [11]


def test_block_override_in_the_environment(gpu_ctx, monkeypatch):
    """PF_REG_BLOCK is read by every call with block 0: 64 and the default give
    the same records; a value that is no power of two in [64, 1024] is refused."""
    from pomfret_amd import PomfretError
    pile, starts, ends, ref = _case(4097)
    monkeypatch.setenv("PF_REG_BLOCK", "64")
    same(gpu_ctx.region_sums(pile, CFG, starts, ends), ref, "PF_REG_BLOCK=64")
    for v in ("100", "32", "1048576", "x", "64x"):
        monkeypatch.setenv("PF_REG_BLOCK", v)
        with pytest.raises(PomfretError, match="argument"):
            gpu_ctx.region_sums(pile, CFG, starts, ends)
        same(gpu_ctx.region_sums(pile, CFG, starts, ends, block=256), ref, "an explicit block wins")
    monkeypatch.delenv("PF_REG_BLOCK")
    same(gpu_ctx.region_sums(pile, CFG, starts, ends), ref, "default")
