"""The read-slice scan that the pileup, the permutation test, the rank test,
assign and tag-check share (pomfret_amd/csrc/pf_reads.h), at the edges the
stages' own tests do not reach: their reads only ever hold calls inside the
window.  Here every read is built from three parts,

    L  entries left of the window,  L  in {0, 1, 63, 64, 65}, the last at ws - 1,
    I  entries inside,              I  in {0, 1, 63, 64, 65, 128, 129}: at ws and
       at we - 1, with no-call (cat 2) entries and duplicate positions,
    Rr entries right of the window, Rr in {0, 1, 70}, the first at we,

in every combination, so that the seek lands at slice offsets 0, 1, 63, 64 and
65 and the stride over 64 calls a trip ends in its first, second and third
trip, both by exhausting the slice and by meeting a call past the end.  Each
combination is a candidate (tag 254) in one of three windows over [1000, 1400)
and tagged 0 / 1 (a few 3) in the other two; a window of length 1 follows.

Every stage is compared exactly with its own literal reference, at the default
geometry and at the smallest (64 threads, tiles of 64), and the stages with
each other: per window the four sums of the permutation test, of the rank test
at min_calls 1 and the column sums of the pileup's counters of haplotype 1 and
2 are the same numbers.  test_references_agree shows that for the references
alone, without a GPU."""
import numpy as np
import pytest

from pomfret_amd.abi import AssignConfig
from tests._assign_ref import assign_ref_batch
from tests._assign_ref import same as assign_same
from tests._perm_ref import perm_ref_batch
from tests._perm_ref import same as perm_same
from tests._rank_ref import rank_ref_batch
from tests._rank_ref import same as rank_same
from tests._tagcheck_ref import same as tagcheck_same
from tests._tagcheck_ref import tagcheck_ref_batch
from tests.test_pileup_gpu import _calls_batch, _cfg, _pile_ref
from tests.test_pileup_gpu import _same as pile_same

WS, WE = 1000, 1400
LEFT, INSIDE, RIGHT = (0, 1, 63, 64, 65), (0, 1, 63, 64, 65, 128, 129), (0, 1, 70)
N_PERM, SEED = 50, 3
MIN_COV, MIN_CALLS, Q16 = 1, 1, 65536
SMALL = ("PF_PERM_THREADS", "PF_RANK_THREADS", "PF_PILE_TILE", "PF_ASSIGN_TILE", "PF_TAGCHECK_TILE")


def _read(k, n_left, n_in, n_right):
    """Combination k's calls: sorted, n_left + n_in + n_right of them."""
    calls = [(WS - n_left + i, (i + k) % 3) for i in range(n_left)]                 # ..., ws - 1
    if n_in == 1:
        calls.append((WS if k % 2 else WE - 1, k % 2))
    elif n_in > 1:
        # ws, pairs of equal positions three apart, we - 1; every third entry a no-call
        calls.append((WS, k % 2))
        calls += [(WS + 1 + 3 * (i // 2), (i + k) % 3) for i in range(n_in - 2)]
        calls.append((WE - 1, (k + 1) % 2))
    calls += [(WE + 2 * i, (i + k) % 3) for i in range(n_right)]                    # we, ...
    assert len(calls) == n_left + n_in + n_right and calls == sorted(calls, key=lambda c: c[0])
    return calls


def _tag(k, widx):
    if k % 3 == widx:
        return 254
    return 3 if k % 35 == 4 else ((k * 2654435761 + widx * 40503) >> 9) & 1


def _build():
    combos = [(a, b, c) for a in LEFT for b in INSIDE for c in RIGHT]
    assert len(combos) == 105
    windows = [(WS, WE, [(_tag(k, widx), _read(k, *combos[k])) for k in range(len(combos))]) for widx in range(3)]
    windows.append((50, 51, [(0, [(49, 0), (50, 0), (51, 0)]), (1, [(50, 1)]), (254, [(50, 0)]), (0, [(50, 2)]),
                             (1, [(49, 1)]), (0, [(51, 0), (52, 1)])]))
    b = _calls_batch(windows)
    # the shapes the text above promises
    tags = np.asarray(b.read_hp)
    assert (tags == 254).sum() == 106 and (tags == 3).sum() >= 2 and (tags == 0).sum() > 80 and (tags == 1).sum() > 80
    pos = np.asarray(b.call_pos)
    assert pos.max() == WE + 2 * 69 and pos.min() == 49
    return b


_CACHE = {}


def _case():
    """The batch and every stage's reference, computed once and never changed."""
    if not _CACHE:
        b = _build()
        _CACHE.update(b=b, pile=_pile_ref(b), perm=perm_ref_batch(b, N_PERM, SEED), rank=rank_ref_batch(b, 1),
                      assign=assign_ref_batch(b, MIN_COV, MIN_CALLS, Q16),
                      tagcheck=tagcheck_ref_batch(b, MIN_COV, MIN_CALLS, Q16))
    return _CACHE


def _pile_sums(win_off, cnt, w):
    """[m1, u1, m2, u2] of window w from the pileup's counters."""
    s0, s1 = int(win_off[w]), int(win_off[w + 1])
    return np.asarray(cnt, np.uint64).reshape(-1, 3, 2)[s0:s1, 0:2, :].sum(axis=0).reshape(4)


def _agree(pile, perm, rank, tag):
    win_off, _, cnt = pile
    W = len(win_off) - 1
    assert W == 4
    for w in range(W):
        ps = _pile_sums(win_off, cnt, w).tolist()
        assert ps == np.asarray(perm["sum"][w], np.uint64).tolist(), f"{tag}: window {w} pileup vs permtest"
        assert ps == np.asarray(rank["sum"][w], np.uint64).tolist(), f"{tag}: window {w} pileup vs ranktest"


def test_references_agree():
    c = _case()
    _agree(c["pile"], c["perm"], c["rank"], "references")
    win_off, pos, cnt = c["pile"]
    assert cnt.max() < 65536
    for w in range(3):
        p = pos[int(win_off[w]):int(win_off[w + 1])].tolist()
        assert WS in p and WE - 1 in p and min(p) >= WS and max(p) < WE
        assert sum(_pile_sums(win_off, cnt, w).tolist()) > 1000
    assert pos[int(win_off[3]):].tolist() == [50] and _pile_sums(win_off, cnt, 3).tolist() == [1, 0, 0, 1]
    # the tests have something to decide: reads on both sides of every stage's line
    assert (c["perm"]["status"][:3] == 0).all() and (c["rank"]["status"][:3] == 0).all()
    assert (np.asarray(c["assign"]["n_used"]) > 0).sum() > 50
    assert (np.asarray(c["tagcheck"]["n_used"]) > 0).sum() > 100


def _acfg():
    c = AssignConfig(min_cov=MIN_COV, min_calls=MIN_CALLS)
    c.min_llr = Q16 / 65536
    assert c.min_llr_q16 == Q16
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True], ids=["default", "64"])
def test_stages_match_references_and_each_other(gpu_ctx, monkeypatch, small):
    if small:
        for name in SMALL:
            monkeypatch.setenv(name, "64")
    c = _case()
    db = gpu_ctx.upload(_cfg(), c["b"])
    try:
        pile = db.pileup()
        perm = db.permtest(N_PERM, seed=SEED)
        rank = db.ranktest(1)
        assign = db.assign(_acfg())
        tagcheck = db.tagcheck(_acfg())
    finally:
        db.free()
    tag = "64" if small else "default"
    pile_same(pile, c["pile"], f"pileup {tag}")
    perm_same(perm, c["perm"], f"permtest {tag}")
    rank_same(rank, c["rank"], f"ranktest {tag}")
    assign_same(assign, c["assign"], f"assign {tag}")
    tagcheck_same(tagcheck, c["tagcheck"], f"tagcheck {tag}")
    _agree((pile["win_off"], pile["pos"], pile["cnt"]), perm, rank, f"device {tag}")
