"""Tags for untagged reads on the device (pf_batch_assign, pf_assign.hip)
against the literal reference tests/_assign_ref.py: n_used, llr, hp, win_n and
win_read_off, all integers, every comparison exact.  Hand-built calls-level
batches are their own reference input; the record-level batch's reference input
comes from the CPU loader (oracle load_reads), not from K0.  Every case runs at
the default tile (4,096 sites) and at PF_ASSIGN_TILE=64.
"""
import numpy as np
import pytest

from pomfret_amd.abi import AssignConfig, LoadConfig

from tests._aln_cases import synth_aln
from tests._assign_ref import assign_ref_batch, same, weights
from tests._perm_ref import perm_ref_batch
from tests._perm_ref import same as perm_same
from tests.test_pileup_gpu import _calls_batch, _cfg, _pile_ref
from tests.test_pileup_gpu import _same as pile_same

pytestmark = pytest.mark.gpu

LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)


@pytest.fixture(params=[None, "64"], ids=["default", "t64"])
def tile(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("PF_ASSIGN_TILE", request.param)
    return int(request.param or 4096)


def _acfg(min_cov=1, min_calls=1, q16=65536):
    c = AssignConfig(min_cov=min_cov, min_calls=min_calls)
    c.min_llr = q16 / 65536                          # exact: to_c() rounds q16 back
    assert c.min_llr_q16 == q16
    return c


def _check(ctx, batch, tag, min_cov=1, min_calls=1, q16=65536, hp=None):
    ref = assign_ref_batch(batch, min_cov, min_calls, q16, hp)
    db = ctx.upload(_cfg(), batch)
    try:
        got = db.assign(_acfg(min_cov, min_calls, q16), read_hp=hp)
    finally:
        db.free()
    same(got, ref, tag)
    return got


def _tagged(positions, rng, depth=2, p_meth=(0.9, 0.1)):
    """depth reads per haplotype over `positions`: haplotype 1 mostly meth, 2 mostly unmeth."""
    reads = []
    for h in (0, 1):
        for _ in range(depth):
            cat = (rng.random(len(positions)) >= p_meth[h]).astype(int)
            reads.append((h, list(zip(positions, cat.tolist()))))
    return reads


def _cand(positions, rng, k, like=0):
    """An untagged read with k calls at distinct positions, drawn like haplotype `like`."""
    pick = sorted(rng.choice(len(positions), size=k, replace=False).tolist())
    cat = (rng.random(k) >= (0.9, 0.1)[like]).astype(int).tolist()
    return 254, [(positions[i], c) for i, c in zip(pick, cat)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_candidates_per_window(gpu_ctx, tile, n):
    """n candidates around the wave width (each wave takes 64 reads at a time), between tagged reads."""
    rng = np.random.default_rng(100 + n)
    pos = list(range(1000, 1400, 10))
    reads = _tagged(pos, rng, 3) + [_cand(pos, rng, int(rng.integers(1, 20)), j % 2) for j in range(n)]
    order = rng.permutation(len(reads)).tolist()
    got = _check(gpu_ctx, _calls_batch([(1000, 1400, [reads[i] for i in order])]), f"n={n}", min_cov=2, min_calls=2, q16=2 << 16)
    assert int(got["win_n"][0][0]) == n                 # every position is informative


@pytest.mark.parametrize("k", [1, 64, 65, 200])
def test_calls_per_candidate(gpu_ctx, tile, k):
    """k calls in range around the stride of 64 calls, with entries left and right of the window."""
    rng = np.random.default_rng(200 + k)
    pos = list(range(5000, 5000 + 3 * 300, 3))
    outside = [(10, 0), (4999, 1), (5900, 0), (90000, 1)]
    reads = _tagged(pos, rng)
    for like in (0, 1):
        h, calls = _cand(pos, rng, k, like)
        reads.append((h, calls + outside))
    got = _check(gpu_ctx, _calls_batch([(5000, 5900, reads)]), f"k={k}")
    assert got["n_used"][-2:].tolist() == [k, k]


@pytest.mark.parametrize("which", ["1", "tile-1", "tile", "tile+1", "3tile+5"])
def test_sites_per_window(gpu_ctx, tile, which):
    """Informative sites around the LDS tile; the last case has candidates
    whose calls span three and four tiles, and one that lies in the last alone."""
    n = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3tile+5": 3 * tile + 5}[which]
    rng = np.random.default_rng(n)
    pos = (100 + 2 * np.arange(n)).tolist()
    reads = _tagged(pos, rng, 1)
    reads.append((254, [(p, int(c)) for p, c in zip(pos[::7], rng.integers(0, 2, len(pos[::7])))]))       # every tile
    reads.append((254, [(p, 0) for p in pos[tile // 2:2 * tile + 3:5]]))                                  # tiles 0 .. 2
    reads.append((254, [(p, 1) for p in pos[-3:]]))                                                       # the last tile
    reads.append((254, [(pos[0], 0), (pos[-1], 1)]))                                                      # first and last site
    reads.append((254, [(p + 1, 0) for p in pos[::3]]))                                                   # between the sites
    got = _check(gpu_ctx, _calls_batch([(100, 100 + 2 * n, reads)]), which)
    assert int(got["n_used"][2]) == len(pos[::7]) and int(got["n_used"][-1]) == 0
    assert int(got["n_used"][-2]) == 2                  # one site: the same position twice


def _seven(rng):
    pos = list(range(200, 300, 4))
    a = _tagged(pos, rng, 2) + [_cand(pos, rng, 9, 0), _cand(pos, rng, 9, 1)]
    b = _tagged(pos, rng, 3) + [_cand(pos, rng, 5, 1), _cand(pos, rng, 25, 0), _cand(pos, rng, 1, 0)]
    return [(200, 300, a),
            (200, 300, [_cand(pos, rng, 7, 0), _cand(pos, rng, 3, 1)]),                 # no tagged read
            (200, 300, [(0, [(p, 0) for p in pos]), (0, [(p, 1) for p in pos]), _cand(pos, rng, 7, 0)]),   # one haplotype: no informative site
            (200, 300, b),                                                             # equal coordinates, other reads
            (200, 300, []),                                                            # no read
            (250, 270, a),                                                             # a sub-range of the same reads
            (7, 7, [(0, [(7, 0)]), (1, [(7, 1)]), (254, [(7, 0)])])]                    # an empty range


@pytest.mark.parametrize("n_windows", [0, 1, 7])
def test_windows(gpu_ctx, tile, n_windows):
    rng = np.random.default_rng(7)
    wins = _seven(rng)[:n_windows]
    b = _calls_batch(wins)
    db = gpu_ctx.upload(_cfg(), b)
    try:
        got = db.assign(_acfg(min_cov=2))
    finally:
        db.free()
    if n_windows == 0:
        assert got["win_n"].shape == (0, 3) and got["hp"].size == 0 and got["n_used"].size == 0 and got["llr"].size == 0
        assert got["win_read_off"].tolist() == [0]
        return
    same(got, assign_ref_batch(b, 2, 1, 65536), f"{n_windows} windows")
    assert got["ms"] > 0
    if n_windows == 7:
        assert got["win_n"][[1, 2, 4, 6]].sum() == 0 and got["win_n"][0][0] == 2 and got["win_n"][3][0] == 3
        assert got["win_n"][5][0] >= 1


def test_who_counts(gpu_ctx, tile):
    """Tags 3 and 254 mixed between tagged reads: a tag-3 read neither enters
    the model nor is a candidate; cat 2 entries and non-informative positions
    count nowhere; a duplicate entry counts each time; entries left and right
    of the range; a candidate that overlaps the window with no call in it."""
    tagged = [(0, [(210, 0), (220, 0), (230, 1)]), (1, [(210, 1), (220, 1), (230, 0)]),
              (0, [(210, 0), (220, 0), (230, 1), (240, 0)]), (1, [(210, 1), (220, 1), (230, 0)])]
    reads = [tagged[0], (254, [(210, 0), (210, 0), (220, 2), (230, 1)]), (3, [(210, 1)] * 9), tagged[1],
             (254, [(100, 0), (199, 1), (300, 0), (5000, 1)]), (254, []), tagged[2], (3, [(220, 1), (230, 0)]),
             (254, [(240, 0), (240, 1), (215, 0)]),                  # 240: haplotype 1 alone; 215: no site
             (254, [(199, 0), (210, 1), (220, 1), (230, 0), (230, 0), (300, 1)]), tagged[3]]
    got = _check(gpu_ctx, _calls_batch([(200, 300, reads)]), "who counts", min_cov=2, min_calls=1, q16=1)
    wm, wu = weights(2, 0, 0, 2)
    assert got["n_used"].tolist() == [0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 0]
    assert got["llr"].tolist() == [0, 3 * wm, 0, 0, 0, 0, 0, 0, 0, 4 * wu, 0]
    assert got["hp"].tolist() == [0, 0, 3, 1, 254, 254, 0, 3, 254, 1, 1]
    assert got["win_n"].tolist() == [[2, 1, 1]]


def test_thresholds(gpu_ctx, tile):
    """S == min_llr_q16 is assigned, S == min_llr_q16 - 1 is not; S == 0 never,
    whatever the threshold; n_used == min_calls - 1 is not."""
    from tests.test_assign import _one_window
    sites = {110: (5, 0, 0, 5), 120: (3, 3, 3, 3)}
    L6 = 169408

    def run(calls, min_calls, q16):
        got = _check(gpu_ctx, _one_window(sites, calls), f"{calls} {min_calls} {q16}", min_cov=3, min_calls=min_calls, q16=q16)
        return int(got["llr"][-1]), int(got["n_used"][-1]), int(got["hp"][-1])
    assert run([(110, 0)], 1, L6) == (L6, 1, 0)
    assert run([(110, 0)], 1, L6 + 1) == (L6, 1, 254)
    assert run([(110, 1)], 1, L6) == (-L6, 1, 1)
    assert run([(110, 1)], 1, L6 + 1) == (-L6, 1, 254)
    for q16 in (1, 0, -5):
        assert run([(120, 0), (120, 1)], 1, q16) == (0, 2, 254)
        assert run([(110, 0), (110, 1)], 1, q16) == (0, 2, 254)
    assert run([(110, 0)], 2, 1) == (L6, 1, 254)
    assert run([(110, 0), (120, 1)], 2, 1) == (L6, 2, 0)
    assert run([(110, 1), (110, 1)], 2, 2 * L6) == (-2 * L6, 2, 1)


def _override_case():
    rng = np.random.default_rng(21)
    pos = list(range(0, 2000, 20))
    reads = _tagged(pos, rng, 6) + [_cand(pos, rng, 12, j % 2) for j in range(10)]
    own = np.asarray([h for h, _ in reads], np.uint8)
    other = own.copy()
    other[[0, 7]] = 254                              # two tagged reads hidden: candidates now, out of the model
    other[[12, 13]] = [0, 1]                         # two untagged reads tagged: in the model, no candidates
    other[14], other[3] = 3, 3
    return reads, own, other


def test_read_hp_override_and_pileup(gpu_ctx, tile):
    """Results under an override equal the reference under it; the batch's own
    tags are intact afterwards; a wrong n_hp is refused; the pileup under the
    result's tags moves exactly the assigned reads' counts out of "other"."""
    from pomfret_amd import PomfretError
    reads, own, other = _override_case()
    b = _calls_batch([(0, 2000, reads)])
    cfg = _acfg(min_cov=3, min_calls=2, q16=2 << 16)
    db = gpu_ctx.upload(_cfg(), b)
    try:
        with_other = db.assign(cfg, read_hp=other)
        with_own = db.assign(cfg)
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.assign(cfg, read_hp=other[:-1])
        pile0 = db.pileup()
        pile1 = db.pileup(read_hp=with_own["hp"])
    finally:
        db.free()
    same(with_other, assign_ref_batch(b, 3, 2, 2 << 16, hp=other), "override")
    ref = assign_ref_batch(b, 3, 2, 2 << 16)
    same(with_own, ref, "own tags afterwards")
    assert with_other["n_used"][[0, 7]].min() > 0 and not with_other["n_used"][[12, 13, 14]].any()
    assert with_other["hp"][[3, 14, 12, 13]].tolist() == [3, 3, 0, 1]
    pile_same(pile0, _pile_ref(b), "pileup, own tags")
    pile_same(pile1, _pile_ref(b, hp=ref["hp"]), "pileup, assigned tags")
    moved = np.flatnonzero(ref["hp"] != own)
    assert moved.size >= 4 and set(ref["hp"][moved].tolist()) == {0, 1}
    calls = sum(len(reads[r][1]) for r in moved)     # every call is in range, cat 0 / 1
    assert int(pile0["cnt"][:, 2].sum()) - int(pile1["cnt"][:, 2].sum()) == calls
    assert np.array_equal(pile0["cnt"].sum(axis=1), pile1["cnt"].sum(axis=1))
    stay = sum(len(reads[r][1]) for r in np.flatnonzero(ref["hp"] == 254))
    assert int(pile1["cnt"][:, 2].sum()) == stay


def test_record_level_batch(gpu_ctx, oracle_lib, tile):
    """A record-level batch runs its load stage first; the reference reads the CPU loader's calls."""
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = assign_ref_batch(ref_b, 3, 2, 2 << 16)
    assert ref["win_n"][:, 0].min() >= 5 and ref["win_n"][:, 1:].sum() >= 5
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        cfg = _acfg(min_cov=3, min_calls=2, q16=2 << 16)
        got = db.assign(cfg)
        again = db.assign(cfg)
    finally:
        db.free()
    same(got, ref, "record level")
    same(again, ref, "record level, second call")


def test_between_runs_and_in_flight(gpu_ctx, oracle_lib):
    """The call leaves the batch as it was: a run before and after it gives
    the same results, the permutation test and the pileup still equal their
    references afterwards; while a launched run is unfinished it is refused."""
    from pomfret_amd import PomfretError
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = assign_ref_batch(ref_b, 3, 1, 65536)
    cfg = _acfg(min_cov=3)
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        res = db.run()
        same(db.assign(cfg), ref, "after a run")
        res2 = db.run()
        for f in ("decision", "read_hp", "dir_table", "win_n_sites", "win_n_reads"):
            assert np.array_equal(getattr(res, f), getattr(res2, f)), f
        perm_same(db.permtest(20, seed=3), perm_ref_batch(ref_b, 20, 3), "permtest afterwards")
        pile_same(db.pileup(), _pile_ref(ref_b), "pileup afterwards")
        db.launch()
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.assign(cfg)
        db.finish()
        same(db.assign(cfg), ref, "after the finish")
    finally:
        db.free()


def test_bad_tile_values(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    b = _calls_batch([(0, 10, [(0, [(1, 0)]), (1, [(1, 1)]), (254, [(1, 0)])])])
    db = gpu_ctx.upload(_cfg(), b)
    try:
        for bad in ("0", "32", "8192", "64x", "", "100"):
            monkeypatch.setenv("PF_ASSIGN_TILE", bad)
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.assign(_acfg())
        for ok in ("64", "256", "4096"):
            monkeypatch.setenv("PF_ASSIGN_TILE", ok)
            same(db.assign(_acfg()), assign_ref_batch(b, 1, 1, 65536), ok)
    finally:
        db.free()
