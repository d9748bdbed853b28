"""The leave-one-out tag check on the device (pf_batch_tagcheck,
pf_tagcheck.hip) against the literal reference tests/_tagcheck_ref.py: n_used,
llr, verdict, hp, win_n and win_read_off, all integers, every comparison exact.
Hand-built calls-level batches are their own reference input; the record-level
batch's reference input comes from the CPU loader (oracle load_reads), not from
K0.  Every case runs at the default tile (2,048 sites) and at
PF_TAGCHECK_TILE=64.
"""
import numpy as np
import pytest

from pomfret_amd.abi import AssignConfig, LoadConfig

from tests._aln_cases import synth_aln
from tests._assign_ref import assign_ref_batch
from tests._assign_ref import same as assign_same
from tests._tagcheck_ref import FLIP, NOT_SCORED, OK, UNDECIDED, entry_weight, same, tagcheck_ref_batch
from tests.test_pileup_gpu import _calls_batch, _cfg

pytestmark = pytest.mark.gpu

LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)
DEFAULT_TILE = 2048


@pytest.fixture(params=[None, "64"], ids=["default", "t64"])
def tile(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("PF_TAGCHECK_TILE", request.param)
    return int(request.param or DEFAULT_TILE)


def _acfg(min_cov=1, min_calls=1, q16=65536):
    c = AssignConfig(min_cov=min_cov, min_calls=min_calls)
    c.min_llr = q16 / 65536                          # exact: to_c() rounds q16 back
    assert c.min_llr_q16 == q16
    return c


def _check(ctx, batch, tag, min_cov=1, min_calls=1, q16=65536, hp=None):
    ref = tagcheck_ref_batch(batch, min_cov, min_calls, q16, hp)
    db = ctx.upload(_cfg(), batch)
    try:
        got = db.tagcheck(_acfg(min_cov, min_calls, q16), read_hp=hp)
    finally:
        db.free()
    same(got, ref, tag)
    return got


def _read(positions, rng, k, h, like=None, p_meth=(0.9, 0.1)):
    """A read tagged h with k calls at distinct positions, drawn like haplotype `like` (h itself by default)."""
    pick = sorted(rng.choice(len(positions), size=k, replace=False).tolist())
    cat = (rng.random(k) >= p_meth[like if like is not None else h if h < 2 else 0]).astype(int).tolist()
    return h, [(positions[i], c) for i, c in zip(pick, cat)]


def _full(positions, rng, depth=2, p_meth=(0.9, 0.1)):
    """depth reads per haplotype with a call at every position."""
    return [_read(positions, rng, len(positions), h, p_meth=p_meth) for h in (0, 1) for _ in range(depth)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_tagged_reads_per_window(gpu_ctx, tile, n):
    """n more tagged reads around the wave width, with untagged (254) and tag-3
    reads between them: those come back 255 and zeros."""
    rng = np.random.default_rng(100 + n)
    pos = list(range(1000, 1400, 10))
    reads = _full(pos, rng, 3) + [_read(pos, rng, int(rng.integers(1, 20)), j % 2) for j in range(n)]
    reads += [_read(pos, rng, 9, 254), _read(pos, rng, 5, 3), _read(pos, rng, 40, 254)]
    order = rng.permutation(len(reads)).tolist()
    reads = [reads[i] for i in order]
    got = _check(gpu_ctx, _calls_batch([(1000, 1400, reads)]), f"n={n}", min_cov=2, min_calls=2, q16=2 << 16)
    other = np.asarray([h > 1 for h, _ in reads])
    assert (got["verdict"][other] == NOT_SCORED).all() and not got["n_used"][other].any() and not got["llr"][other].any()
    assert int(got["win_n"][0, :, 0].sum()) == n + 6 and int(got["win_n"][0, :, 1].sum()) == n + 6


@pytest.mark.parametrize("k", [1, 64, 65, 200])
def test_calls_per_read(gpu_ctx, tile, k):
    """k calls in range around the stride of 64 calls, with entries left and right of the window."""
    rng = np.random.default_rng(200 + k)
    pos = list(range(5000, 5000 + 3 * 300, 3))
    outside = [(10, 0), (4999, 1), (5900, 0), (90000, 1)]
    reads = _full(pos, rng)
    for h in (0, 1):
        _, calls = _read(pos, rng, k, h)
        reads.append((h, calls + outside))
    got = _check(gpu_ctx, _calls_batch([(5000, 5900, reads)]), f"k={k}")
    assert got["n_used"][-2:].tolist() == [k, k]


@pytest.mark.parametrize("which", ["1", "tile-1", "tile", "tile+1", "3tile+5"])
def test_sites_per_window(gpu_ctx, tile, which):
    """Exactly 1, tile-1, tile, tile+1 and 3*tile+5 sites in the window (the
    pileup's own count is asserted); reads that span every tile, three of them,
    lie in the last alone, touch only the first and the last site, or fall
    between the sites.  Any cat 0 / 1 entry makes its position a site, so the
    entries between the sites are no-calls (cat 2): the read still hits every
    tile, its calls are looked at and count nowhere; its one real call sits on
    a site the other reads made."""
    n = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3tile+5": 3 * tile + 5}[which]
    rng = np.random.default_rng(n)
    pos = (100 + 2 * np.arange(n)).tolist()
    reads = _full(pos, rng, 2)
    reads.append((0, [(p, int(c)) for p, c in zip(pos[::7], rng.integers(0, 2, len(pos[::7])))]))       # every tile
    reads.append((1, [(p, 0) for p in pos[tile // 2:2 * tile + 3:5]]))                                  # tiles 0 .. 2
    reads.append((0, [(p, 1) for p in pos[-3:]]))                                                       # the last tile
    reads.append((1, [(pos[0], 0), (pos[-1], 1)]))                                                      # first and last site
    reads.append((1, [(p + 1, 2) for p in pos[::3]] + [(pos[n // 2], 0)]))                              # between the sites
    b = _calls_batch([(100, 101 + 2 * n, reads)])
    ref = tagcheck_ref_batch(b, 1, 1, 65536)
    db = gpu_ctx.upload(_cfg(), b)
    try:
        sites = db.pileup()["win_off"].tolist()
        got = db.tagcheck(_acfg())
    finally:
        db.free()
    assert sites == [0, n]                              # the window holds exactly the named number of sites
    same(got, ref, which)
    assert int(got["n_used"][4]) == len(pos[::7]) and int(got["n_used"][-2]) == 2
    assert int(got["n_used"][-1]) == 1 and int(got["verdict"][-1]) != NOT_SCORED


def test_only_read_of_its_haplotype(gpu_ctx, tile):
    """min_cov 1: the only read of haplotype 2 cannot be scored -- with its
    entry gone its sites hold no call of haplotype 2 -- while self-scoring
    would have scored it; the haplotype-1 reads are scored against it."""
    pos = list(range(300, 400, 10))
    reads = [(0, [(p, 0) for p in pos]), (0, [(p, 0) for p in pos]), (1, [(p, 1) for p in pos])]
    b = _calls_batch([(300, 400, reads)])
    got = _check(gpu_ctx, b, "only read", min_cov=1, min_calls=1, q16=1)
    assert got["n_used"].tolist() == [10, 10, 0] and got["verdict"].tolist() == [OK, OK, NOT_SCORED]
    assert got["win_n"].tolist() == [[[2, 2, 2, 0], [1, 0, 0, 0]]]
    naive = tagcheck_ref_batch(b, 1, 1, 1, self_scoring=True)
    assert naive["n_used"].tolist() == [10, 10, 10] and naive["verdict"].tolist() == [OK, OK, OK]


@pytest.mark.parametrize("h", [0, 1])
def test_min_cov_boundary(gpu_ctx, tile, h):
    """n_h - 1 == min_cov - 1 against == min_cov, on each haplotype: with
    min_cov 3, three reads of haplotype h leave two (not usable for them, usable
    for the other haplotype's reads), four leave three."""
    pos = [500, 510, 520]
    for depth, usable in ((3, False), (4, True)):
        reads = [(h, [(p, h) for p in pos]) for _ in range(depth)] + [(1 - h, [(p, 1 - h) for p in pos]) for _ in range(5)]
        got = _check(gpu_ctx, _calls_batch([(500, 530, reads)]), f"depth {depth}", min_cov=3, min_calls=1, q16=1)
        assert got["n_used"][:depth].tolist() == [3 if usable else 0] * depth
        assert got["n_used"][depth:].tolist() == [3] * 5
        assert (got["verdict"][:depth] == (OK if usable else NOT_SCORED)).all() and (got["verdict"][depth:] == OK).all()


def test_duplicate_entries_and_count_of_one(gpu_ctx, tile):
    """The same position twice on one read, same and different category: each
    entry is scored with one entry removed, the read's other entry stays in the
    model.  Position 640 holds exactly one meth call of haplotype 1: L(1) = 0."""
    base = [(0, [(600, 0), (610, 0), (620, 1), (640, 1)]), (0, [(600, 0), (610, 1), (620, 0), (640, 1)]),
            (1, [(600, 1), (610, 1), (620, 0), (640, 0)]), (1, [(600, 1), (610, 0), (620, 1), (640, 1)])]
    dup = [(0, [(600, 0), (600, 0), (610, 0), (610, 1), (630, 2), (640, 0)]), (1, [(620, 1), (620, 1), (620, 0), (600, 0)])]
    b = _calls_batch([(600, 700, base + dup)])
    got = _check(gpu_ctx, b, "duplicates", min_cov=1, min_calls=1, q16=1)
    assert got["n_used"][-2:].tolist() == [5, 4]        # cat 2 counts nowhere
    # 600 holds m1 = 4 (two of them this read's), u2 = 2, m2 = 1: either duplicate sees the other one still there
    w600 = entry_weight([4, 0, 1, 2], 0, 0, 1)
    w610 = entry_weight([2, 2, 1, 1], 0, 0, 1) + entry_weight([2, 2, 1, 1], 0, 1, 1)
    w640 = entry_weight([1, 2, 1, 1], 0, 0, 1)          # m1 = 1: L(m1' + 1) = L(1) = 0
    assert int(got["llr"][-2]) == 2 * w600 + w610 + w640


def test_flipped_read(gpu_ctx, tile):
    """A strongly allele-specific window with one read's tag swapped through
    read_hp: that read flips, the others stay ok; under the batch's own tags
    every read is ok."""
    rng = np.random.default_rng(5)
    pos = list(range(0, 600, 10))
    reads = _full(pos, rng, 8, p_meth=(0.95, 0.05))
    b = _calls_batch([(0, 600, reads)])
    own = np.asarray([h for h, _ in reads], np.uint8)
    swapped = own.copy()
    swapped[3] = 1 - own[3]
    got_own = _check(gpu_ctx, b, "own tags", min_cov=3, min_calls=2, q16=3 << 16)
    got = _check(gpu_ctx, b, "one swapped", min_cov=3, min_calls=2, q16=3 << 16, hp=swapped)
    assert (got_own["verdict"] == OK).all() and np.array_equal(got_own["hp"], own)
    assert int(got["verdict"][3]) == FLIP and (np.delete(got["verdict"], 3) == OK).all()
    assert np.array_equal(got["hp"], swapped) and int(got["win_n"][0, int(swapped[3]), 3]) == 1


def _seven(rng):
    pos = list(range(200, 300, 4))
    a = _full(pos, rng, 3) + [_read(pos, rng, 9, 0), _read(pos, rng, 9, 254), _read(pos, rng, 9, 1, like=0)]
    b = _full(pos, rng, 4) + [_read(pos, rng, 5, 1), _read(pos, rng, 25, 0), _read(pos, rng, 1, 0)]
    return [(200, 300, a),
            (200, 300, [_read(pos, rng, 7, 254), _read(pos, rng, 3, 3)]),              # no tagged read
            (200, 300, [(0, [(p, 0) for p in pos]), (0, [(p, 1) for p in pos]), _read(pos, rng, 7, 254)]),   # one haplotype only
            (200, 300, b),                                                             # equal coordinates, other reads
            (200, 300, []),                                                            # no read
            (250, 270, a),                                                             # a sub-range of the same reads
            (7, 7, [(0, [(7, 0)]), (1, [(7, 1)]), (0, [(7, 0)])])]                      # an empty range


@pytest.mark.parametrize("n_windows", [0, 1, 7])
def test_windows(gpu_ctx, tile, n_windows):
    rng = np.random.default_rng(7)
    wins = _seven(rng)[:n_windows]
    b = _calls_batch(wins)
    db = gpu_ctx.upload(_cfg(), b)
    try:
        got = db.tagcheck(_acfg(min_cov=2))
    finally:
        db.free()
    if n_windows == 0:
        assert got["win_n"].shape == (0, 2, 4) and got["verdict"].size == 0 and got["n_used"].size == 0 and got["llr"].size == 0
        assert got["win_read_off"].tolist() == [0] and got["hp"].size == 0
        return
    same(got, tagcheck_ref_batch(b, 2, 1, 65536), f"{n_windows} windows")
    assert got["ms"] > 0
    if n_windows == 7:
        assert got["win_n"][[1, 4]].sum() == 0
        assert got["win_n"][2].tolist() == [[2, 0, 0, 0], [0, 0, 0, 0]] and got["win_n"][6].tolist() == [[2, 0, 0, 0], [1, 0, 0, 0]]
        assert got["win_n"][0, :, 0].tolist() == [4, 4] and got["win_n"][0, :, 1].tolist() == [4, 4]
        assert got["win_n"][3, :, 1].sum() == 11 and got["win_n"][5, :, 1].sum() >= 6


def test_read_hp_override(gpu_ctx, tile):
    """Results under the caller's tags equal the reference under them; the
    batch's own tags are intact afterwards; a wrong n_hp is refused."""
    from pomfret_amd import PomfretError
    rng = np.random.default_rng(21)
    pos = list(range(0, 2000, 20))
    reads = _full(pos, rng, 6) + [_read(pos, rng, 12, (0, 1, 254)[j % 3]) for j in range(12)]
    own = np.asarray([h for h, _ in reads], np.uint8)
    other = own.copy()
    other[[0, 7]] = 254                              # two tagged reads hidden: out of the model, not scored
    other[[14, 17]] = [0, 1]                         # two untagged reads tagged: in the model, scored
    other[3] = 3
    b = _calls_batch([(0, 2000, reads)])
    cfg = _acfg(min_cov=3, min_calls=2, q16=2 << 16)
    db = gpu_ctx.upload(_cfg(), b)
    try:
        with_other = db.tagcheck(cfg, read_hp=other)
        with_own = db.tagcheck(cfg)
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.tagcheck(cfg, read_hp=other[:-1])
    finally:
        db.free()
    same(with_other, tagcheck_ref_batch(b, 3, 2, 2 << 16, hp=other), "override")
    same(with_own, tagcheck_ref_batch(b, 3, 2, 2 << 16), "own tags afterwards")
    assert (with_other["verdict"][[0, 7, 3]] == NOT_SCORED).all() and with_other["n_used"][[14, 17]].min() > 0
    assert (with_own["verdict"][[14, 17]] == NOT_SCORED).all() and with_own["n_used"][[0, 7, 3]].min() > 0


def test_record_level_batch_and_assign_around_it(gpu_ctx, oracle_lib, tile):
    """A record-level batch (16 windows) runs its load stage first; the
    reference reads the CPU loader's calls.  assign before and after the call
    returns identical arrays: the call leaves the batch as it was."""
    aln = synth_aln(16, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = tagcheck_ref_batch(ref_b, 3, 2, 2 << 16)
    assert ref_b.n_windows == 16 and ref["win_n"][:, :, 1].min() >= 5
    kinds = [int((ref["verdict"] == v).sum()) for v in (OK, FLIP, UNDECIDED, NOT_SCORED)]
    assert min(kinds) >= 1, kinds
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        cfg = _acfg(min_cov=3, min_calls=2, q16=2 << 16)
        before = db.assign(cfg)
        got = db.tagcheck(cfg)
        again = db.tagcheck(cfg)
        after = db.assign(cfg)
    finally:
        db.free()
    same(got, ref, "record level")
    same(again, ref, "record level, second call")
    assign_same(before, assign_ref_batch(ref_b, 3, 2, 2 << 16), "assign before")
    assign_same(after, before, "assign after")


def test_bad_tile_values(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    b = _calls_batch([(0, 10, [(0, [(1, 0)]), (0, [(1, 0)]), (1, [(1, 1)]), (1, [(1, 1)]), (254, [(1, 0)])])])
    db = gpu_ctx.upload(_cfg(), b)
    try:
        for bad in ("0", "32", "4096", "64x", "", "100"):
            monkeypatch.setenv("PF_TAGCHECK_TILE", bad)
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.tagcheck(_acfg())
        for ok in ("64", "256", "2048"):
            monkeypatch.setenv("PF_TAGCHECK_TILE", ok)
            same(db.tagcheck(_acfg()), tagcheck_ref_batch(b, 1, 1, 65536), ok)
    finally:
        db.free()
