"""The read-label permutation test on the device (pf_batch_permtest,
pf_perm.hip) against the literal reference tests/_perm_ref.py: hits, status,
n_reads and sum, all integers, every comparison exact.  Hand-built
calls-level batches are their own reference input; the record-level batch's
reference input comes from the CPU loader (oracle load_reads), not from K0.
Every case runs at PF_PERM_THREADS 64 (one wave) and the default.

Not tested: N >= 2^31 calls in one window (PF_ERR_LIMIT) -- it needs two
billion call entries.
"""
import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig

from tests._aln_cases import synth_aln
from tests._perm_ref import perm_ref_batch, same
from tests.test_permtest import KNOWN
from tests.test_pileup_gpu import _calls_batch, _cfg

pytestmark = pytest.mark.gpu

LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)


@pytest.fixture(params=[None, "64"], ids=["default", "t64"])
def threads(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("PF_PERM_THREADS", request.param)
    return request.param


def _read(ws, we, m, u, hp):
    """A read with m meth and u unmeth entries inside [ws, we): positions wrap
    around a short window, so entries repeat there (they count each time)."""
    span = we - ws
    return hp, [(ws + k % span, 0) for k in range(m)] + [(ws + k % span, 1) for k in range(u)]


def _check(ctx, batch, n_perm, seed, tag, hp=None):
    ref = perm_ref_batch(batch, n_perm, seed, hp)
    db = ctx.upload(_cfg(), batch)
    try:
        got = db.permtest(n_perm, seed=seed, read_hp=hp)
    finally:
        db.free()
    same(got, ref, tag)
    assert got["n_perm"] == n_perm and got["seed"] == seed and got["ms"] > 0
    return got


def test_known_answers(gpu_ctx, threads):
    for name, ((m, u, tags, ws, we, n_perm, seed), (hits, status)) in sorted(KNOWN.items()):
        b = _calls_batch([(ws, we, [_read(ws, we, a, c, h) for a, c, h in zip(m, u, tags)])])
        got = _check(gpu_ctx, b, n_perm, seed, name)
        assert (int(got["hits"][0]), int(got["status"][0])) == (hits, status), name
        assert got["n_reads"][0].tolist() == [tags.count(0), tags.count(1)]
        assert int(got["sum"][0].sum()) == sum(m) + sum(u)


@pytest.mark.parametrize("n", [2, 63, 64, 65, 130])
def test_random_counts(gpu_ctx, threads, n):
    """n participating reads around the wave width, random m, u and tags."""
    rng = np.random.default_rng(1000 + n)
    m, u = rng.integers(0, 40, n), rng.integers(0, 40, n)
    m[(m + u) == 0] = 1
    tags = rng.integers(0, 2, n)
    tags[0], tags[-1] = 0, 1
    b = _calls_batch([(100, 1000, [_read(100, 1000, int(a), int(c), int(h)) for a, c, h in zip(m, u, tags)])])
    got = _check(gpu_ctx, b, 200, 7, f"n={n}")
    assert int(got["status"][0]) == 0 and got["n_reads"][0].sum() == n


def test_1024_threads(gpu_ctx, monkeypatch):
    """Sixteen waves: more waves than permutations, and reads over several rounds' worth of waves."""
    monkeypatch.setenv("PF_PERM_THREADS", "1024")
    rng = np.random.default_rng(5)
    reads = [_read(100, 1000, int(a), int(c), int(h))
             for a, c, h in zip(rng.integers(1, 30, 1500), rng.integers(0, 30, 1500), rng.integers(0, 2, 1500))]
    _check(gpu_ctx, _calls_batch([(100, 1000, reads)]), 9, 2, "1024 threads")


@pytest.mark.parametrize("n_perm", [1, 17, 1000])
def test_n_perm(gpu_ctx, threads, n_perm):
    rng = np.random.default_rng(3)
    reads = [_read(0, 500, int(a), int(c), k % 2) for k, (a, c) in enumerate(zip(rng.integers(1, 9, 12), rng.integers(1, 9, 12)))]
    got = _check(gpu_ctx, _calls_batch([(0, 500, reads)]), n_perm, 11, f"n_perm={n_perm}")
    assert int(got["hits"][0]) <= n_perm


def test_who_participates(gpu_ctx, threads):
    """Windows without reads; reads that overlap the window without a call in
    it (they shift i); tags 254 and 3 between tagged reads; cat 2 entries and
    duplicate entries."""
    inside = [(1, [(210, 0), (220, 1)]), (0, [(230, 0), (231, 0), (240, 1)]), (1, [(250, 1), (251, 1)]), (0, [(260, 0)])]
    out_l, out_r, nocall = (0, [(10, 0), (199, 1)]), (1, [(300, 0), (5000, 1)]), (0, [(250, 2)])
    shifted = [out_l, inside[0], nocall, inside[1], out_r, (0, []), inside[2], inside[3]]
    other = [inside[0], (254, [(210, 0)] * 5), inside[1], (3, [(215, 1)] * 7), inside[2], (254, []), inside[3]]
    dup = [(1, [(210, 0), (210, 0), (220, 1), (222, 2)]), (0, [(230, 0), (230, 1), (230, 2), (230, 2)]),
           (1, [(250, 1), (250, 1), (250, 1)]), (0, [(299, 0), (299, 0), (300, 0)])]
    b = _calls_batch([(200, 300, []), (200, 300, inside), (200, 300, shifted), (200, 300, other), (200, 300, dup),
                      (7, 7, [(0, [(7, 0)]), (1, [(7, 1)])]), (200, 300, [nocall, out_l, (254, [(210, 0)])])])
    got = _check(gpu_ctx, b, 300, 1, "participation")
    assert got["n_reads"].tolist() == [[0, 0], [2, 2], [2, 2], [2, 2], [2, 2], [0, 0], [0, 0]]
    assert got["status"].tolist() == [1, 0, 0, 0, 0, 1, 1]
    # the same participating reads in the same order: the same keys, the same hits
    assert int(got["hits"][1]) == int(got["hits"][2]) == int(got["hits"][3])
    assert got["sum"][2].tolist() == got["sum"][1].tolist() == [3, 1, 1, 3]
    assert got["sum"][4].tolist() == [3, 1, 2, 4]


def test_windows_are_independent(gpu_ctx, threads):
    """Two windows with equal coordinates and different reads, two with equal
    reads (equal hits), and an overlapping window."""
    rng = np.random.default_rng(9)

    def reads(k):
        return [_read(50, 400, int(a), int(c), j % 2) for j, (a, c) in enumerate(zip(rng.integers(1, 20, k), rng.integers(1, 20, k)))]
    ra, rb = reads(9), reads(14)
    got = _check(gpu_ctx, _calls_batch([(50, 400, ra), (50, 400, rb), (50, 400, ra), (60, 300, ra)]), 400, 1, "independent")
    assert int(got["hits"][0]) == int(got["hits"][2]) and got["sum"][0].tolist() == got["sum"][2].tolist()
    assert got["sum"][0].tolist() != got["sum"][1].tolist() and got["sum"][3].sum() < got["sum"][0].sum()


def test_read_hp_override(gpu_ctx, threads):
    from pomfret_amd import PomfretError
    rng = np.random.default_rng(21)
    n = 40
    m, u = rng.integers(1, 25, n), rng.integers(1, 25, n)
    own = rng.integers(0, 2, n).astype(np.uint8)
    other = own.copy()
    other[::3] ^= 1
    other[5], other[17] = 254, 3

    def batch(tags):
        return _calls_batch([(0, 2000, [_read(0, 2000, int(a), int(c), int(h)) for a, c, h in zip(m, u, tags)])])
    db = gpu_ctx.upload(_cfg(), batch(own))
    try:
        with_other = db.permtest(250, seed=4, read_hp=other)
        with_own = db.permtest(250, seed=4)              # the batch's own tags are intact afterwards
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.permtest(250, seed=4, read_hp=other[:-1])   # n_hp must be the batch's reads
    finally:
        db.free()
    same(with_other, perm_ref_batch(batch(other), 250, 4), "override")
    same(with_other, perm_ref_batch(batch(own), 250, 4, hp=other), "override, reference override")
    same(with_own, perm_ref_batch(batch(own), 250, 4), "own tags afterwards")
    assert with_other["n_reads"][0].sum() == n - 2 and with_own["n_reads"][0].sum() == n


def test_read_limit(gpu_ctx, threads):
    """4,096 participating reads are tested, 4,097 are not (status 2, no
    error); reads outside the range do not count towards the limit."""
    rng = np.random.default_rng(4096)

    def reads(k):
        return [(int(h), [(100 + j % 50, int(c))]) for j, (h, c) in enumerate(zip(rng.integers(0, 2, k), rng.integers(0, 2, k)))]
    far = [(0, [(5000, 0)])] * 10
    b = _calls_batch([(100, 150, far + reads(4096)), (100, 150, reads(4097)), (100, 150, reads(4096) + [(254, [(120, 0)])])])
    got = _check(gpu_ctx, b, 8, 6, "limit")
    assert got["status"].tolist() == [0, 2, 0] and int(got["hits"][1]) == 0
    assert got["n_reads"].sum(axis=1).tolist() == [4096, 4097, 4096]


def test_bad_arguments(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    db = gpu_ctx.upload(_cfg(), _calls_batch([(0, 10, [(0, [(1, 0)]), (1, [(2, 1)])])]))
    try:
        for n_perm in (0, 1_000_001):
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.permtest(n_perm)
        # the largest n_perm; one read against one: either labelling separates them as far, so every permutation hits
        top = db.permtest(1_000_000)
        assert top["status"].tolist() == [0] and top["hits"].tolist() == [1_000_000]
        for bad in ("128", "0", "2048", "64x", ""):
            monkeypatch.setenv("PF_PERM_THREADS", bad)
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.permtest(5)
        monkeypatch.setenv("PF_PERM_THREADS", "1024")
        assert db.permtest(5)["status"].tolist() == [0]
    finally:
        db.free()


def test_no_windows(gpu_ctx):
    db = gpu_ctx.upload(_cfg(), _calls_batch([]))
    got = db.permtest(5)
    db.free()
    assert got["hits"].size == 0 and got["n_reads"].shape == (0, 2) and got["sum"].shape == (0, 4)


def test_record_level_batch(gpu_ctx, oracle_lib, threads):
    """A record-level batch runs its load stage first; the reference reads
    the CPU loader's calls.  The pileup of the same batch still works after."""
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = perm_ref_batch(ref_b, 40, 1)
    assert ref["status"].tolist() == [0, 0] and ref["n_reads"].min() >= 5
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        got = db.permtest(40)
        again = db.permtest(40)
        pile = db.pileup()
    finally:
        db.free()
    same(got, ref, "record level")
    same(again, ref, "record level, second call")
    assert pile["pos"].size > 0
    # the pooled counts of the window are the pileup's, summed over its sites
    k = int(pile["win_off"][1])
    assert pile["cnt"][:k, :2].reshape(k, 4).sum(axis=0).tolist() == got["sum"][0].tolist()


def test_between_runs_and_in_flight(gpu_ctx, oracle_lib):
    """The test leaves the batch as it was: a run before and after it gives
    the same results, the test after a run the same hits; while a launched run
    is unfinished the call is refused."""
    from pomfret_amd import PomfretError
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = perm_ref_batch(ref_b, 20, 3)
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        res = db.run()
        same(db.permtest(20, seed=3), ref, "after a run")
        res2 = db.run()
        for f in ("decision", "read_hp", "dir_table", "win_n_sites", "win_n_reads"):
            assert np.array_equal(getattr(res, f), getattr(res2, f)), f
        db.launch()
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.permtest(20, seed=3)
        db.finish()
        same(db.permtest(20, seed=3), ref, "after the finish")
    finally:
        db.free()
