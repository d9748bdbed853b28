"""The read-level rank-sum test on the device (pf_batch_ranktest, pf_rank.hip)
against the literal reference tests/_rank_ref.py: n_reads, n_short, cls, sum,
u2, ties and status, all integers, every comparison exact.  Hand-built
calls-level batches are their own reference input; the record-level batch's
reference input comes from the CPU loader (oracle load_reads), not from K0.
Every case runs at PF_RANK_THREADS 64 (one wave) and the default, and with
PF_RANK_WIDE unset (the kernel chooses 32-bit or 64-bit products per window)
and 1 (64-bit products everywhere).

Not tested: N >= 2^31 calls in one window (PF_ERR_LIMIT) -- it needs two
billion call entries.
"""
import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig

from tests._aln_cases import synth_aln
from tests._rank_ref import rank_ref_batch, same
from tests.test_permtest_gpu import _read
from tests.test_pileup_gpu import _calls_batch, _cfg
from tests.test_ranktest import KNOWN

pytestmark = pytest.mark.gpu

LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)


@pytest.fixture(params=[(None, None), ("64", None), (None, "1"), ("64", "1")], ids=["default", "t64", "wide", "t64-wide"])
def geom(request, monkeypatch):
    threads, wide = request.param
    if threads:
        monkeypatch.setenv("PF_RANK_THREADS", threads)
    if wide:
        monkeypatch.setenv("PF_RANK_WIDE", wide)
    return request.param


def _window(ws, we, m, u, tags):
    return ws, we, [_read(ws, we, int(a), int(c), int(h)) for a, c, h in zip(m, u, tags)]


def _check(ctx, batch, min_calls, tag, hp=None, ref=None):
    ref = rank_ref_batch(batch, min_calls, hp) if ref is None else ref
    db = ctx.upload(_cfg(), batch)
    try:
        got = db.ranktest(min_calls, read_hp=hp)
    finally:
        db.free()
    same(got, ref, tag)
    assert got["min_calls"] == min_calls and got["ms"] > 0
    return got


def test_known_answers(gpu_ctx, geom):
    for name, ((m, u, tags, mc), (nr, ns, cls, u2, ties, status)) in sorted(KNOWN.items()):
        got = _check(gpu_ctx, _calls_batch([_window(5, 900, m, u, tags)]), mc, name)
        assert (got["n_reads"][0].tolist(), got["n_short"][0].tolist(), got["cls"][0].tolist()) == (nr, ns, cls), name
        assert (int(got["u2"][0]), int(got["ties"][0]), int(got["status"][0])) == (u2, ties, status), name


_RANDOM = {}


def _random_case(n):
    """One batch and its reference per n, shared by the four geometries."""
    if n not in _RANDOM:
        rng = np.random.default_rng(2000 + n)
        m, u = rng.integers(0, 41, n), rng.integers(0, 41, n)
        m[(m + u) == 0] = 1
        tags = rng.integers(0, 2, n)
        tags[0], tags[-1] = 0, 1
        b = _calls_batch([_window(100, 1000, m, u, tags)])
        _RANDOM[n] = (b, rank_ref_batch(b, 1))
    return _RANDOM[n]


@pytest.mark.parametrize("n", [2, 63, 64, 65, 130, 257, 300])
def test_random_counts(gpu_ctx, geom, n):
    """n counted reads around the wave and workgroup widths, m and u in 0 .. 40: many ties."""
    b, ref = _random_case(n)
    got = _check(gpu_ctx, b, 1, f"n={n}", ref=ref)
    assert int(got["status"][0]) == 0 and got["n_reads"][0].sum() == n and (n < 63 or int(got["ties"][0]) > 0)


def test_equal_fractions_different_denominators(gpu_ctx, geom):
    """1/2, 2/4, 3/6 and 50/100 are one tie group across both haplotypes, beside 1/3 and 2/3."""
    m, u, tags = [1, 2, 3, 50, 1, 2, 2, 40], [1, 2, 3, 50, 2, 1, 4, 20], [0, 1, 0, 1, 0, 1, 1, 0]
    got = _check(gpu_ctx, _calls_batch([_window(0, 400, m, u, tags)]), 1, "denominators")
    # groups: {1/2 x 4}, {1/3 x 2}, {2/3 x 2}: 60 + 6 + 6
    assert int(got["ties"][0]) == 72 and int(got["status"][0]) == 0


def test_product_edge(gpu_ctx, geom):
    """n_i = m_i = 65,535 is the last size of the 32-bit products (65,535^2 =
    4,294,836,225); one read of 70,000 entries makes the kernel take the 64-bit
    ones for its window.  Both equal the reference, forced wide or not."""
    big = 65535
    narrow = [(0, [(10 + k % 90, 0) for k in range(big)]), (1, [(10 + k % 90, 0) for k in range(big - 1)] + [(50, 1)]),
              (1, [(10 + k % 90, 0) for k in range(big)]), (0, [(20, 0), (21, 1)]), (1, [(30, 1)] * 3)]
    wide = [(0, [(10 + k % 90, k % 2) for k in range(70000)]), (1, [(10 + k % 90, 0) for k in range(big)]),
            (0, [(15, 0), (16, 1)]), (1, [(40, 0)] + [(41, 1)] * 3), (0, [(42, 1)] * 4)]
    got = _check(gpu_ctx, _calls_batch([(10, 100, narrow), (10, 100, wide)]), 1, "product edge")
    assert got["status"].tolist() == [0, 0] and got["n_reads"].tolist() == [[2, 3], [3, 2]]
    assert int(got["sum"][0][0]) == big + 1 and int(got["sum"][1].sum()) == 70000 + big + 10
    # narrow window: 65535/65535 ties 65535/65535 across the haplotypes, beats 65534/65535, 1/2 and 0/3
    assert int(got["u2"][0]) == 2 * (2 + 1) + 1 and int(got["ties"][0]) == 6
    # wide window: 35000/70000 and 1/2 beat 1/4 and lose to 65535/65535; 0/4 beats nothing
    assert int(got["u2"][1]) == 2 * (1 + 1 + 0) and int(got["ties"][1]) == 6


@pytest.mark.parametrize("min_calls", [1, 2, 3])
def test_who_participates(gpu_ctx, geom, min_calls):
    """The permutation test's participation cases -- windows without reads,
    reads that overlap the window without a call in it, tags 254 and 3 between
    tagged reads, cat 2 and duplicate entries, an empty and a zero-width window
    -- at three values of min_calls for n_short."""
    inside = [(1, [(210, 0), (220, 1)]), (0, [(230, 0), (231, 0), (240, 1)]), (1, [(250, 1), (251, 1)]), (0, [(260, 0)])]
    out_l, out_r, nocall = (0, [(10, 0), (199, 1)]), (1, [(300, 0), (5000, 1)]), (0, [(250, 2)])
    shifted = [out_l, inside[0], nocall, inside[1], out_r, (0, []), inside[2], inside[3]]
    other = [inside[0], (254, [(210, 0)] * 5), inside[1], (3, [(215, 1)] * 7), inside[2], (254, []), inside[3]]
    dup = [(1, [(210, 0), (210, 0), (220, 1), (222, 2)]), (0, [(230, 0), (230, 1), (230, 2), (230, 2)]),
           (1, [(250, 1), (250, 1), (250, 1)]), (0, [(299, 0), (299, 0), (300, 0)])]
    b = _calls_batch([(200, 300, []), (200, 300, inside), (200, 300, shifted), (200, 300, other), (200, 300, dup),
                      (7, 7, [(0, [(7, 0)]), (1, [(7, 1)])]), (200, 300, [nocall, out_l, (254, [(210, 0)])])])
    got = _check(gpu_ctx, b, min_calls, f"participation, min_calls {min_calls}")
    part = [[0, 0], [2, 2], [2, 2], [2, 2], [2, 2], [0, 0], [0, 0]]
    assert (got["n_reads"] + got["n_short"]).tolist() == part
    exp = {1: ([[0, 0]] * 7, [1, 0, 0, 0, 0, 1, 1]),
           2: ([[0, 0], [1, 0], [1, 0], [1, 0], [0, 0], [0, 0], [0, 0]], [1, 0, 0, 0, 0, 1, 1]),
           3: ([[0, 0], [1, 2], [1, 2], [1, 2], [2, 0], [0, 0], [0, 0]], [1, 1, 1, 1, 1, 1, 1])}[min_calls]
    assert got["n_short"].tolist() == exp[0] and got["status"].tolist() == exp[1]
    for k in ("u2", "ties", "sum", "cls"):                   # the same counted reads in the same order
        assert got[k][1].tolist() == got[k][2].tolist() == got[k][3].tolist(), k
    if min_calls == 1:
        assert got["sum"][1].tolist() == [3, 1, 1, 3] and got["sum"][4].tolist() == [3, 1, 2, 4]
    if min_calls == 3:                                       # status 1: min_calls removes a haplotype
        assert got["n_reads"][1].tolist() == [1, 0] and int(got["u2"][1]) == 0 and int(got["ties"][1]) == 0


def test_all_reads_tied(gpu_ctx, geom):
    n = 70
    m, u, tags = [k % 7 + 1 for k in range(n)], [2 * (k % 7 + 1) for k in range(n)], [k % 2 for k in range(n)]
    got = _check(gpu_ctx, _calls_batch([_window(0, 50, m, u, tags)]), 1, "tied")
    assert int(got["u2"][0]) == 35 * 35 and int(got["ties"][0]) == n ** 3 - n and int(got["status"][0]) == 0


_LIMIT = {}


def test_read_limit(gpu_ctx, geom):
    """4,096 counted reads are tested, 4,097 are not (status 2, no error), and
    4,097 participating reads of which one is short are; reads outside the
    range do not count towards the limit."""
    if not _LIMIT:
        rng = np.random.default_rng(4096)

        def reads(k):
            return [(int(h), [(100 + j % 50, int(c)), (101 + j % 40, int(d))])
                    for j, (h, c, d) in enumerate(zip(rng.integers(0, 2, k), rng.integers(0, 2, k), rng.integers(0, 2, k)))]
        far = [(0, [(5000, 0), (5001, 0)])] * 10
        b = _calls_batch([(100, 150, far + reads(4096)), (100, 150, reads(4097)),
                          (100, 150, reads(2000) + [(1, [(120, 0)])] + reads(2096) + [(254, [(120, 0), (121, 0)])])])
        _LIMIT["b"], _LIMIT["ref"] = b, rank_ref_batch(b, 2)
    got = _check(gpu_ctx, _LIMIT["b"], 2, "limit", ref=_LIMIT["ref"])
    assert got["status"].tolist() == [0, 2, 0] and int(got["u2"][1]) == 0 and int(got["ties"][1]) == 0
    assert got["n_reads"].sum(axis=1).tolist() == [4096, 4097, 4096] and got["n_short"].tolist() == [[0, 0], [0, 0], [0, 1]]
    assert int(got["u2"][0]) > 0 and int(got["ties"][0]) > 0


@pytest.mark.parametrize("wide", [None, "1"])
def test_1024_threads(gpu_ctx, monkeypatch, wide):
    """Sixteen waves: reads over several rounds' worth of waves, rows past the workgroup."""
    monkeypatch.setenv("PF_RANK_THREADS", "1024")
    if wide:
        monkeypatch.setenv("PF_RANK_WIDE", wide)
    rng = np.random.default_rng(5)
    w = _window(100, 1000, rng.integers(1, 30, 1500), rng.integers(0, 30, 1500), rng.integers(0, 2, 1500))
    got = _check(gpu_ctx, _calls_batch([w]), 3, "1024 threads")
    assert int(got["status"][0]) == 0 and got["n_short"][0].sum() > 0


def test_windows_are_independent(gpu_ctx, geom):
    """Two windows with equal coordinates and different reads, two with equal
    reads (equal results), and an overlapping window."""
    rng = np.random.default_rng(9)

    def reads(k):
        return [_read(50, 400, int(a), int(c), j % 2) for j, (a, c) in enumerate(zip(rng.integers(1, 20, k), rng.integers(1, 20, k)))]
    ra, rb = reads(9), reads(14)
    got = _check(gpu_ctx, _calls_batch([(50, 400, ra), (50, 400, rb), (50, 400, ra), (60, 300, ra)]), 2, "independent")
    for k in ("u2", "ties", "sum", "cls", "n_reads"):
        assert got[k][0].tolist() == got[k][2].tolist(), k
    assert got["sum"][0].tolist() != got["sum"][1].tolist() and got["sum"][3].sum() < got["sum"][0].sum()


def test_read_hp_override(gpu_ctx, geom):
    from pomfret_amd import PomfretError
    rng = np.random.default_rng(21)
    n = 40
    m, u = rng.integers(1, 25, n), rng.integers(1, 25, n)
    own = rng.integers(0, 2, n).astype(np.uint8)
    other = own.copy()
    other[::3] ^= 1
    other[5], other[17] = 254, 3

    def batch(tags):
        return _calls_batch([_window(0, 2000, m, u, tags)])
    db = gpu_ctx.upload(_cfg(), batch(own))
    try:
        with_other = db.ranktest(3, read_hp=other)
        with_own = db.ranktest(3)                        # the batch's own tags are intact afterwards
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.ranktest(3, read_hp=other[:-1])           # n_hp must be the batch's reads
    finally:
        db.free()
    same(with_other, rank_ref_batch(batch(other), 3), "override")
    same(with_other, rank_ref_batch(batch(own), 3, hp=other), "override, reference override")
    same(with_own, rank_ref_batch(batch(own), 3), "own tags afterwards")
    assert (with_other["n_reads"][0].sum() + with_other["n_short"][0].sum()) == n - 2
    assert int(with_other["u2"][0]) != int(with_own["u2"][0])


def test_bad_arguments(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    db = gpu_ctx.upload(_cfg(), _calls_batch([(0, 10, [(0, [(1, 0)]), (1, [(2, 1)])])]))
    try:
        for mc in (0, 65536, 1 << 31):
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.ranktest(mc)
        top = db.ranktest(65535)
        assert top["status"].tolist() == [1] and top["n_short"].tolist() == [[1, 1]]
        one = db.ranktest(1)
        assert one["status"].tolist() == [0] and one["u2"].tolist() == [2] and one["ties"].tolist() == [0]
        for bad in ("128", "0", "2048", "64x", ""):
            monkeypatch.setenv("PF_RANK_THREADS", bad)
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.ranktest(1)
        monkeypatch.setenv("PF_RANK_THREADS", "1024")
        assert db.ranktest(1)["u2"].tolist() == [2]
        for bad in ("2", "yes", "", "01", "-1"):
            monkeypatch.setenv("PF_RANK_WIDE", bad)
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.ranktest(1)
        monkeypatch.setenv("PF_RANK_WIDE", "0")
        assert db.ranktest(1)["u2"].tolist() == [2]
    finally:
        db.free()


def test_no_windows(gpu_ctx):
    db = gpu_ctx.upload(_cfg(), _calls_batch([]))
    got = db.ranktest()
    db.free()
    assert got["u2"].size == 0 and got["n_reads"].shape == (0, 2) and got["cls"].shape == (0, 2, 3)
    assert got["sum"].shape == (0, 4) and got["min_calls"] == 3


def test_record_level_batch(gpu_ctx, oracle_lib, geom):
    """A record-level batch runs its load stage first; the reference reads
    the CPU loader's calls.  The pileup of the same batch still works after."""
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = rank_ref_batch(ref_b, 3)
    assert ref["status"].tolist() == [0, 0] and ref["n_reads"].min() >= 5
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        got = db.ranktest(3)
        again = db.ranktest(3)
        pile = db.pileup()
    finally:
        db.free()
    same(got, ref, "record level")
    same(again, ref, "record level, second call")
    assert pile["pos"].size > 0


def test_between_runs_and_in_flight(gpu_ctx, oracle_lib):
    """The test leaves the batch as it was: a run before and after it gives
    the same results, the test after a run the same integers; while a launched
    run is unfinished the call is refused."""
    from pomfret_amd import PomfretError
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ref = rank_ref_batch(ref_b, 2)
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        res = db.run()
        same(db.ranktest(2), ref, "after a run")
        res2 = db.run()
        for f in ("decision", "read_hp", "dir_table", "win_n_sites", "win_n_reads"):
            assert np.array_equal(getattr(res, f), getattr(res2, f)), f
        db.launch()
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.ranktest(2)
        db.finish()
        same(db.ranktest(2), ref, "after the finish")
    finally:
        db.free()
