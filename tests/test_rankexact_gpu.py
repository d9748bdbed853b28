"""The exact rank test on the device (pf_batch_rankexact, pf_rank_exact in
pf_rank.hip) against tests/_rankexact_ref.py's dp(), which tests/test_rankexact.py
pins to brute force: n_reads, n_short, u2, total, le, ge, two and status, every
integer compared exactly, and n_reads, n_short and u2 against DeviceBatch.ranktest
on the same batch.  Hand-built calls-level batches are their own reference
input; the record-level batch's reference input comes from the CPU loader.
Every case runs under the default geometry (1,024 threads), PF_RANKX_THREADS=64 (one wave),
PF_RANKX_HBM=1 (every table in the workgroup's slab) and PF_RANKX_GRID=1 (one
workgroup takes every window in turn).  Each batch's reference is computed
once and shared by the four.

Not tested: N >= 2^31 calls in one window (PF_ERR_LIMIT) -- it needs two
billion call entries.
"""
from math import comb

import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig

from tests._aln_cases import synth_aln
from tests._rankexact_ref import rankexact_ref_batch, same
from tests.test_permtest_gpu import _read
from tests.test_pileup_gpu import _calls_batch, _cfg

pytestmark = pytest.mark.gpu

LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)
KNOBS = [{}, {"PF_RANKX_THREADS": "64"}, {"PF_RANKX_HBM": "1"}, {"PF_RANKX_GRID": "1"}]


@pytest.fixture(params=KNOBS, ids=["default", "t64", "hbm", "grid1"])
def geom(request, monkeypatch):
    for k, v in request.param.items():
        monkeypatch.setenv(k, v)
    return request.param


def _window(ws, we, m, u, tags):
    return ws, we, [_read(ws, we, int(a), int(c), int(h)) for a, c, h in zip(m, u, tags)]


_REF = {}


def _ref(key, batch, min_calls, max_reads=64, hp=None):
    k = (key, min_calls, max_reads)
    if k not in _REF:
        _REF[k] = rankexact_ref_batch(batch, min_calls, max_reads, hp)
    return _REF[k]


def _check(ctx, key, batch, min_calls, max_reads=64, hp=None):
    ref = _ref(key, batch, min_calls, max_reads, hp)
    db = ctx.upload(_cfg(), batch)
    try:
        got = db.rankexact(min_calls, max_reads, read_hp=hp)
        rank = db.ranktest(min_calls, read_hp=hp)
    finally:
        db.free()
    same(got, ref, f"{key}, max_reads {max_reads}")
    for k in ("n_reads", "n_short", "u2"):
        assert np.array_equal(got[k], rank[k]), (key, k)
    assert got["min_calls"] == min_calls and got["max_reads"] == max_reads and got["ms"] > 0
    tested = got["status"] == 0
    assert np.array_equal(got["total"][tested], [comb(int(a + b), int(a)) for a, b in got["n_reads"][tested]])
    return got


def _distinct(n, den, rng):
    """n reads of den calls each with distinct numbers of meth calls: no ties."""
    m = rng.permutation(den + 1)[:n]
    return m, den - m


_BATCH = {}


def _shapes():
    """n = 2, 3; 1 + 63, the narrowest table; 32 + 32 without ties, the widest,
    and all tied, one live cell a row; 31 + 33 and 33 + 31, either class the
    smaller; 63, 64 and 65 reads with ties; a read of 70,000 calls beside small
    ones (64-bit products)."""
    if "shapes" not in _BATCH:
        rng = np.random.default_rng(6464)
        w = []
        w.append(_window(10, 90, [3, 1], [1, 3], [0, 1]))
        w.append(_window(10, 90, [3, 1, 2], [1, 3, 2], [1, 0, 1]))
        m, u = _distinct(64, 70, rng)
        w.append(_window(10, 90, m, u, [1] * 40 + [0] + [1] * 23))
        w.append(_window(10, 90, m, u, rng.permutation([0] * 32 + [1] * 32)))
        w.append(_window(10, 90, [1 + k % 7 for k in range(64)], [1 + k % 7 for k in range(64)], [k % 2 for k in range(64)]))
        m, u = _distinct(64, 75, rng)
        t = rng.permutation([0] * 31 + [1] * 33)
        w.append(_window(10, 90, m, u, t))
        w.append(_window(10, 90, m, u, 1 - t))
        for n in (63, 64, 65):
            m, u = rng.integers(0, 9, n), rng.integers(0, 9, n)
            m[(m + u) == 0] = 1
            w.append(_window(10, 90, m, u, rng.integers(0, 2, n)))
        w.append(_window(10, 90, [35000, 1, 1, 3, 2, 0], [35000, 1, 3, 1, 2, 4], [0, 1, 0, 1, 0, 1]))
        _BATCH["shapes"] = _calls_batch(w)
    return _BATCH["shapes"]


def test_shapes(gpu_ctx, geom):
    got = _check(gpu_ctx, "shapes", _shapes(), 1)
    assert got["status"].tolist() == [0] * 9 + [2, 0]
    assert got["n_reads"].tolist()[:7] == [[1, 1], [1, 2], [1, 63], [32, 32], [32, 32], [31, 33], [33, 31]]
    assert got["n_reads"].sum(axis=1).tolist()[7:] == [63, 64, 65, 6]
    big = comb(64, 32)
    assert int(got["total"][3]) == big > 2 ** 60 and 0 < int(got["two"][3]) < big and int(got["le"][3]) + int(got["ge"][3]) > big
    assert [int(got[k][4]) for k in ("le", "ge", "two", "total")] == [big] * 4
    # the complementary tags: le and ge change places, two stays
    assert (int(got["le"][5]), int(got["ge"][5]), int(got["two"][5])) == (int(got["ge"][6]), int(got["le"][6]), int(got["two"][6]))
    assert [int(got[k][9]) for k in ("le", "ge", "two", "total")] == [0] * 4 and int(got["u2"][9]) > 0


def test_shapes_at_max_reads_8(gpu_ctx, geom):
    got = _check(gpu_ctx, "shapes", _shapes(), 1, max_reads=8)
    assert got["status"].tolist() == [0, 0] + [2] * 8 + [0]
    over = got["status"] == 2
    assert not got["total"][over].any() and not got["two"][over].any() and got["u2"][over].all()


def test_placement_boundary_and_reuse(gpu_ctx, geom, monkeypatch):
    """36 reads, 18 a class, is the last table in LDS (8,113 cells) and 40 / 20
    the first in the slab (11,081).  Five windows under PF_RANKX_GRID=2: one
    workgroup takes 40, a window without haplotype 1 and 38 reads, reusing its
    slab after a larger table, the other 36 and 30, reusing its LDS array."""
    if "PF_RANKX_GRID" not in geom:
        monkeypatch.setenv("PF_RANKX_GRID", "2")
    if "place" not in _BATCH:
        rng = np.random.default_rng(3640)
        w = []
        for n, k in ((40, 20), (36, 18), (7, 0), (30, 15), (38, 19)):
            m, u = (rng.integers(0, 30, n), rng.integers(0, 30, n)) if n != 36 else _distinct(36, 50, rng)
            m[(m + u) == 0] = 1
            w.append(_window(100, 200, m, u, rng.permutation([0] * k + [1] * (n - k))))
        _BATCH["place"] = _calls_batch(w)
    got = _check(gpu_ctx, "place", _BATCH["place"], 1)
    assert got["status"].tolist() == [0, 0, 1, 0, 0] and got["n_reads"].tolist()[2] == [0, 7]
    assert [int(got[k][2]) for k in ("u2", "le", "ge", "two", "total")] == [0] * 5


@pytest.mark.parametrize("min_calls", [1, 2, 3])
def test_who_participates(gpu_ctx, geom, min_calls):
    """test_ranktest_gpu's participation cases: windows without reads, reads
    that overlap the window without a call in it, tags 254 and 3 between
    tagged reads, cat 2 and duplicate entries, an empty and a zero-width
    window."""
    inside = [(1, [(210, 0), (220, 1)]), (0, [(230, 0), (231, 0), (240, 1)]), (1, [(250, 1), (251, 1)]), (0, [(260, 0)])]
    out_l, out_r, nocall = (0, [(10, 0), (199, 1)]), (1, [(300, 0), (5000, 1)]), (0, [(250, 2)])
    shifted = [out_l, inside[0], nocall, inside[1], out_r, (0, []), inside[2], inside[3]]
    other = [inside[0], (254, [(210, 0)] * 5), inside[1], (3, [(215, 1)] * 7), inside[2], (254, []), inside[3]]
    dup = [(1, [(210, 0), (210, 0), (220, 1), (222, 2)]), (0, [(230, 0), (230, 1), (230, 2), (230, 2)]),
           (1, [(250, 1), (250, 1), (250, 1)]), (0, [(299, 0), (299, 0), (300, 0)])]
    b = _calls_batch([(200, 300, []), (200, 300, inside), (200, 300, shifted), (200, 300, other), (200, 300, dup),
                      (7, 7, [(0, [(7, 0)]), (1, [(7, 1)])]), (200, 300, [nocall, out_l, (254, [(210, 0)])])])
    got = _check(gpu_ctx, "participation", b, min_calls)
    assert (got["n_reads"] + got["n_short"]).tolist() == [[0, 0], [2, 2], [2, 2], [2, 2], [2, 2], [0, 0], [0, 0]]
    exp = {1: [1, 0, 0, 0, 0, 1, 1], 2: [1, 0, 0, 0, 0, 1, 1], 3: [1, 1, 1, 1, 1, 1, 1]}[min_calls]
    assert got["status"].tolist() == exp
    for k in ("u2", "le", "ge", "two", "total"):
        assert int(got[k][1]) == int(got[k][2]) == int(got[k][3]), k
    if min_calls == 1:
        assert int(got["total"][1]) == 6 and int(got["total"][4]) == 6


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
        with_other = db.rankexact(3, read_hp=other)
        with_own = db.rankexact(3)                       # the batch's own tags are intact afterwards
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.rankexact(3, read_hp=other[:-1])          # n_hp must be the batch's reads
    finally:
        db.free()
    same(with_other, _ref("hp other", batch(other), 3), "override")
    same(with_other, _ref("hp own, other given", batch(own), 3, hp=other), "override, reference override")
    same(with_own, _ref("hp own", batch(own), 3), "own tags afterwards")
    assert int(with_other["two"][0]) != int(with_own["two"][0]) and with_other["status"].tolist() == [0]


def test_record_level_batch(gpu_ctx, oracle_lib, geom):
    """A record-level batch runs its load stage first; the reference reads the
    CPU loader's calls.  At coverage 20 the two windows hold 42 and 34 counted
    reads: one table in the slab, one in LDS.  The rank test and the pileup
    still work after."""
    aln = synth_aln(2, 20, 5, len_scale=0.3)
    if "rec" not in _BATCH:
        _BATCH["rec"] = oracle_lib.load_reads(LCFG, aln)[0]
    ref = _ref("rec", _BATCH["rec"], 3)
    assert ref["status"].tolist() == [0, 0] and ref["n_reads"].sum(axis=1).tolist() == [42, 34]
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        got = db.rankexact(3)
        again = db.rankexact(3)
        rank = db.ranktest(3)
        pile = db.pileup()
    finally:
        db.free()
    same(got, ref, "record level")
    same(again, ref, "record level, second call")
    assert np.array_equal(got["u2"], rank["u2"]) and np.array_equal(got["n_reads"], rank["n_reads"]) and pile["pos"].size > 0


def test_between_runs_and_in_flight(gpu_ctx, oracle_lib):
    """The call leaves the batch as it was, and is refused while a launched run is unfinished."""
    from pomfret_amd import PomfretError
    aln = synth_aln(2, 20, 5, len_scale=0.3)
    if "rec" not in _BATCH:
        _BATCH["rec"] = oracle_lib.load_reads(LCFG, aln)[0]
    ref = _ref("rec", _BATCH["rec"], 2)
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        res = db.run()
        same(db.rankexact(2), ref, "after a run")
        res2 = db.run()
        for f in ("decision", "read_hp", "dir_table", "win_n_sites", "win_n_reads"):
            assert np.array_equal(getattr(res, f), getattr(res2, f)), f
        db.launch()
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.rankexact(2)
        db.finish()
        same(db.rankexact(2), ref, "after the finish")
    finally:
        db.free()


def test_256_threads(gpu_ctx, monkeypatch):
    """The default is 1,024 threads and the fixture's other size one wave: four waves here."""
    monkeypatch.setenv("PF_RANKX_THREADS", "256")
    _check(gpu_ctx, "shapes", _shapes(), 1)


def test_bad_arguments(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    db = gpu_ctx.upload(_cfg(), _calls_batch([(0, 10, [(0, [(1, 0)]), (1, [(2, 1)])])]))
    try:
        for mc, mx in ((0, 64), (65536, 64), (1 << 31, 64), (1, 1), (1, 0), (1, 65), (1, 1 << 31)):
            with pytest.raises(PomfretError, match=r"\(-1\)"):
                db.rankexact(mc, mx)
        top = db.rankexact(65535)
        assert top["status"].tolist() == [1] and top["n_short"].tolist() == [[1, 1]] and top["total"].tolist() == [0]
        one = db.rankexact(1, 2)
        assert (one["status"].tolist(), one["u2"].tolist(), one["total"].tolist(), one["le"].tolist(), one["ge"].tolist(),
                one["two"].tolist()) == ([0], [2], [2], [2], [1], [2])
        for name, bad, good in (("PF_RANKX_THREADS", ("128", "0", "2048", "64x", ""), "1024"),
                                ("PF_RANKX_HBM", ("2", "yes", "", "01", "-1"), "0"),
                                ("PF_RANKX_GRID", ("0", "-1", "", "2x", "65537", "x"), "65536")):
            for v in bad:
                monkeypatch.setenv(name, v)
                with pytest.raises(PomfretError, match=r"\(-1\)"):
                    db.rankexact(1)
            monkeypatch.setenv(name, good)
            assert db.rankexact(1)["two"].tolist() == [2]
            monkeypatch.delenv(name)
    finally:
        db.free()


def test_no_windows(gpu_ctx):
    db = gpu_ctx.upload(_cfg(), _calls_batch([]))
    got = db.rankexact()
    db.free()
    assert got["two"].size == 0 and got["n_reads"].shape == (0, 2) and got["min_calls"] == 3 and got["max_reads"] == 64
