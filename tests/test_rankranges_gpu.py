"""The rank test over position ranges inside a batch's windows
(pf_batch_rankranges: pf_rank_ranges, pf_rank.hip) against
the literal reference tests/_rank_ref.rank_ref_batch on the same reads with one
window per range: n_reads, n_short, cls, sum, u2, ties and status, all
integers, every comparison exact.  Every case runs at PF_RANK_THREADS 64, 256
and 1024 and with PF_RANK_WIDE unset and 1.

Not tested: N >= 2^31 calls in one range (PF_ERR_LIMIT), which needs two
billion call entries, and ranges times the workgroup size above 2^32 - 1
(PF_ERR_LIMIT), which needs more than four million ranges and their arrays.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig

from tests._aln_cases import synth_aln
from tests._rank_ref import KEYS, rank_ref_batch, same
from tests.test_permtest_gpu import _read
from tests.test_pileup_gpu import _calls_batch, _cfg
from tests.test_ranktest import KNOWN

pytestmark = pytest.mark.gpu

LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)


@pytest.fixture(params=[(t, w) for t in ("64", "256", "1024") for w in (None, "1")],
                ids=lambda p: "t%s%s" % (p[0], "-wide" if p[1] else ""))
def geom(request, monkeypatch):
    threads, wide = request.param
    monkeypatch.setenv("PF_RANK_THREADS", threads)
    if wide:
        monkeypatch.setenv("PF_RANK_WIDE", wide)
    return request.param


def _flat(ranges):
    """ranges: per window a list of (start, end) -> (off [W + 1], starts, ends)."""
    off = np.cumsum([0] + [len(r) for r in ranges]).astype(np.uint64)
    flat = [x for r in ranges for x in r]
    return off, np.array([s for s, _ in flat], np.uint32), np.array([e for _, e in flat], np.uint32)


def ranges_ref(batch, ranges, min_calls, hp=None):
    """rank_ref_batch with one window per range: range i of window w is the
    window [start, end) over window w's reads of the WindowBatch."""
    parts = []
    for w, rr in enumerate(ranges):
        for s, e in rr:
            one = SimpleNamespace(n_windows=1, win_start=[s], win_end=[e],
                                  win_read_off=[int(batch.win_read_off[w]), int(batch.win_read_off[w + 1])],
                                  read_hp=batch.read_hp, read_call_off=batch.read_call_off, call_pos=batch.call_pos,
                                  call_cat=batch.call_cat)
            parts.append(rank_ref_batch(one, min_calls, hp))
    if not parts:
        return rank_ref_batch(SimpleNamespace(n_windows=0), min_calls)
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


def _check(ctx, batch, ranges, min_calls, tag, hp=None, ref=None):
    ref = ranges_ref(batch, ranges, min_calls, hp) if ref is None else ref
    db = ctx.upload(_cfg(), batch)
    try:
        got = db.rankranges(*_flat(ranges), min_calls=min_calls, read_hp=hp)
    finally:
        db.free()
    same(got, ref, tag)
    assert got["min_calls"] == min_calls and (got["ms"] > 0 or not len(ref["u2"]))
    return got


def _reads(rng, ws, we, k):
    """k reads with 1 .. 12 calls each anywhere in [ws, we), tags 0 / 1 and now and then 254."""
    out = []
    for j in range(k):
        n = int(rng.integers(1, 13))
        a = int(rng.integers(ws, we - 1))
        b = int(rng.integers(a + 1, min(we, a + 700) + 1))
        out.append((254 if j % 9 == 8 else int(rng.integers(0, 2)),
                    [(int(p), int(c)) for p, c in zip(rng.integers(a, b, n), rng.integers(0, 3, n))]))
    return out


_WHOLE = {}


def test_whole_window_is_ranktest(gpu_ctx, geom):
    """One range equal to its window: ranktest's dict for the batch, field for field."""
    if not _WHOLE:
        rng = np.random.default_rng(77)
        wins = [(100, 3000, _reads(rng, 100, 3000, 150)), (5000, 5400, _reads(rng, 5000, 5400, 70)), (9000, 9100, [])]
        _WHOLE["b"] = _calls_batch(wins)
        _WHOLE["r"] = [[(s, e)] for s, e, _ in wins]
        _WHOLE["ref"] = rank_ref_batch(_WHOLE["b"], 2)
    b, ranges = _WHOLE["b"], _WHOLE["r"]
    got = _check(gpu_ctx, b, ranges, 2, "whole", ref=_WHOLE["ref"])
    db = gpu_ctx.upload(_cfg(), b)
    try:
        whole = db.ranktest(2)
    finally:
        db.free()
    same(got, whole, "whole window against ranktest")
    assert got["status"].tolist() == [0, 0, 1]


def test_known_answers_inside_a_wider_window(gpu_ctx, geom):
    """Every KNOWN case of tests/test_ranktest.py as the range [505, 1400) of
    the window [0, 2000), between reads that lie left of it, right of it, on
    both sides without a call inside, and an untagged read inside."""
    others = [(0, [(10, 0), (504, 1)]), (1, [(1400, 0), (1999, 1)]), (0, [(300, 0), (1700, 0)]), (254, [(600, 0), (700, 1)])]
    for name, ((m, u, tags, mc), (nr, ns, cls, u2, ties, status)) in sorted(KNOWN.items()):
        reads = [_read(505, 1400, int(a), int(c), int(h)) for a, c, h in zip(m, u, tags)]
        b = _calls_batch([(0, 2000, others[:2] + reads + others[2:])])
        got = _check(gpu_ctx, b, [[(505, 1400)]], mc, name)
        assert (got["n_reads"][0].tolist(), got["n_short"][0].tolist(), got["cls"][0].tolist()) == (nr, ns, cls), name
        assert (int(got["u2"][0]), int(got["ties"][0]), int(got["status"][0])) == (u2, ties, status), name


def test_range_edges(gpu_ctx, geom):
    """A call at start and one at end - 1 are in; one at end and one at start - 1
    are out; reads left of, right of, and around the range take no part."""
    reads = [(0, [(200, 0)]), (1, [(299, 1)]), (0, [(300, 0)]), (1, [(199, 1)]), (0, [(10, 0), (150, 1)]),
             (1, [(400, 0), (900, 1)]), (0, [(100, 0), (500, 1)])]
    b = _calls_batch([(0, 1000, reads)])
    got = _check(gpu_ctx, b, [[(200, 300), (201, 299), (199, 301), (300, 301), (160, 199)]], 1, "edges")
    assert got["n_reads"].tolist() == [[1, 1], [0, 0], [2, 2], [1, 0], [0, 0]]
    assert got["sum"].tolist() == [[1, 0, 0, 1], [0, 0, 0, 0], [2, 0, 0, 2], [1, 0, 0, 0], [0, 0, 0, 0]]
    assert got["status"].tolist() == [0, 1, 0, 1, 1] and got["u2"].tolist() == [2, 0, 8, 0, 0]


def test_span_overlaps_without_a_call_inside(gpu_ctx, geom):
    """Every read's calls lie on both sides of the range, so the seek's end
    checks pass; only the search can tell that all but two have no call in it."""
    around = [(k % 2, [(100 + k, 0), (250 - k, 1), (400 + k, k % 2), (900, 1)]) for k in range(90)]
    inside = [(0, [(120, 0), (300, 0), (310, 0)]), (1, [(130, 1), (305, 1), (880, 0)])]
    b = _calls_batch([(0, 1000, around[:50] + inside + around[50:])])
    got = _check(gpu_ctx, b, [[(260, 390), (251, 400), (0, 1000)]], 1, "spans")
    assert got["n_reads"].tolist() == [[1, 1], [1, 1], [46, 46]] and got["sum"][0].tolist() == [2, 0, 0, 1]
    assert got["u2"][:2].tolist() == [2, 2]


def test_range_mix(gpu_ctx, geom):
    """An empty range, a range with no read, overlapping ranges and two identical ranges."""
    rng = np.random.default_rng(31)
    b = _calls_batch([(1000, 5000, _reads(rng, 1000, 4000, 120))])
    ranges = [[(2000, 2000), (4500, 5000), (1500, 2500), (2000, 3000), (1500, 2500), (1000, 5000), (5000, 5000), (1000, 1000)]]
    got = _check(gpu_ctx, b, ranges, 1, "mix")
    for k in KEYS:
        assert got[k][2].tolist() == got[k][4].tolist(), k                 # identical ranges, identical entries
        for i in (0, 1, 6, 7):
            assert not np.asarray(got[k][i]).any() or k == "status", (k, i)
    assert got["status"].tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    assert got["n_reads"][2].sum() < got["n_reads"][5].sum() > got["n_reads"][3].sum()


def test_window_lookup(gpu_ctx, geom):
    """Five windows with 0, 3, 0, 1, 0 ranges: windows without a range at both
    ends and in the middle; every result also equals that of a batch that
    holds its window alone."""
    rng = np.random.default_rng(8)
    wins = [(k * 10_000, k * 10_000 + 3000, _reads(rng, k * 10_000, k * 10_000 + 3000, 30 + 7 * k)) for k in range(5)]
    ranges = [[], [(10_000, 11_000), (11_000, 12_000), (12_000, 13_000)], [], [(30_500, 32_500)], []]
    got = _check(gpu_ctx, _calls_batch(wins), ranges, 2, "lookup")
    assert got["status"].tolist() == [0, 0, 0, 0] and got["u2"].size == 4
    alone1 = _check(gpu_ctx, _calls_batch([wins[1]]), [ranges[1]], 2, "window 1 alone")
    alone3 = _check(gpu_ctx, _calls_batch([wins[3]]), [ranges[3]], 2, "window 3 alone")
    for k in KEYS:
        assert got[k][:3].tolist() == alone1[k].tolist() and got[k][3:].tolist() == alone3[k].tolist(), k
    # ranges in the first and in the last window, none between
    ends = _check(gpu_ctx, _calls_batch(wins), [[(0, 3000)], [], [], [], [(40_000, 41_000), (41_000, 43_000)]], 2, "ends")
    assert ends["n_reads"].sum(axis=1).min() > 0


_LIMIT = {}


def test_read_limit(gpu_ctx, geom):
    """4,097 counted reads in one range: status 2; the neighbouring range of
    the same window, 40 reads, is tested."""
    if not _LIMIT:
        rng = np.random.default_rng(4097)
        k = 4097
        many = [(int(h), [(100 + j % 50, int(c)), (101 + j % 40, int(d))])
                for j, (h, c, d) in enumerate(zip(rng.integers(0, 2, k), rng.integers(0, 2, k), rng.integers(0, 2, k)))]
        few = [(j % 2, [(150 + (3 * j) % 50, int(c)), (152 + j % 40, int(d)), (199, j % 2)])
               for j, (c, d) in enumerate(zip(rng.integers(0, 2, 40), rng.integers(0, 2, 40)))]
        _LIMIT["b"] = _calls_batch([(100, 200, many[:2000] + few + many[2000:])])
        _LIMIT["r"] = [[(100, 150), (150, 200), (100, 200)]]
        _LIMIT["ref"] = ranges_ref(_LIMIT["b"], _LIMIT["r"], 2)
    got = _check(gpu_ctx, _LIMIT["b"], _LIMIT["r"], 2, "limit", ref=_LIMIT["ref"])
    assert got["status"].tolist() == [2, 0, 2] and got["n_reads"].sum(axis=1).tolist() == [4097, 40, 4137]
    assert got["u2"].tolist()[0] == 0 and int(got["u2"][1]) > 0 and int(got["ties"][1]) > 0


@pytest.mark.parametrize("min_calls", [1, 3])
def test_min_calls(gpu_ctx, geom, min_calls):
    rng = np.random.default_rng(12)
    b = _calls_batch([(0, 6000, _reads(rng, 0, 6000, 260))])
    ranges = [[(s, s + 500) for s in range(0, 6000, 500)]]
    got = _check(gpu_ctx, b, ranges, min_calls, f"min_calls {min_calls}")
    if min_calls == 1:
        assert not got["n_short"].any()
    else:
        one = ranges_ref(b, ranges, 1)
        assert got["n_short"].sum() > 20
        assert (got["n_short"] + got["n_reads"]).tolist() == one["n_reads"].tolist()    # the same participating reads


def test_read_hp_override(gpu_ctx, geom):
    from pomfret_amd import PomfretError
    rng = np.random.default_rng(21)
    reads = _reads(rng, 0, 3000, 80)
    own = np.array([h for h, _ in reads], np.uint8)
    other = own.copy()
    other[::3] ^= 1
    other[5], other[17] = 254, 3
    ranges = [[(0, 1000), (500, 2500), (2000, 3000)]]

    def batch(tags):
        return _calls_batch([(0, 3000, [(int(t), c) for t, (_, c) in zip(tags, reads)])])
    off, s, e = _flat(ranges)
    db = gpu_ctx.upload(_cfg(), batch(own))
    try:
        with_other = db.rankranges(off, s, e, 2, read_hp=other)
        with_own = db.rankranges(off, s, e, 2)               # the batch's own tags are intact afterwards
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.rankranges(off, s, e, 2, read_hp=other[:-1])  # n_hp must be the batch's reads
    finally:
        db.free()
    same(with_other, ranges_ref(batch(other), ranges, 2), "override")
    same(with_other, ranges_ref(batch(own), ranges, 2, hp=other), "override, reference override")
    same(with_own, ranges_ref(batch(own), ranges, 2), "own tags afterwards")
    assert with_other["u2"].tolist() != with_own["u2"].tolist()


_RECORD = {}


def test_record_level_batch(gpu_ctx, oracle_lib, geom):
    """A record-level batch through K0, two windows in tiles of 1 kb; the
    reference reads the CPU loader's calls.  The pileup of the same batch still
    works after, and a second call gives the same."""
    if not _RECORD:
        aln = synth_aln(2, 30, 5, len_scale=0.3)
        ref_b, _ = oracle_lib.load_reads(LCFG, aln)
        ranges = [[(s, min(s + 1000, int(e))) for s in range(int(ws), int(e), 1000)]
                  for ws, e in zip(ref_b.win_start, ref_b.win_end)]
        _RECORD.update(aln=aln, ranges=ranges, ref=ranges_ref(ref_b, ranges, 3))
    ref, ranges = _RECORD["ref"], _RECORD["ranges"]
    assert len(ref["u2"]) == 100 and (ref["status"] == 0).sum() > 40 and ref["n_short"].sum() > 0
    db = gpu_ctx.upload_aln(_cfg(), _RECORD["aln"], LCFG)
    try:
        got = db.rankranges(*_flat(ranges), min_calls=3)
        pile = db.pileup()
        again = db.rankranges(*_flat(ranges), min_calls=3)
    finally:
        db.free()
    same(got, ref, "record level")
    same(again, ref, "record level, after the pileup")
    assert pile["pos"].size > 0


def test_bad_arguments(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    b = _calls_batch([(10, 100, [(0, [(20, 0)]), (1, [(30, 1)])]), (200, 300, [(0, [(210, 0)]), (1, [(220, 1)])])])
    db = gpu_ctx.upload(_cfg(), b)

    def bad(off, s, e, mc=1):
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.rankranges(np.array(off, np.uint64), s, e, mc)
    try:
        ok = db.rankranges([0, 1, 2], [10, 200], [100, 300], 1)
        assert ok["status"].tolist() == [0, 0] and ok["u2"].tolist() == [2, 2]
        bad([0, 1, 2], [9, 200], [100, 300])                 # start left of the window
        bad([0, 1, 2], [10, 200], [101, 300])                # end right of it
        bad([0, 1, 2], [50, 200], [49, 300])                 # end left of start
        bad([0, 1, 2], [10, 10], [100, 100])                 # the second range lies in the first window
        bad([0, 3, 2], [10, 200], [100, 300])                # offsets that decrease
        bad([1, 1, 2], [10, 200], [100, 300])                # offsets that do not start at 0
        for mc in (0, 65536, 1 << 31):
            bad([0, 1, 2], [10, 200], [100, 300], mc)
        # more than 2^31 - 1 ranges: refused on the offsets alone, before a start or an end is read.  The
        # wrapper wants as many starts as off[-1], so this one goes to the library directly
        import ctypes as C
        from pomfret_amd import lib
        from pomfret_amd.abi import PfRank
        one = np.zeros(1, np.uint32)
        for top, rc in ((1 << 31, -1), (1 << 40, -1)):
            off = np.array([0, 1, top], np.uint64)
            p = C.POINTER(PfRank)()
            assert lib().pf_batch_rankranges(db.ctx.handle, db.handle, None, 0, 1, off.ctypes.data, one.ctypes.data,
                                             one.ctypes.data, C.byref(p)) == rc and not p
        assert db.rankranges([0, 1, 2], [10, 200], [100, 300], 65535)["n_short"].tolist() == [[1, 1], [1, 1]]
        for v in ("128", "0", "2048", "64x", ""):
            monkeypatch.setenv("PF_RANK_THREADS", v)
            bad([0, 1, 2], [10, 200], [100, 300])
        monkeypatch.setenv("PF_RANK_THREADS", "1024")
        assert db.rankranges([0, 1, 2], [10, 200], [100, 300], 1)["u2"].tolist() == [2, 2]
        monkeypatch.delenv("PF_RANK_THREADS")
        for v in ("2", "yes", ""):
            monkeypatch.setenv("PF_RANK_WIDE", v)
            bad([0, 1, 2], [10, 200], [100, 300])
        monkeypatch.delenv("PF_RANK_WIDE")
        for v in ("2", "on"):
            monkeypatch.setenv("PF_RANKR_LDS_FIXED", v)
            bad([0, 1, 2], [10, 200], [100, 300])
        monkeypatch.setenv("PF_RANKR_LDS_FIXED", "1")        # the 4,096-read array: the same integers
        same(db.rankranges([0, 1, 2], [10, 200], [100, 300], 1), ok, "fixed LDS")
        monkeypatch.delenv("PF_RANKR_LDS_FIXED")
        # windows without a single range: an empty result, not an error
        none = db.rankranges([0, 0, 0], [], [], 1)
        assert none["u2"].size == 0 and none["n_reads"].shape == (0, 2) and none["cls"].shape == (0, 2, 3)
    finally:
        db.free()


def test_no_windows(gpu_ctx):
    db = gpu_ctx.upload(_cfg(), _calls_batch([]))
    got = db.rankranges([0], [], [])
    db.free()
    assert got["u2"].size == 0 and got["sum"].shape == (0, 4) and got["min_calls"] == 3


def test_refused_while_a_run_is_in_flight(gpu_ctx, oracle_lib):
    from pomfret_amd import PomfretError
    aln = synth_aln(2, 30, 5, len_scale=0.3)
    ref_b, _ = oracle_lib.load_reads(LCFG, aln)
    ranges = [[(int(s), int(s) + 2000)] for s in ref_b.win_start]
    ref = ranges_ref(ref_b, ranges, 2)
    db = gpu_ctx.upload_aln(_cfg(), aln, LCFG)
    try:
        res = db.run()
        same(db.rankranges(*_flat(ranges), min_calls=2), ref, "after a run")
        db.launch()
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            db.rankranges(*_flat(ranges), min_calls=2)
        db.finish()
        same(db.rankranges(*_flat(ranges), min_calls=2), ref, "after the finish")
        res2 = db.run()
        assert np.array_equal(res.decision, res2.decision)
    finally:
        db.free()
