"""Record-level batches whose calls K12 reads where K0 staged them.

The pack step copies no call: every read carries a range [begin, end) in
K0's staging arrays (static slices with unused tails, filtered records'
slices in between, a bump-allocated tail), and K12, pf_k12_chunks and
pf_k2_methmers walk the window's calls read by read.  These tests drive every
K12 route over such ranges, put run lengths on the edges of the per-read loop
(64-call groups, four in flight), show that no kernel reads the slack between
the ranges, and keep two runs in flight on one batch.  The CPU oracle
(load_reads + methphase) is the reference throughout: integer fields bit for
bit, Fisher p at rtol 1e-6.
"""
import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig

from tests._aln_cases import LOAD_CFG_SMALL, records_batch, synth_aln

pytestmark = pytest.mark.gpu

INT_FIELDS = ("decision", "dir_table", "dir_join", "dir_which_way", "win_n_sites", "win_n_reads", "read_hp")
ALL_FIELDS = INT_FIELDS + ("dir_fisher_p", "dir_score")
UNROLL = 4                                   # PF_K12_CU: 64-call groups in flight per wave


def _cfg():
    from pomfret_amd import Config
    return Config.from_coverage(30, given=False)


class _Ref:
    """The oracle's view of a record-level batch, computed once."""

    def __init__(self, oracle_lib, cfg, lcfg, aln):
        self.cfg, self.lcfg, self.aln = cfg, lcfg, aln
        self.b, self.rec_read = oracle_lib.load_reads(lcfg, aln)
        self.out = oracle_lib.methphase(cfg, self.b, n_threads=8)
        self.mmr = [[oracle_lib.window_methmers(cfg, self.b, w, d) for w in range(self.b.n_windows)]
                    for d in (0, 1)]


def _compare(ref, out, tag):
    for f in INT_FIELDS:
        a, g = getattr(ref, f), getattr(out, f)
        assert np.array_equal(a, g), f"{tag}: {f} differs at {np.argwhere(a != g)[:5].tolist()}"
    np.testing.assert_allclose(out.dir_fisher_p, ref.dir_fisher_p, rtol=1e-6, atol=0, err_msg=tag)


def _methmers(db):
    return [db.debug_methmers(d) for d in (0, 1)]


def _compare_methmers(ref: _Ref, got, tag):
    ro = ref.b.win_read_off
    for d in (0, 1):
        n, st, keys = got[d]
        k0 = 0
        for w in range(ref.b.n_windows):
            on, ost, okeys = ref.mmr[d][w]
            assert np.array_equal(on, n[ro[w]:ro[w + 1]]), f"{tag}: w{w} d{d} mmr_n"
            assert np.array_equal(ost, st[ro[w]:ro[w + 1]]), f"{tag}: w{w} d{d} mmr_start"
            assert np.array_equal(okeys, keys[k0:k0 + len(okeys)]), f"{tag}: w{w} d{d} keys"
            k0 += len(okeys)
        assert k0 == len(keys), f"{tag}: d{d} key count"


@pytest.fixture(scope="module")
def mix_ref(oracle_lib):
    """Every MM/ML layout of the generator: slices with slack (trigger bounds
    of two entries or two codes for one list of calls, records that drop out)
    and reads in the bump tail (implicit-canonical).  The generator writes no
    record with several C m entries; test_run_lengths_at_loop_edges sends
    some through pf_k0_multi."""
    aln = synth_aln(3, 30, 61, mm_mix=True, implicit_frac=0.2)
    return _Ref(oracle_lib, _cfg(), LoadConfig(), aln)


ROUTES = [{}, {"PF_K12_DENSE": "1"}, {"PF_K12_SMAX": "0"}, {"PF_K12_CAP": "0"},
          {"PF_K12_CAP": "0", "PF_K2_ENTCAP": "0"}, {"PF_K12_CAP": "40"}, {"PF_K12C_MINR": "1"},
          {"PF_TEST_TIGHT": "1"}]


@pytest.mark.parametrize("env", ROUTES, ids=["default", "dense", "no_lds_sites", "all_reads_fallback",
                                             "fallback_hbm_scratch", "mixed", "all_windows_chunked", "tight"])
def test_every_k12_route_at_record_level(gpu_ctx, monkeypatch, mix_ref, env):
    """The fast and the dense site paths, the K2 fallback (LDS and HBM
    scratch), pf_k12_chunks and a batch whose arrays all start too small, on
    call ranges that are not adjacent: every read's methmers in both
    directions and the whole result equal the oracle's."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    db = gpu_ctx.upload_aln(mix_ref.cfg, mix_ref.aln, mix_ref.lcfg)
    got = _methmers(db)
    assert db.n_reads == mix_ref.b.n_reads
    _compare_methmers(mix_ref, got, str(env))
    out = db.run()
    _compare(mix_ref.out, out, str(env))
    if "PF_K12_DENSE" in env:
        k12 = db.k12_paths()
        assert set(k12[k12 > 0].tolist()) == {3}
        assert (k12 == 3).sum() >= (out.win_n_sites > 0).sum() > 0
    db.free()


# ---- run lengths at the edges of the per-read loop
RUN_LENGTHS = sorted({1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
                      UNROLL * 64 - 1, UNROLL * 64 + 1})


def _edge_record(n, hp, rng, pos, mapq=60, second_entry=False):
    """A read of exactly n calls: a CG repeat (every C a CpG) with every C
    called (zero skips), methylated on one haplotype's even CpGs and the
    other's odd ones, with a little seeded noise.  The repeat starts at read
    position 1 (a call on the first base is none, blockjoin.c:847) and a tail
    without C or G keeps the shortest read above the length filter.
    second_entry: a C-m entry that calls the first C again, so the record goes
    through pf_k0_multi (the two calls merge: still n)."""
    seq = "A" + "CG" * n + "AT" * 4
    meth = (np.arange(n) + hp) % 2 == 0
    meth ^= rng.random(n) < 0.05
    ml = np.where(meth, 220, 20).astype(np.uint8).tolist()
    mm = "C+m?," + ",".join(["0"] * n) + ";"
    if second_entry:
        mm += "C-m?,0;"
        ml.append(ml[0])
    return dict(seq=seq, cigar=f"{len(seq)}M", mm=mm, ml=ml, pos=pos, hp=hp, mapq=mapq)


def _edge_batch():
    rng = np.random.default_rng(7)
    lens = [RUN_LENGTHS[i % len(RUN_LENGTHS)] for i in range(32)]
    w0 = [_edge_record(n, i % 2, rng, 1000) for i, n in enumerate(lens)]
    # the same reads behind and in front of a filtered record (MAPQ 0), some through pf_k0_multi
    w1 = ([_edge_record(300, 0, rng, 5000, mapq=0)] +
          [_edge_record(n, i % 2, rng, 5000, second_entry=i % 5 == 0) for i, n in enumerate(lens[::-1])] +
          [_edge_record(129, 1, rng, 5000, mapq=0)])
    # no kept read at all
    w2 = [_edge_record(65, i % 2, rng, 9000, mapq=0) for i in range(4)]
    return records_batch([(1000, 1400, w0), (5000, 5400, w1), (9000, 9400, w2)]), lens


def test_run_lengths_at_loop_edges(oracle_lib, gpu_ctx):
    """32 reads (16 per haplotype, all starting at the window start) of 1 to
    513 calls, around every multiple of the 64-call group and of the four
    groups a wave keeps in flight: sites, calls and results equal the
    oracle's; so do a window whose first and last records are filtered out and
    one with no kept read."""
    cfg = _cfg()
    aln, lens = _edge_batch()
    ref = _Ref(oracle_lib, cfg, LOAD_CFG_SMALL, aln)
    b = ref.b
    assert np.diff(b.win_read_off).tolist() == [32, 32, 0]
    assert np.diff(b.read_call_off.astype(np.int64)).tolist() == lens + lens[::-1]
    assert ref.out.win_n_sites[0] > 0 and ref.out.win_n_sites[1] > 0
    db = gpu_ctx.upload_aln(cfg, aln, LOAD_CFG_SMALL)
    off, gpos, gcat, gfirst, glast = db.debug_calls()
    assert db.n_reads == b.n_reads
    assert db.load_counters()["multi_cm"] >= 7
    assert np.array_equal(off, b.read_call_off)
    co = b.read_call_off.astype(np.int64)
    pos, cat = b.call_pos.copy(), b.call_cat.copy()
    for r in range(b.n_reads):                   # the kernels consume a read's calls sorted by (pos, cat)
        o = np.lexsort((cat[co[r]:co[r + 1]], pos[co[r]:co[r + 1]]))
        pos[co[r]:co[r + 1]] = pos[co[r]:co[r + 1]][o]
        cat[co[r]:co[r + 1]] = cat[co[r]:co[r + 1]][o]
    assert np.array_equal(gpos, pos) and np.array_equal(gcat, cat)
    for w in range(b.n_windows):
        for d in (0, 1):
            real, starts, slen = oracle_lib.window_sites(cfg, b, w, d)
            g_real, g_starts, g_len = db.debug_sites(w, d)
            assert np.array_equal(real, g_real), f"w{w} d{d} sites"
            assert np.array_equal(starts, g_starts), f"w{w} d{d} starts"
            assert np.array_equal(slen, g_len), f"w{w} d{d} lens"
    _compare(ref.out, db.run(), "edges")
    db.free()


def test_slack_is_never_read(gpu_ctx, monkeypatch, mix_ref):
    """The staging arrays start from all-zero bytes and from all-one bytes
    (PF_TEST_STAGE_FILL): a kernel that read a slot outside a read's range
    would see a call at position 0 in one run and at 2^32 - 1 in the other.
    Every field of the result and both directions' methmer lists are the same
    in the two runs and equal the oracle's."""
    res = []
    for fill in ("0", "255"):
        monkeypatch.setenv("PF_TEST_STAGE_FILL", fill)
        db = gpu_ctx.upload_aln(mix_ref.cfg, mix_ref.aln, mix_ref.lcfg)
        mm = _methmers(db)
        out = db.run()
        db.free()
        _compare_methmers(mix_ref, mm, f"fill {fill}")
        _compare(mix_ref.out, out, f"fill {fill}")
        res.append((mm, out))
    (mm0, out0), (mm1, out1) = res
    for f in ALL_FIELDS:
        assert np.array_equal(getattr(out0, f), getattr(out1, f)), f
    for d in (0, 1):
        for a, g in zip(mm0[d], mm1[d]):
            assert np.array_equal(a, g), f"methmers d{d}"


def test_two_runs_in_flight(gpu_ctx, monkeypatch, mix_ref):
    """launch, launch, finish, finish on one record-level batch, the two
    heaviest greedy problems on the second stream: the second run's K0
    rewrites the staging arrays only after the first run's kernels have read
    them, and both results equal run()'s (and the oracle's)."""
    monkeypatch.setenv("PF_K3_HEAVY", "2")
    db = gpu_ctx.upload_aln(mix_ref.cfg, mix_ref.aln, mix_ref.lcfg)
    want = db.run()
    _compare(mix_ref.out, want, "run")
    db.launch()
    db.launch()
    o1 = db.finish()
    o2 = db.finish()
    for tag, o in (("first", o1), ("second", o2)):
        for f in ALL_FIELDS:
            assert np.array_equal(getattr(want, f), getattr(o, f)), f"{tag}: {f}"
    db.free()
