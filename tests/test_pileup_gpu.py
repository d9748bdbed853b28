"""Per-haplotype CpG methylation pileup on the device (pf_batch_pileup,
pf_pileup.hip) against one literal numpy reference, _pile_ref.

For record-level inputs the reference's WindowBatch comes from the CPU loader
(oracle load_reads), not from K0, so a K0 error cannot move both sides
together; calls-level inputs are their own reference input.  Counts are
integers: every comparison is exact.
"""
import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig, WindowBatch

from tests._aln_cases import LOAD_CFG_SMALL, HANDMADE, handmade_batch, records_batch, synth_aln

pytestmark = pytest.mark.gpu

TILE = 4096                                  # PF_PILE_TILE's default (pf_device.h)


def _pile_ref(batch: WindowBatch, hp=None):
    """The pileup's semantics, literally: per window, every call entry of
    every read with win_start <= pos < win_end and cat 0 / 1 adds one to
    cnt[pos][h][cat], h = 0 / 1 for tag 0 / 1 and 2 for any other; a position
    with a non-zero counter is a site.  Returns (win_off u64 [W+1], pos u32
    [n], cnt u32 [n, 3, 2])."""
    hp = np.asarray(batch.read_hp if hp is None else hp, np.uint8)
    assert hp.size == batch.n_reads
    win_off, pos, cnt = [0], [], []
    for w in range(batch.n_windows):
        ws, we = int(batch.win_start[w]), int(batch.win_end[w])
        dense = np.zeros((max(we - ws, 0), 3, 2), np.uint32)
        for r in range(int(batch.win_read_off[w]), int(batch.win_read_off[w + 1])):
            c0, c1 = int(batch.read_call_off[r]), int(batch.read_call_off[r + 1])
            h = int(hp[r]) if hp[r] < 2 else 2
            for c in range(c0, c1):
                p, cat = int(batch.call_pos[c]), int(batch.call_cat[c])
                if ws <= p < we and cat < 2:
                    dense[p - ws, h, cat] += 1
        sites = np.flatnonzero(dense.reshape(len(dense), 6).any(axis=1))
        pos.append((sites + ws).astype(np.uint32))
        cnt.append(dense[sites])
        win_off.append(win_off[-1] + len(sites))
    return (np.asarray(win_off, np.uint64), np.concatenate(pos) if pos else np.zeros(0, np.uint32),
            np.concatenate(cnt) if cnt else np.zeros((0, 3, 2), np.uint32))


def _same(got, ref, tag):
    assert np.array_equal(got["win_off"], ref[0]), f"{tag}: win_off {got['win_off'].tolist()[:8]} vs {ref[0].tolist()[:8]}"
    assert np.array_equal(got["pos"], ref[1]), f"{tag}: pos"
    assert got["cnt"].shape == ref[2].shape and np.array_equal(got["cnt"], ref[2]), f"{tag}: cnt"
    for w in range(len(ref[0]) - 1):                 # strictly ascending inside a window
        p = got["pos"][int(got["win_off"][w]):int(got["win_off"][w + 1])].astype(np.int64)
        assert (np.diff(p) > 0).all(), f"{tag}: window {w} not ascending"


def _cfg():
    from pomfret_amd import Config
    return Config.from_coverage(30, given=False)


def _calls_batch(windows):
    """windows: [(s, e, [(hp, [(pos, cat), ...]), ...])] -> a calls-level WindowBatch."""
    ws, we, wro, hp, co, cp, cc = [], [], [0], [], [0], [], []
    for s, e, reads in windows:
        ws.append(s)
        we.append(e)
        for h, calls in reads:
            hp.append(h)
            for p, c in sorted(calls):
                cp.append(p)
                cc.append(c)
            co.append(len(cp))
        wro.append(len(hp))
    R = len(hp)
    return WindowBatch(win_start=ws, win_end=we, win_read_off=wro, read_start=np.zeros(R), read_end=np.ones(R),
                       read_hp=hp, read_call_off=co, call_pos=cp, call_cat=cc)


# ---- 1. hand-worked -------------------------------------------------------
def test_hand_worked_three_reads(gpu_ctx, tmp_path):
    """Forward read (hp 0), reverse read (hp 1) over the same two CpGs, and an
    untagged read one CpG further right.  ACGTTCGA has its CpG C's at offsets
    1 and 5; a reverse read's ML values run from the read's end (HANDMADE
    "rev"), so ml [50, 220] puts 220 on the left CpG.  ML 200 / 220 are meth
    (>= 156), 10 / 50 unmeth (< 100), 130 a no-call.

        pos 101: A meth (h1), B meth (h2)
        pos 105: A unmeth (h1), B unmeth (h2), C no-call (counts nowhere)
        pos 109: C meth (other)
    """
    from pomfret_amd.pipeline import write_hapmeth
    A = dict(seq="ACGTTCGA", cigar="8M", mm="C+m?,0,0;", ml=[200, 10], pos=100, hp=0)
    B = dict(seq="ACGTTCGA", cigar="8M", mm="C+m?,0,0;", ml=[50, 220], pos=100, flag=16, hp=1)
    Cr = dict(seq="ACGTTCGA", cigar="8M", mm="C+m?,0,0;", ml=[130, 220], pos=104, hp=254)
    db = gpu_ctx.upload_aln(_cfg(), records_batch([(100, 110, [A, B, Cr])]), LOAD_CFG_SMALL)
    got = db.pileup()
    db.free()
    assert got["win_off"].tolist() == [0, 3]
    assert got["pos"].tolist() == [101, 105, 109]
    assert got["cnt"].reshape(3, 6).tolist() == [[1, 0, 1, 0, 0, 0], [0, 1, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0]]
    assert got["ms"] > 0
    out = str(tmp_path / "h.bed")
    write_hapmeth(out, "chrT", got, header=False)
    assert open(out).read() == ("chrT\t101\t102\t1\t0\t1\t0\t0\t0\t1\n"
                                "chrT\t105\t106\t0\t1\t0\t1\t0\t0\t1\n"
                                "chrT\t109\t110\t0\t0\t0\t0\t1\t0\t1\n")


@pytest.mark.parametrize("win", [(0, 10), (0, 1200)])
def test_handmade_records(gpu_ctx, oracle_lib, win):
    """Every hand-made loader record; (0, 10) is handmade_batch()'s own window
    (no call lies inside: an empty, valid result), (0, 1200) holds them all."""
    aln = handmade_batch() if win == (0, 10) else records_batch([(win[0], win[1], [r for _, r, _ in HANDMADE])])
    ref_b, _ = oracle_lib.load_reads(LOAD_CFG_SMALL, aln)
    ref = _pile_ref(ref_b)
    assert (len(ref[1]) == 0) == (win == (0, 10))
    db = gpu_ctx.upload_aln(_cfg(), aln, LOAD_CFG_SMALL)
    _same(db.pileup(), ref, f"handmade {win}")
    db.free()


# ---- 2. window and tile edges ---------------------------------------------
def _edge_batch():
    s = 1000
    e = s + 2 * TILE + 808                       # three default tiles, the last one short
    offs = [63, 64, 127, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE]   # tile offsets T-1, T, 2T-1 for T = 64 and 4096
    r0 = [(s - 1, 0), (s, 0), (e - 1, 1), (e, 0)] + [(s + o, 0) for o in offs] + [(2000, 2)]
    r1 = [(s, 1), (e - 1, 1), (2000, 2), (s + TILE - 1, 2), (s + TILE, 1), (s + 2 * TILE - 1, 0)]
    outside = [(5, 0), (s - 1, 1), (e, 1), (e + 70000, 0)]
    return _calls_batch([
        (s, e, [(0, r0), (1, r1), (0, []), (254, outside), (7, [(s + 64, 1), (s + 64, 1)])]),
        (50, 51, [(1, [(49, 0), (50, 0), (51, 0)]), (0, [(50, 2)])]),     # a window of length 1
        (0, 100000, []),                                                  # no reads
        (300, 400, [(0, [(350, 2)]), (1, [(350, 2), (10, 0)])]),          # only no-calls inside: no site
        (7, 7, [(0, [(7, 0)])]),                                          # an empty range
    ])


@pytest.mark.parametrize("tile", [None, 64])
def test_edges(gpu_ctx, monkeypatch, tile):
    if tile:
        monkeypatch.setenv("PF_PILE_TILE", str(tile))
    b = _edge_batch()
    ref = _pile_ref(b)
    s, e = int(b.win_start[0]), int(b.win_end[0])
    w0 = ref[1][:int(ref[0][1])].tolist()
    assert s in w0 and e - 1 in w0 and s - 1 not in w0 and e not in w0 and 2000 not in w0
    assert ref[0].tolist()[1:] == [len(w0), len(w0) + 1, len(w0) + 1, len(w0) + 1, len(w0) + 1]
    db = gpu_ctx.upload(_cfg(), b)
    _same(db.pileup(), ref, f"edges tile {tile}")
    db.free()


def test_no_windows(gpu_ctx):
    db = gpu_ctx.upload(_cfg(), _calls_batch([]))
    got = db.pileup()
    db.free()
    assert got["win_off"].tolist() == [0] and got["pos"].size == 0 and got["cnt"].shape == (0, 3, 2)


def test_bad_tile_is_refused(gpu_ctx, monkeypatch):
    from pomfret_amd import PomfretError
    db = gpu_ctx.upload(_cfg(), _calls_batch([(0, 10, [(0, [(1, 0)])])]))
    for bad in ("96", "32", "16384", "64x"):
        monkeypatch.setenv("PF_PILE_TILE", bad)
        with pytest.raises(PomfretError):
            db.pileup()
    db.free()


# ---- 3. one record in two adjacent windows --------------------------------
def test_record_in_two_windows(gpu_ctx, oracle_lib):
    rec = dict(seq="ACGTTCGAACGTACG", cigar="15M", mm="C+m?,0,0,0,0;", ml=[200, 10, 220, 30], pos=100, hp=1)
    two = records_batch([(100, 107, [rec]), (107, 120, [rec])])
    one = records_batch([(100, 120, [rec])])
    ctx = gpu_ctx
    res = []
    for aln in (two, one):
        ref_b, _ = oracle_lib.load_reads(LOAD_CFG_SMALL, aln)
        db = ctx.upload_aln(_cfg(), aln, LOAD_CFG_SMALL)
        got = db.pileup()
        db.free()
        _same(got, _pile_ref(ref_b), "two windows")
        res.append(got)
    g2, g1 = res
    assert g1["pos"].tolist() == [101, 105, 109, 113]
    k = int(g2["win_off"][1])
    left, right = g2["pos"][:k], g2["pos"][k:]
    assert left.size and right.size and left.max() < 107 <= right.min()
    assert not set(left.tolist()) & set(right.tolist())
    assert np.array_equal(g2["pos"], g1["pos"]) and np.array_equal(g2["cnt"], g1["cnt"])


# ---- 4. counter width ------------------------------------------------------
def test_counter_width(gpu_ctx):
    """300 reads (past 8 bits) and 65,535 reads (the documented limit of reads
    per window, the 16-bit field's maximum) on one position and haplotype."""
    b = _calls_batch([(10, 20, [(0, [(15, 0)])] * 300), (10, 20, [(1, [(12, 1)])] * 65535)])
    db = gpu_ctx.upload(_cfg(), b)
    got = db.pileup()
    db.free()
    assert got["win_off"].tolist() == [0, 1, 2] and got["pos"].tolist() == [15, 12]
    assert got["cnt"].reshape(2, 6).tolist() == [[300, 0, 0, 0, 0, 0], [0, 0, 0, 65535, 0, 0]]


def test_counter_wrap_is_an_error(gpu_ctx):
    """Duplicate entries can pass 65,535: never a wrapped value."""
    from pomfret_amd import PomfretError
    b = _calls_batch([(10, 20, [(0, [(15, 0), (15, 0)])] * 32768)])
    db = gpu_ctx.upload(_cfg(), b)
    with pytest.raises(PomfretError, match="limit"):
        db.pileup()
    db.free()


# ---- 5. synthetic batches, 7. tile invariance -----------------------------
@pytest.fixture(scope="module")
def aln_case(oracle_lib):
    aln = synth_aln(3, 30, 91)
    ref_b, _ = oracle_lib.load_reads(LoadConfig(), aln)
    return aln, ref_b, _pile_ref(ref_b)


@pytest.fixture(scope="module")
def calls_case():
    from pomfret_amd.synth import SynthSpec, make_batch
    b = make_batch(SynthSpec(n_windows=4, coverage=60))
    assert int((b.win_end - b.win_start).min()) > 2 * TILE       # several tiles per window
    return b, _pile_ref(b)


def test_synth_record_level(gpu_ctx, aln_case):
    aln, ref_b, ref = aln_case
    assert len(ref[1]) > 1000
    db = gpu_ctx.upload_aln(_cfg(), aln, LoadConfig())
    _same(db.pileup(), ref, "synth_aln(3, 30, 91)")
    db.free()


def test_synth_calls_level(gpu_ctx, calls_case):
    b, ref = calls_case
    assert len(ref[1]) > 1000
    db = gpu_ctx.upload(_cfg(), b)
    _same(db.pileup(), ref, "make_batch 60x")
    db.free()


def test_tile_invariance(gpu_ctx, aln_case, calls_case, monkeypatch):
    aln, _, ref_a = aln_case
    b, ref_c = calls_case
    dba = gpu_ctx.upload_aln(_cfg(), aln, LoadConfig())
    dbc = gpu_ctx.upload(_cfg(), b)
    base = None
    for tile in (None, 64, 1024):
        if tile:
            monkeypatch.setenv("PF_PILE_TILE", str(tile))
        got = [dba.pileup(), dbc.pileup()]
        _same(got[0], ref_a, f"record level, tile {tile}")
        _same(got[1], ref_c, f"calls level, tile {tile}")
        blob = [g[k].tobytes() for g in got for k in ("win_off", "pos", "cnt")]
        if base is None:
            base = blob
        assert blob == base, f"tile {tile}"
    dba.free()
    dbc.free()


# ---- 6. read_hp override ---------------------------------------------------
def test_read_hp_override_calls_level(gpu_ctx):
    from pomfret_amd import PomfretError
    from pomfret_amd.synth import SynthSpec, make_batch
    b = make_batch(SynthSpec(n_windows=4, coverage=30, seed=5))
    db = gpu_ctx.upload(_cfg(), b)
    res = db.run()
    assert (res.read_hp != b.read_hp).any(), "the run re-tagged no read: pick another batch"
    own = db.pileup()
    new = db.pileup(read_hp=res.read_hp)
    _same(own, _pile_ref(b), "own tags")
    _same(new, _pile_ref(b, res.read_hp), "the run's tags")
    assert not np.array_equal(own["cnt"], new["cnt"])
    res2 = db.run()
    for f in ("decision", "read_hp", "dir_table", "dir_join", "dir_which_way", "dir_fisher_p", "dir_score",
              "win_n_sites", "win_n_reads"):
        assert np.array_equal(getattr(res, f), getattr(res2, f)), f
    for n in (b.n_reads - 1, b.n_reads + 1, 0):
        with pytest.raises(PomfretError):
            db.pileup(read_hp=np.zeros(n, np.uint8))
    db.free()


def test_read_hp_override_record_level(gpu_ctx, aln_case):
    from pomfret_amd import PomfretError
    aln, ref_b, ref = aln_case
    db = gpu_ctx.upload_aln(_cfg(), aln, LoadConfig())
    res = db.run()
    assert res.read_hp.size == ref_b.n_reads
    _same(db.pileup(read_hp=res.read_hp), _pile_ref(ref_b, res.read_hp), "the run's tags")
    _same(db.pileup(), ref, "own tags after a run")
    res2 = db.run()
    for f in ("decision", "read_hp", "dir_table", "win_n_sites", "win_n_reads"):
        assert np.array_equal(getattr(res, f), getattr(res2, f)), f
    with pytest.raises(PomfretError):
        db.pileup(read_hp=np.zeros(aln.n_recs + 1, np.uint8))
    db.launch()
    with pytest.raises(PomfretError):                # a launched run is unfinished
        db.pileup()
    db.finish()
    db.free()
