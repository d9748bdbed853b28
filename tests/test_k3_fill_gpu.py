"""The greedy kernel's term fill, insert and cache copy at the sizes where
their wave-uniform bounds change, against the CPU oracle.

The term fill deals G = 64 / next_pow2(nc) lanes of each wave to a candidate
and runs as many slots of GS = 4 G methmers as the iteration's longest
in-range span needs, four at a time and then two and one: the windows here
put that longest span one below, at and one above GS, 4 GS and 8 GS for every
listed n_cand.  The insert of the winner and the copy of a list into the
candidate cache mask the lanes past the list's length, 256 threads a round:
two windows hold lists of 1, 63, 64, 65, 255, 256, 257 and 513 methmers (a
wave with no lane, with one lane, and a second round).

Every window is built so that the reference reads of both sides cover every
site cov_for_runtime times: the in-range sites are then [0, n_sites - 1) in
both directions from the first iteration to the last (update_range stops at
the last site's index), and a read's span is its methmer list cut there.  Each
case checks that on the CPU, from the oracle's site and methmer lists, before
anything runs on the device.
"""
import numpy as np
import pytest

from pomfret_amd.abi import Config, WindowBatch

pytestmark = pytest.mark.gpu

K = 3
COV = 2
N_REF = 8
NCANDS = [1, 2, 3, 5, 8, 9, 15, 16, 17, 33, 64]
INSERT_LENS = [1, 63, 64, 65, 255, 256, 257, 513]
ENVS = {"default": {},
        "cache": {"PF_K3_CACHE": "force"},
        "cache_gcnt": {"PF_K3_CACHE": "force", "PF_K3_GCNT": "force"},
        "fold": {"PF_K3_PATH": "fold"},
        "heavy": {"PF_K3_HEAVY": "64"}}
S, E, SITE0, STEP = 100_000, 190_000, 100_500, 40


def _next_pow2(x):
    return 1 if x <= 1 else 1 << (x - 1).bit_length()


def slot_span(n_cand):
    """Methmers one slot covers per candidate over the four waves."""
    return 4 * (64 // _next_pow2(n_cand))


def fill_targets(n_cand):
    gs = slot_span(n_cand)
    return [m * gs + d for m in (1, 4, 8) for d in (-1, 0, 1)]


def _cfg(n_cand):
    return Config(k=K, k_span=5000, cov_for_selection=COV, cov_for_runtime=COV, n_cand=n_cand, hard_cov=N_REF)


def _window(rng, n_sites, lists, n_ref=N_REF):
    """Reads of one window over n_sites sites STEP apart.  n_ref reference
    reads per haplotype and side call every site (hap h reads the site's
    pattern bit xor h); `lists` gives the untagged reads as (first site,
    number of methmers): such a read calls the n + K sites from `first` on,
    which gives it n methmers in either direction as long as it stays four
    sites off both ends; its haplotype's pattern with one call in eight
    flipped."""
    pos = SITE0 + STEP * np.arange(n_sites)
    assert pos[-1] < E - 1000
    meth = rng.integers(0, 2, n_sites)
    reads = []

    def ref(start, end, h):
        reads.append((start, end, h, [(int(pos[j]), int(meth[j] ^ h)) for j in range(n_sites)]))

    for i in range(2 * n_ref):                       # left references: start <= S
        ref(S - 40_000 + i, E + 5_000, i % 2)
    mids = []
    for first, n in lists:
        h = int(rng.integers(0, 2))
        last = first + n + K - 1
        assert (first >= 4 and last < n_sites - 4) or (first == 0 and last == n_sites - 1)
        flip = rng.random(last + 1 - first) < 0.125
        calls = [(int(pos[j]), int(meth[j] ^ h ^ int(flip[j - first]))) for j in range(first, last + 1)]
        mids.append((S + 100 + len(mids), E + 6_000 + len(mids), 254, calls))
    reads += mids
    for i in range(2 * n_ref):                       # right references: start > S, end >= E
        ref(S + 20_000 + i, E + 8_000 + i, i % 2)
    return reads


def _batch(windows):
    reads = [r for w in windows for r in w]
    return WindowBatch(
        win_start=[S] * len(windows), win_end=[E] * len(windows),
        win_read_off=np.concatenate([[0], np.cumsum([len(w) for w in windows])]),
        read_start=[r[0] for r in reads], read_end=[r[1] for r in reads], read_hp=[r[2] for r in reads],
        read_call_off=np.cumsum([0] + [len(r[3]) for r in reads]),
        call_pos=[c[0] for r in reads for c in r[3]], call_cat=[c[1] for r in reads for c in r[3]])


def fill_batches(n_cand):
    """Two batches (six and three windows): window i's untagged reads have
    spans of at most fill_targets(n_cand)[i], the first two and the last two
    reads (the first candidates of either direction) exactly that."""
    rng = np.random.default_rng(1000 + n_cand)
    n_mid = n_cand + 6
    wins = []
    for t in fill_targets(n_cand):
        if n_cand == 1:
            # the library runs n_cand 1 as 2 (the reference's clamp), so one
            # candidate is what the last iteration of a direction holds when
            # every read before it was tagged: every read of these windows,
            # reference or not, spans all t in-range sites of direction 0
            # (t + 1 of direction 1, whose range is one site longer)
            wins.append(_window(rng, t + 2, [(0, t + 2 - K)] * n_mid))
            continue
        n_sites = t + K + 16
        lists = []
        for i in range(n_mid):
            if i < 2 or i >= n_mid - 2 or t < 3:
                n = t
            else:
                n = int(rng.integers(max(1, t // 3), t + 1))
            lists.append((int(rng.integers(4, n_sites - 4 - (n + K) + 1)), n))
        wins.append(_window(rng, n_sites, lists))
    return [(fill_targets(n_cand)[:6], _batch(wins[:6])), (fill_targets(n_cand)[6:], _batch(wins[6:]))]


INSERT_SHORT = [n for n in INSERT_LENS if n <= 257]


def insert_batch():
    """Two windows whose untagged reads have the INSERT_LENS list lengths (each
    twice, in both orders) and a few ordinary ones: window 0 the lengths up to
    257 over so few sites that no list, a reference read's included, passes
    the candidate cache's 512 entries; window 1 all of them up to 513, which
    the cache cannot take."""
    rng = np.random.default_rng(77)
    wins = []
    for lens in (INSERT_SHORT, INSERT_LENS):
        n_sites = max(lens) + K + 16
        lens = lens + [40, 90] + lens[::-1]
        lists = [(int(rng.integers(4, n_sites - 4 - (n + K) + 1)), n) for n in lens]
        wins.append(_window(rng, n_sites, lists))
    return _batch(wins)


def spans(oracle_lib, cfg, batch, w, d):
    """(per-read list length, per-read in-range span) of window w in
    direction d from the oracle's site and methmer lists.  The range is the
    one the direction's reference reads open (haplotag_region1's start and
    update_range, restated); no other read's insert can widen it, which is
    checked: no read covers a site at or past its end, and it starts at 0."""
    real, _, _ = oracle_lib.window_sites(cfg, batch, w, d)
    n, st, _ = oracle_lib.window_methmers(cfg, batch, w, d)
    ro = batch.win_read_off
    hp = np.asarray(batch.read_hp)[ro[w]:ro[w + 1]]
    ns = len(real)
    assert ns > 1 and real[0] > S and real[-1] <= E
    n, st = n.astype(np.int64), st.astype(np.int64)
    mid = np.flatnonzero(hp == 254)
    refs = range(0, mid[0]) if d == 0 else range(mid[-1] + 1, len(hp))
    cover = np.zeros(ns, np.int64)
    for r in refs:
        assert hp[r] in (0, 1) and n[r] > 0
        cover[st[r]:min(st[r] + n[r], ns)] += 1
    lo = hi = 0 if d == 0 else ns - 1
    for i in range(lo, -1, -1):
        if cover[i] < cfg.cov_for_runtime:
            break
        lo = i
    for i in range(hi, ns):
        if cover[i] < cfg.cov_for_runtime:
            break
        hi = i
    assert lo == 0 and hi >= ns - 2, (lo, hi, ns)
    assert hi == ns - 1 or (st + n).max() <= hi + 1, "a later insert could widen the range"
    a, b = np.maximum(st, lo), np.minimum(st + n, hi)
    return n, np.where((n > 0) & (b > a), b - a, 0)


_REFS = {}


def _ref(oracle_lib, key, cfg, batch):
    if key not in _REFS:
        _REFS[key] = oracle_lib.methphase(cfg, batch, n_threads=8)
    return _REFS[key]


def _compare(ref, out, tag):
    for name in ("decision", "dir_table", "dir_join", "dir_which_way", "win_n_sites", "win_n_reads", "read_hp"):
        a, g = getattr(ref, name), getattr(out, name)
        assert np.array_equal(a, g), f"{tag}: {name} differs at {np.argwhere(a != g)[:5].tolist()}"
    np.testing.assert_allclose(out.dir_fisher_p, ref.dir_fisher_p, rtol=1e-6, atol=0, err_msg=tag)
    np.testing.assert_allclose(out.dir_score, ref.dir_score, rtol=1e-6, atol=0, err_msg=tag)


_LONGEST = {}


def _longest_lists(oracle_lib, key, cfg, batch):
    """Per window, the longest methmer list of any read in either direction."""
    if key not in _LONGEST:
        _LONGEST[key] = [max(int(oracle_lib.window_methmers(cfg, batch, w, d)[0].max()) for d in (0, 1))
                         for w in range(batch.n_windows)]
    return _LONGEST[key]


def _run(oracle_lib, gpu_ctx, monkeypatch, envname, key, cfg, batch):
    for k in ("PF_K3_CACHE", "PF_K3_GCNT", "PF_K3_PATH", "PF_K3_HEAVY", "PF_K3_LDS", "PF_K3_LDS_FB", "PF_K3_IMPL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[envname].items():
        monkeypatch.setenv(k, v)
    ref = _ref(oracle_lib, key, cfg, batch)
    db = gpu_ctx.upload(cfg, batch)
    out = db.run()
    paths = db.k3_paths()
    iters = db.stats()[:, :, 2]
    heavy = set(db.heavy_problems().tolist())
    db.free()
    tag = f"{key}/{envname}"
    print(tag, "paths", paths.tolist(), "iters", iters.tolist(), "heavy", sorted(heavy))
    _compare(ref, out, tag)
    assert (iters >= 1).all(), (tag, iters.tolist())          # no window degenerated into a skip
    # the intended path (k3_run): the slim loop with the slot lists from
    # wherever they fit (1 LDS, 2 cache, 3 HBM) by default, and in pf_k3_heavy;
    # with the cache forced, the cache (2, or 6 with the counts in HBM) for a
    # window it can take -- at most 63 candidates and no list past 512 entries
    # -- and the HBM lists (3) for the others; the general body (4) for the
    # fold.  These windows are far below every LDS budget.
    every = {(w << 1) | d for w in range(batch.n_windows) for d in (0, 1)}
    assert heavy == (every if envname == "heavy" else set()), (tag, heavy)
    for w, longest in enumerate(_longest_lists(oracle_lib, key, cfg, batch)):
        cache_ok = cfg.n_cand <= 63 and longest <= 512
        want = {"default": {1, 2, 3}, "heavy": {1, 2, 3}, "fold": {4}, "cache": {2} if cache_ok else {3},
                "cache_gcnt": {6} if cache_ok else {3}}[envname]
        assert set(paths[w].tolist()) <= want, (tag, w, paths[w].tolist(), want)


def check_fill_case(oracle_lib, n_cand, targets, batch):
    """The oracle alone: in each window and direction there are at least
    n_cand untagged reads (so nc = n_cand in the first iteration), the first
    n_cand candidates hold a read whose span is the target, and no untagged
    read between the references has a longer one.  n_cand 1 (run as 2): every
    candidate of direction 0 spans the target and every one is tagged, so the
    direction's last iteration has that span with one candidate."""
    cfg = _cfg(n_cand)
    ro = batch.win_read_off
    counts = oracle_lib.trace(cfg, batch)[3]
    for w, t in enumerate(targets):
        hp = np.asarray(batch.read_hp)[ro[w]:ro[w + 1]]
        mid = np.flatnonzero(hp == 254)
        assert len(mid) >= max(n_cand, 2)
        for d in (0, 1):
            n, sp = spans(oracle_lib, cfg, batch, w, d)
            assert counts[w, d] >= 1
            if n_cand == 1:
                if d == 0:
                    cand = np.arange(mid[0], len(hp))
                    assert (sp[cand] == t).all(), (w, t, sp[cand].tolist())
                    assert counts[w, d] == len(cand), (w, counts[w, d], len(cand))
                continue
            assert sp[mid].max() == t, (n_cand, w, d, t, sp[mid].tolist())
            first = mid[:n_cand] if d == 0 else mid[::-1][:n_cand]
            assert sp[first].max() == t, (n_cand, w, d, t, sp[first].tolist())


def check_insert_case(oracle_lib, batch):
    """The oracle alone: every intended length is some untagged read's list
    in both directions, those that can win (three methmers or more: a shorter
    list never passes the pick's rule) were tagged, so inserted, and window
    0's longest list fits the candidate cache while window 1's does not."""
    cfg = _cfg(8)
    ro = batch.win_read_off
    ids, _, _, counts = oracle_lib.trace(cfg, batch)
    for w, lens in enumerate((INSERT_SHORT, INSERT_LENS)):
        hp = np.asarray(batch.read_hp)[ro[w]:ro[w + 1]]
        for d in (0, 1):
            n, sp = spans(oracle_lib, cfg, batch, w, d)
            have = set(n[hp == 254].tolist())
            assert set(lens) <= have, (w, d, sorted(have))
            won = set(n[ids[w, d, :counts[w, d]]].tolist())
            assert set(lens) - {1} <= won, (w, d, sorted(won))
            assert (n.max() <= 512) == (w == 0), (w, d, int(n.max()))


_FILL = {}


def _fill(n_cand):
    if n_cand not in _FILL:
        _FILL[n_cand] = fill_batches(n_cand)
    return _FILL[n_cand]


@pytest.mark.parametrize("envname", list(ENVS))
@pytest.mark.parametrize("n_cand", NCANDS)
def test_fill_span_boundaries(oracle_lib, gpu_ctx, monkeypatch, n_cand, envname):
    cfg = _cfg(n_cand)
    for i, (targets, batch) in enumerate(_fill(n_cand)):
        check_fill_case(oracle_lib, n_cand, targets, batch)
        _run(oracle_lib, gpu_ctx, monkeypatch, envname, f"fill{n_cand}.{i}", cfg, batch)


@pytest.mark.parametrize("envname", list(ENVS))
def test_insert_and_cache_copy_boundaries(oracle_lib, gpu_ctx, monkeypatch, envname):
    batch = insert_batch()
    check_insert_case(oracle_lib, batch)
    _run(oracle_lib, gpu_ctx, monkeypatch, envname, "insert", _cfg(8), batch)
