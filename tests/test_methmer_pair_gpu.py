"""The fused two-direction methmer core (k2_pair, pf_kernels.hip) against the
oracle on small hand-built windows: every read's methmer list in both
directions, the site arrays, then the window results.

Each case names a situation of the core and asserts, from the oracle's own
site arrays and the batch's calls (`_model` below repeats the range rules of
get_mmr_of_read, blockjoin.c:3375-3391), that its input really contains it.

A window here is: 30 tagged reads left of the gap with one call at position 50
(the coverage check; a read with no call inside the sites' range), two
carrier reads that call every site position methylated / unmethylated (with
cov_for_selection = 1 exactly these positions are sites), and the case's own
reads.  Calls the case adds off the sites are methylated only, so they create
no site.

Two situations the issue lists cannot occur in any input, and the cases say
why instead of testing them:
  * "the last entry's start is above the read's last call" (usable = E - 1):
    the right bound is xr = lower_bound(starts, L) (or S when L is beyond the
    last start, which is then < L), so every entry's start is < L, and L, the
    last call in array order, is <= the largest call.  test_usable asserts
    that the model finds usable == E for every read and that methmers are
    still cut off at the read's end by e + len <= usable.
  * "each range fits PF_K12_CAP and the union does not": a read reaches the
    fused core only when its bound, (#sites in [F, L]) + 3k + 4, is <=
    PF_K12_CAP, and the union of the two real-index ranges is at most that
    count + k + 2 (a direction-1 start lies at most k sites left of its
    site).  test_union_and_cap runs the batch with PF_K12_CAP at the widest
    union, which sends every read with a larger bound to the fallback kernel
    and keeps the rest in the fused core, and with PF_K12_CAP at the smallest
    and the largest bound of a read.
The build switch PF_K12_PAIR is not readable at run time.
"""
import numpy as np
import pytest

from pomfret_amd.abi import Config, WindowBatch

pytestmark = pytest.mark.gpu

S_GAP, E_GAP = 60, 70
BASE = 1000


def _cfg(k, span):
    return Config(k=k, k_span=span, cov_for_selection=1, cov_for_runtime=2, n_cand=4)


def _window(sites, reads):
    """Reads [(start, end, hp, [(pos, cat), ...])] of one window with the given site positions."""
    far = int(max(sites)) + 1000
    rs = [(10, S_GAP, i % 2, [(50, 0)]) for i in range(30)]
    rs.append((90, far, 254, [(int(p), 0) for p in sites]))
    rs.append((90, far, 254, [(int(p), 1) for p in sites]))
    rs += [(90, far, 254, list(c)) for c in reads]
    return rs


def _batch(windows):
    ro, rstart, rend, hp, co, pos, cat = [0], [], [], [], [0], [], []
    for rs in windows:
        for r in rs:
            rstart.append(r[0]); rend.append(r[1]); hp.append(r[2])
            pos += [c[0] for c in r[3]]
            cat += [c[1] for c in r[3]]
            co.append(len(pos))
        ro.append(len(rstart))
    n = len(windows)
    return WindowBatch(win_start=[S_GAP] * n, win_end=[E_GAP] * n, win_read_off=ro, read_start=rstart,
                       read_end=rend, read_hp=hp, read_call_off=co, call_pos=pos, call_cat=cat)


def _range(st, F, L):
    """[xl, xr) of search_arr on the starts, None where the read has none."""
    S = len(st)
    if S == 0 or F > st[-1] or L < st[0]:
        return None
    lb = int(np.searchsorted(st, F, "left"))
    xl = 0 if F < st[0] else (lb if st[lb] == F else max(lb - 1, 0))
    xr = S if L > st[-1] else int(np.searchsorted(st, L, "left"))
    return (xl, xr) if xl < xr else None


def _model(oracle_lib, cfg, b, w):
    """Per read of window w: dict(F, L, maxcall, ncalls, pos) and per direction rng, E (entries), last_start,
    q (real-index range); plus the window's sp, st1, lens."""
    _, sp, l0 = oracle_lib.window_sites(cfg, b, w, 0)
    _, st1, l1 = oracle_lib.window_sites(cfg, b, w, 1)
    sp, st1 = sp.astype(np.int64), st1.astype(np.int64)
    q1 = np.searchsorted(sp, st1)
    out = []
    co = b.read_call_off.astype(np.int64)
    for r in range(int(b.win_read_off[w]), int(b.win_read_off[w + 1])):
        p = b.call_pos[co[r]:co[r + 1]].astype(np.int64)
        m = dict(ncalls=len(p), pos=p, dirs=[None, None])
        if len(p):
            m.update(F=int(p[0]), L=int(p[-1]), maxcall=int(p.max()))
            for d, st in ((0, sp), (1, st1)):
                rg = _range(st, m["F"], m["L"])
                if rg is None:
                    continue
                xl, xr = rg
                ent = [i for i in range(xl, xr) if not (i > 1 and st[i] == st[i - 1])]
                q = (xl, xr) if d == 0 else (int(q1[xl]), int(q1[xr - 1]) + 1)
                m["dirs"][d] = dict(xl=xl, xr=xr, E=len(ent), q=q,
                                    last_start=int(st[ent[-1]]) if ent else None)
        out.append(m)
    return dict(sp=sp, st1=st1, l0=l0, l1=l1, reads=out)


def _check(oracle_lib, gpu_ctx, cfg, b, tag):
    """test_sites_and_methmers_parity's comparison, then the window results."""
    db = gpu_ctx.upload(cfg, b)
    ro = b.win_read_off
    got = {}
    for d in (0, 1):
        n, st, keys = db.debug_methmers(d)
        got[d] = (n.copy(), st.copy(), keys.copy())
        k0 = 0
        for w in range(b.n_windows):
            for o, g, what in zip(oracle_lib.window_sites(cfg, b, w, d), db.debug_sites(w, d), ("sites", "starts", "lens")):
                assert np.array_equal(o, g), f"{tag} w{w} d{d} {what}"
            on, ost, okeys = oracle_lib.window_methmers(cfg, b, w, d)
            gn = n[ro[w]:ro[w + 1]]
            assert np.array_equal(on, gn), f"{tag} w{w} d{d} mmr_n {np.argwhere(on != gn)[:3].tolist()}"
            assert np.array_equal(ost, st[ro[w]:ro[w + 1]]), f"{tag} w{w} d{d} mmr_start"
            assert np.array_equal(okeys, keys[k0:k0 + len(okeys)]), f"{tag} w{w} d{d} keys"
            k0 += len(okeys)
        assert k0 == len(keys), f"{tag} d{d} key count"
    ref = oracle_lib.methphase(cfg, b, n_threads=4)
    out = db.run()
    for name in ("decision", "dir_table", "dir_join", "dir_which_way", "win_n_sites", "win_n_reads", "read_hp"):
        assert np.array_equal(getattr(ref, name), getattr(out, name)), f"{tag}: {name}"
    np.testing.assert_allclose(out.dir_fisher_p, ref.dir_fisher_p, rtol=1e-6, atol=0, err_msg=tag)
    np.testing.assert_allclose(out.dir_score, ref.dir_score, rtol=1e-6, atol=0, err_msg=tag)
    paths = db.k12_paths().copy()
    db.free()
    return got, paths


def _grid(n, step=100):
    return [BASE + step * i for i in range(n)]


def _clusters(k):
    """Clusters of 1 .. k + 2 sites 10 apart, 10,000 between clusters: with k_span = 10 * (k + 1) the
    lengths run from 1 to k in both directions and direction-1 starts repeat inside every cluster."""
    sites, p = [], BASE
    for n in range(1, k + 3):
        sites += [p + 10 * j for j in range(n)]
        p += 10_000
    return sites


def _random_reads(sites, n, seed, off_site=True):
    """n reads over random site intervals: calls at most of the interval's sites with random categories,
    some methylated calls between sites, first / last calls sometimes off the sites."""
    rng = np.random.default_rng(seed)
    sites = np.asarray(sites)
    reads = []
    for _ in range(n):
        i = int(rng.integers(0, len(sites)))
        j = int(rng.integers(i, len(sites)))
        calls = {int(p): int(rng.integers(0, 2)) for p in sites[i:j + 1] if rng.random() < 0.8}
        if off_site:
            for p in sites[i:j + 1]:
                if rng.random() < 0.2:
                    calls.setdefault(int(p) + int(rng.integers(1, 9)), 0)
            if rng.random() < 0.3:
                calls.setdefault(int(sites[i]) - int(rng.integers(1, 9)), 0)
        reads.append(sorted(calls.items()))
    return reads


# ---------------------------------------------------------------------------
ENDS_SITES = _grid(12)
ENDS_READS = [
    [(900, 0), (1300, 1), (1500, 0), (5000, 0)],          # 0: first call before the first site, last beyond the last
    [(1300, 0), (1400, 1), (1600, 0), (1800, 1)],         # 1: first and last call on a site
    [(1350, 0), (1400, 1), (1600, 0), (1850, 0)],         # 2: first and last call strictly between two sites
    [],                                                   # 3: no call at all
    [(100, 0), (200, 0)],                                 # 4: calls left of every site only
    [(9000, 0), (9100, 0)],                               # 5: calls right of every site only
    [(1200, 1), (1400, 0), (1400, 1), (1700, 0)],         # 6: two calls at one position
    [(1000, 1), (1100, 0)],                               # 7: the range's left end at index 0
    [(2100, 1)],                                          # 8: one call, on the last site
    [(2050, 0), (2100, 0)],                               # 9: first call between the last two sites
]


def test_one_and_two_sites(oracle_lib, gpu_ctx):
    """S = 1 and S = 2: the searches over one- and two-element arrays, ranges [0, 1), [0, 2), [1, 2)."""
    r1 = [[(1000, 0)], [(900, 0), (1100, 0)], [(1000, 1), (1100, 0)], [(950, 0)], [(1050, 0)], []]
    r2 = [[(1000, 0)], [(900, 0), (1200, 0)], [(1000, 1), (1100, 0)], [(1100, 1)], [(950, 0)], [(1050, 0), (1100, 1)], []]
    cfg = _cfg(3, 5000)
    b = _batch([_window([1000], r1), _window([1000, 1100], r2)])
    for w, S in ((0, 1), (1, 2)):
        m = _model(oracle_lib, cfg, b, w)
        assert len(m["sp"]) == S
        rngs = {(d, tuple(x["dirs"][d][k] for k in ("xl", "xr"))) for x in m["reads"] for d in (0, 1) if x["dirs"][d]}
        assert {(0, (0, S)), (1, (0, S))} <= rngs, rngs
    _check(oracle_lib, gpu_ctx, cfg, b, "s1s2")


@pytest.mark.parametrize("env", [{}, {"PF_K12C_MINR": "1"}, {"PF_K12_DENSE": "1"}, {"two_segments": "1"}],
                         ids=["plain", "chunks", "dense", "two_segments"])
def test_range_ends(oracle_lib, gpu_ctx, monkeypatch, env):
    """The rules at the two ends of a read's range (before / on / between sites, beyond / on the last
    site), reads without a range, two calls at one position, and direction-1 starts that repeat from
    index 0 (the i > 1 quirk, the first entry's '-') and in a run of at least 3.  Again in
    pf_k12_chunks, on the dense site path and in a window of two bitmap segments."""
    sites = list(ENDS_SITES)
    two = env.pop("two_segments", None)
    if two:
        sites.append(BASE + 600_000)                      # the calls span more than one 512 Ki segment
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = _cfg(3, 5000)
    reads = [list(r) for r in ENDS_READS]
    reads[0][-1] = (sites[-1] + 2900, 0)                  # beyond the last site, wherever that is
    reads[5] = [(sites[-1] + 4000, 0), (sites[-1] + 4100, 0)]
    b = _batch([_window(sites, reads + _random_reads(sites, 20, 7))])
    m = _model(oracle_lib, cfg, b, 0)
    sp, st1, R = m["sp"], m["st1"], m["reads"][32:]
    assert list(sp) == sites
    assert st1[0] == st1[1] and (st1[:4] == st1[0]).all()                       # run of k + 1 = 4 from index 0
    assert R[0]["F"] < sp[0] and R[0]["L"] > sp[-1] and R[0]["dirs"][0]["xl"] == 0 and R[0]["dirs"][0]["xr"] == len(sp)
    assert R[1]["F"] in sp and R[1]["L"] in sp and R[1]["dirs"][0]["xl"] == 3 and R[1]["dirs"][0]["xr"] == 8
    assert R[2]["F"] not in sp and sp[3] < R[2]["F"] < sp[4] and R[2]["dirs"][0]["xl"] == 3       # the step back
    assert R[2]["L"] not in sp and R[2]["dirs"][0]["xr"] == 9
    assert R[3]["ncalls"] == 0
    assert R[4]["dirs"] == [None, None] and R[5]["dirs"] == [None, None]
    assert (np.diff(R[6]["pos"]) == 0).any()
    # a read whose range covers indices 0 and 1 in direction 1: the duplicated-start fix-up fires
    assert any(x["dirs"][1] and x["dirs"][1]["xl"] == 0 and x["dirs"][1]["xr"] >= 2 for x in R)
    # only one direction has a range (such a read takes the two k2_core calls): read 9's calls lie
    # right of the last direction-1 start
    assert two or (R[9]["dirs"][0] is not None and R[9]["dirs"][1] is None)
    _, paths = _check(oracle_lib, gpu_ctx, cfg, b, "ends")
    if two:
        assert paths[0] == 2
    if env.get("PF_K12_DENSE"):
        assert paths[0] == 3


def test_union_and_cap(oracle_lib, gpu_ctx, monkeypatch):
    """Reads whose direction-1 real range starts left of their direction-0 range (the first call is
    on a site that starts no methmer of direction 1), so the characters span more than either; the
    same batch with PF_K12_CAP at the widest union and at the smallest and largest bound of a read
    (module docstring)."""
    k = 3
    cfg = _cfg(k, 10 * (k + 1))
    sites = _clusters(k)
    reads = [[(sites[2], 0), (sites[4], 1), (sites[8], 0)],          # first call on the 2nd site of a cluster
             [(sites[4], 1), (sites[5], 0), (sites[13], 1)],
             [(sites[7] + 3, 0), (sites[12], 1)]] + _random_reads(sites, 40, 11)
    b = _batch([_window(sites, reads)])
    m = _model(oracle_lib, cfg, b, 0)
    wider = [x for x in m["reads"] if x["dirs"][0] and x["dirs"][1] and x["dirs"][1]["q"][0] < x["dirs"][0]["q"][0]]
    assert len(wider) >= 3
    unions, bounds = [], []
    for x in m["reads"]:
        if x["dirs"][0] and x["dirs"][1]:
            (a0, b0), (a1, b1) = x["dirs"][0]["q"], x["dirs"][1]["q"]
            u = max(b0, b1) - min(a0, a1)
            cnt = int(np.searchsorted(m["sp"], x["L"], "right") - np.searchsorted(m["sp"], x["F"], "left"))
            unions.append(u)
            bounds.append(cnt + 3 * k + 4)
            assert u <= cnt + k + 2 < cnt + 3 * k + 4            # why the union never exceeds PF_K12_CAP
    ref, _ = _check(oracle_lib, gpu_ctx, cfg, b, "union")
    for cap in sorted({max(unions), min(bounds), max(bounds)}):
        monkeypatch.setenv("PF_K12_CAP", str(cap))
        got, _ = _check(oracle_lib, gpu_ctx, cfg, b, f"union/cap{cap}")
        for d in (0, 1):
            for a, g in zip(ref[d], got[d]):
                assert np.array_equal(a, g)


def test_entry_counts(oracle_lib, gpu_ctx):
    """Reads of 63, 64, 65, 128 and 129 entries in each direction: the 64-lane rounds of the entry
    pass and of the emission."""
    cfg = _cfg(3, 5000)
    sites = _grid(140)
    reads = []
    for j in range(58, 136):
        reads.append([(sites[0], j & 1)] + [(sites[i], (i + j) & 1) for i in range(1, j, 2)] + [(sites[j], 1)])
    b = _batch([_window(sites, reads)])
    m = _model(oracle_lib, cfg, b, 0)
    want = {63, 64, 65, 128, 129}
    for d in (0, 1):
        assert want <= {x["dirs"][d]["E"] for x in m["reads"] if x["dirs"][d]}, d
    _check(oracle_lib, gpu_ctx, cfg, b, "entries")


def test_usable(oracle_lib, gpu_ctx):
    """usable = E - (last entry's start > last call).  The model finds the start below the last call
    for every read of every batch of this file's shapes (module docstring: it cannot be otherwise),
    reads whose last call is on a site and beyond it included; methmers are still cut off at the
    read's end (0 < n < E)."""
    cfg = _cfg(3, 5000)
    sites = _grid(30)
    b = _batch([_window(sites, ENDS_READS + _random_reads(sites, 60, 3))])
    m = _model(oracle_lib, cfg, b, 0)
    on_site = beyond = 0
    for x in m["reads"]:
        for d in (0, 1):
            if x["dirs"][d] and x["dirs"][d]["E"]:
                assert x["dirs"][d]["last_start"] < x["L"] <= x["maxcall"]
                on_site += x["L"] in m["sp"]
                beyond += x["L"] > m["sp"][-1]
    assert on_site and beyond
    got, _ = _check(oracle_lib, gpu_ctx, cfg, b, "usable")
    cut = 0
    for d in (0, 1):
        for x, n in zip(m["reads"], got[d][0]):
            if x["dirs"][d]:
                cut += 0 < n < x["dirs"][d]["E"]
    assert cut > 0


@pytest.mark.parametrize("k", [1, 3, 5, 15])
def test_k_and_span(oracle_lib, gpu_ctx, k):
    """k = 1, 3, 5, 15 with a k_span that gives every length from 1 to k in both directions, runs of
    equal direction-1 starts of every length up to k + 1 away from index 0, and reads whose last
    methmers are cut off.  k = 15 fills the 30-bit key window."""
    cfg = _cfg(k, 10 * (k + 1))
    sites = _clusters(k)
    b = _batch([_window(sites, _random_reads(sites, 60, 100 + k, off_site=False) + _random_reads(sites, 40, 200 + k))])
    m = _model(oracle_lib, cfg, b, 0)
    assert set(range(1, k + 1)) <= set(m["l0"].tolist()) and set(range(1, k + 1)) <= set(m["l1"].tolist())
    st1 = m["st1"]
    runs = np.diff(np.flatnonzero(np.r_[True, np.diff(st1) != 0, True]))
    assert runs.max() >= min(k + 1, 3) or k == 1
    if k >= 2:
        assert any(st1[i] == st1[i - 1] and i > 1 for i in range(2, len(st1)))
    got, _ = _check(oracle_lib, gpu_ctx, cfg, b, f"k{k}")
    cut = sum(0 < n < x["dirs"][d]["E"] for d in (0, 1) for x, n in zip(m["reads"], got[d][0]) if x["dirs"][d])
    assert cut > 0 or k == 1                              # k = 1: every length is 1, nothing is cut off
    if k == 15:
        assert int(got[0][2].max()) >= 1 << 28            # a 15-character key's top characters are in use
