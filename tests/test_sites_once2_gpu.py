"""Pass A of K12's fast sites path (pf_kernels.hip: one atomic on the seen-once bitmap per call, one
on the seen-twice bitmap per repeated call) at the edges of its bitmap words and segments, against
the oracle: the site arrays of every window and win_n_sites.  Written with a variant of the pass
that kept the two bits of a position side by side in one word, 32 positions per word
(profiles/k12_siteside/README.md: measured and not kept); the cases hold for either layout.

A window's bitmap starts at its smallest call position P0, so a position's segment offset is pos -
P0; offsets 31 | 32 and 63 | 64 are the edges of 32- and of 64-position bitmap words,
524,287 the last position of segment 1 and 524,288 the first of segment 2 (every window here takes
two segments).  Each window puts one pattern of calls on all of these offsets:

  once      one methylated call: seen once, never a site
  twice     one methylated and one unmethylated call: a site when cov_for_selection is 1
  cat2      two category-2 calls and nothing else: skipped by every pass, no site
  short     cov_sel methylated and cov_sel - 1 unmethylated calls: no site
  full      cov_sel calls of each kind: a site

and has anchor sites of its own (cov_sel calls of each kind) elsewhere.  The 30 tagged reads left of
the gap each call offset 1,000 methylated: a repeated position that is no site.
"""
import numpy as np
import pytest

from pomfret_amd.abi import Config, WindowBatch

pytestmark = pytest.mark.gpu

P0 = 5_000
SEG = 524_288
OFFS = (0, 31, 32, 63, 64, SEG - 1, SEG)
ANCHORS = (100, 200, 300_000, 400_000)
S_GAP, E_GAP = 60, 70
PATTERNS = ("once", "twice", "cat2", "short", "full")


def _cfg(cov_sel):
    return Config(k=3, k_span=5000, cov_for_selection=cov_sel, cov_for_runtime=2, n_cand=4)


def _pattern_reads(pat, c):
    """The pattern's reads: each calls every offset of OFFS with one category."""
    cats = {"once": [0], "twice": [0, 1], "cat2": [2, 2], "short": [0] * c + [1] * (c - 1), "full": [0] * c + [1] * c}[pat]
    return [[(P0 + o, cat) for o in OFFS] for cat in cats]


def _window(reads, c):
    """30 tagged reads left of the gap, cov_sel carrier reads of each kind on the anchors, the reads."""
    far = P0 + SEG + 1000
    rs = [(10, S_GAP, i % 2, [(P0 + 1000, 0)]) for i in range(30)]
    for cat in (0, 1):
        rs += [(90, far, 254, [(P0 + a, cat) for a in ANCHORS]) for _ in range(c)]
    rs += [(90, far, 254, list(r)) for r in reads]
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


def _expected(pat, c):
    """The window's sites by the rule: the anchors, and the offsets where the pattern qualifies."""
    on = pat == "full" or (pat == "twice" and c == 1)
    return sorted(P0 + a for a in ANCHORS + (OFFS if on else ()))


def _check_sites(oracle_lib, db, cfg, b, want, tag):
    out = db.run()
    ref = oracle_lib.methphase(cfg, b, n_threads=4)
    assert np.array_equal(out.win_n_sites, ref.win_n_sites), f"{tag}: win_n_sites {out.win_n_sites} {ref.win_n_sites}"
    for w in range(b.n_windows):
        for d in (0, 1):
            for o, g, what in zip(oracle_lib.window_sites(cfg, b, w, d), db.debug_sites(w, d, cap=1 << 12),
                                  ("sites", "starts", "lens")):
                assert np.array_equal(o, g), f"{tag} w{w} d{d} {what}: {g.tolist()} != {o.tolist()}"
        if want is not None:
            assert db.debug_sites(w, 0, cap=1 << 12)[0].tolist() == want[w], f"{tag} w{w}"
    assert np.array_equal(out.decision, ref.decision), tag
    return out


@pytest.mark.parametrize("cov_sel", [1, 2, 3])
def test_patterns_at_word_and_segment_edges(oracle_lib, gpu_ctx, cov_sel):
    """One window per pattern, all in one batch: the sites are the oracle's and are the anchors plus,
    for the patterns that qualify, every edge offset; every window took two segments."""
    cfg = _cfg(cov_sel)
    b = _batch([_window(_pattern_reads(p, cov_sel), cov_sel) for p in PATTERNS])
    db = gpu_ctx.upload(cfg, b)
    try:
        _check_sites(oracle_lib, db, cfg, b, [_expected(p, cov_sel) for p in PATTERNS], f"cov{cov_sel}")
        assert db.k12_paths().tolist() == [2] * len(PATTERNS)
    finally:
        db.free()


def test_two_short_reads_in_one_lane_group(oracle_lib, gpu_ctx):
    """Two reads of 20 calls at the same 20 positions, one methylated and one unmethylated, 16 reads
    apart: K12's wave 14 walks the window's reads 14, 30 and 46.  A 64-lane group of k12_each_call
    holds the rest of one read and the first calls of the next, so read 14 is given exactly 64 calls
    (one whole group) and reads 30 and 46 share the next one: the two calls of a position reach
    its word in one instruction.  With cov_for_selection = 1 all 20 positions are sites."""
    pos = [P0 + o for o in OFFS[:5]] + [P0 + 71 + 3 * i for i in range(13)] + [P0 + o for o in OFFS[5:]]
    assert len(pos) == 20 and pos == sorted(pos)
    far = P0 + SEG + 1000
    rs = _window([], 1)
    assert len(rs) == 32
    rs[14] = (10, S_GAP, 0, [(P0 + 1000 + i, 0) for i in range(64)])
    # reads 33 .. 45 and 47: no calls
    rs = rs[:30] + [(90, far, 254, [(p, 0) for p in pos])] + rs[30:] + [(90, far, 254, [])] * 13 + \
        [(90, far, 254, [(p, 1) for p in pos])] + [(90, far, 254, [])]
    calls = [len(r[3]) for r in rs]
    assert calls[14] == 64 and calls[30] == calls[46] == 20 and 30 % 16 == 46 % 16 == 14 and len(rs) <= 64
    b = _batch([rs])
    cfg = _cfg(1)
    db = gpu_ctx.upload(cfg, b)
    try:
        _check_sites(oracle_lib, db, cfg, b, [sorted(pos + [P0 + a for a in ANCHORS])], "pair")
        assert db.k12_paths().tolist() == [2]
    finally:
        db.free()


def test_masked_site_at_the_edges(oracle_lib, gpu_ctx):
    """pf_batch_set_mask on qualifying sites at offsets 32 and 524,288: they leave the sites, the
    others stay; the reference is the oracle on the batch whose calls there are no-calls."""
    cfg = _cfg(2)
    b = _batch([_window(_pattern_reads("full", 2), 2)])
    masked = [P0 + 32, P0 + SEG]
    nb = b.select(range(b.n_windows))
    cat = np.array(nb.call_cat, np.uint8)
    cat[np.isin(np.asarray(b.call_pos), masked)] = 2
    nb.call_cat = cat
    db = gpu_ctx.upload(cfg, b)
    try:
        _check_sites(oracle_lib, db, cfg, b, [_expected("full", 2)], "unmasked")
        db.set_mask(masked)
        out = db.run()
        ref = oracle_lib.methphase(cfg, nb, n_threads=4)
        assert np.array_equal(out.win_n_sites, ref.win_n_sites)
        assert db.masked_sites().tolist() == [2]
        want = [p for p in _expected("full", 2) if p not in masked]
        got = db.debug_sites(0, 0, cap=1 << 12)[0].tolist()
        assert got == want == oracle_lib.window_sites(cfg, nb, 0, 0)[0].tolist()
        assert np.array_equal(out.decision, ref.decision)
    finally:
        db.free()
