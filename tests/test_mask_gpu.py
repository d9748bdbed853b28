"""GPU tests of the site mask (pf_batch_set_mask, --mask-bed, --mask-variants).

A position that qualifies as a methylation site by its call counts and is
masked is no site, and nothing else changes (blockjoin.c:3202-3205, 3277-3283).
So the unchanged oracle checks every masked run: a masked run on a batch B must
equal the oracle's run on B with every call at a masked position turned into a
no-call (call_cat 2) -- such a position has no meth or unmeth call and never
qualifies, while the call still sits in its read, so the read's first and last
calls (3375-3384) and the window's position range are those of B.  Compared
with the field list and tolerances of tests/test_parity_gpu.py.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests._cases import _batch_from_reads, synth
from tests.test_parity_gpu import CASES, _compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c[0]: c for c in CASES}
FIELDS = ("decision", "dir_table", "dir_join", "dir_which_way", "win_n_sites", "win_n_reads", "read_hp",
          "dir_fisher_p", "dir_score")


def _calls_of(b, w):
    ro, co = b.win_read_off, b.read_call_off
    return int(co[ro[w]]), int(co[ro[w + 1]])


def _nocall(b, masks):
    """B': every call of window w at a position of masks[w] becomes a no-call."""
    nb = b.select(range(b.n_windows))
    cat = np.array(nb.call_cat, np.uint8)
    for w in range(b.n_windows):
        c0, c1 = _calls_of(b, w)
        hit = np.isin(np.asarray(b.call_pos[c0:c1]), np.asarray(masks[w], np.int64))
        cat[c0:c1][hit] = 2
    nb.call_cat = cat
    return nb


def _sites(oracle_lib, cfg, b):
    return [oracle_lib.window_sites(cfg, b, w, 0)[0].astype(np.int64) for w in range(b.n_windows)]


def _same(a, b, tag):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f"{tag}: {f}"


def _check(oracle_lib, gpu_ctx, cfg, b, pos, tag, win_rng=None, sites=None, want_paths=None):
    """Unmasked run, masked run, the oracle on the no-call batch; returns
    (unmasked result, masked result, removed counts, K12 paths)."""
    pos = np.unique(np.asarray(pos, np.int64))
    db = gpu_ctx.upload(cfg, b)
    try:
        out0 = db.run()
        paths0 = db.k12_paths()
        assert not db.masked_sites().any(), tag
        db.set_mask(pos, win_rng)
        out = db.run()
        removed = db.masked_sites().astype(np.int64)
        paths = db.k12_paths()
    finally:
        db.free()
    if win_rng is None:
        masks = [pos] * b.n_windows
    else:
        masks = [pos[int(a):int(e)] for a, e in np.asarray(win_rng).reshape(-1, 2)]
    ref = oracle_lib.methphase(cfg, _nocall(b, masks), n_threads=8)
    _compare(ref, out, tag)
    assert np.array_equal(paths, paths0), f"{tag}: K12 paths {paths.tolist()} != {paths0.tolist()}"
    if want_paths is not None:
        assert set(paths[paths > 0].tolist()) == set(want_paths), f"{tag}: paths {paths.tolist()}"
    assert np.array_equal(out0.win_n_sites.astype(np.int64) - out.win_n_sites, removed), tag
    if sites is not None:
        # a window without a sites pass (no calls, left coverage) has no sites to remove
        want = [np.isin(sites[w], masks[w]).sum() if paths0[w] else 0 for w in range(b.n_windows)]
        assert removed.tolist() == want, tag
    return out0, out, removed, paths


def _mask_from_sites(b, sites, every=3):
    """Every third site of each window, each chosen site +-1, the window's
    smallest and largest call position, and positions outside every read."""
    pos, chosen = [], []
    for w in range(b.n_windows):
        ch = sites[w][::every]
        chosen.append(ch)
        pos += ch.tolist() + (ch + 1).tolist() + (ch - 1).tolist()
        c0, c1 = _calls_of(b, w)
        if c1 > c0:
            cp = np.asarray(b.call_pos[c0:c1])
            pos += [int(cp.min()), int(cp.max())]
    # +-1 of a chosen site must not hit a site that was not chosen
    allsites = np.concatenate(sites) if sites else np.zeros(0, np.int64)
    chosen_all = np.concatenate(chosen) if chosen else np.zeros(0, np.int64)
    pos = np.unique(np.asarray(pos, np.int64))
    pos = pos[~np.isin(pos, np.setdiff1d(allsites, chosen_all)) | np.isin(pos, _extremes(b))]
    hi = int(np.asarray(b.read_end).max()) if b.n_reads else 1000
    pos = np.unique(np.concatenate([pos, [0, 3, hi + 1000, hi + 1001, (1 << 29) - 1]]))
    return pos, chosen


def _extremes(b):
    ex = []
    for w in range(b.n_windows):
        c0, c1 = _calls_of(b, w)
        if c1 > c0:
            cp = np.asarray(b.call_pos[c0:c1])
            ex += [int(cp.min()), int(cp.max())]
    return np.asarray(ex, np.int64)


def _k6_case():
    from pomfret_amd import Config
    return "k6", Config(k=6, k_span=5000, cov_for_selection=4, cov_for_runtime=8, n_cand=8), synth(4, 30, 33)


def _parity_cases():
    return [BY_NAME["synth30"], BY_NAME["gapmix"], BY_NAME["report200"], _k6_case()]


PARITY = _parity_cases()


@pytest.mark.parametrize("name,cfg,batch", PARITY, ids=[c[0] for c in PARITY])
def test_masked_windows_parity(oracle_lib, gpu_ctx, name, cfg, batch):
    """1. Window level: the masked run equals the oracle on the no-call batch;
    the removed count is the number of chosen sites, win_n_sites drops by it,
    and K12 takes the paths of the unmasked run."""
    sites = _sites(oracle_lib, cfg, batch)
    pos, chosen = _mask_from_sites(batch, sites)
    out0, out, removed, paths = _check(oracle_lib, gpu_ctx, cfg, batch, pos, name, sites=sites)
    assert removed.sum() > 0
    for w in range(batch.n_windows):
        if paths[w]:
            assert removed[w] >= len(chosen[w]), f"{name} w{w}"      # + an extreme that is a site


@pytest.mark.parametrize("name,cfg,batch", PARITY[:2], ids=[c[0] for c in PARITY[:2]])
def test_masked_dense_path(oracle_lib, gpu_ctx, monkeypatch, name, cfg, batch):
    """2a. The same check with every window on K12's dense path."""
    monkeypatch.setenv("PF_K12_DENSE", "1")
    sites = _sites(oracle_lib, cfg, batch)
    pos, _ = _mask_from_sites(batch, sites)
    _, _, removed, _ = _check(oracle_lib, gpu_ctx, cfg, batch, pos, name + "/dense", sites=sites, want_paths={3})
    assert removed.sum() > 0


def test_masked_two_segments(oracle_lib, gpu_ctx):
    """2b. The wide windows of test_wide_windows_parity: call positions span
    more than 2^19, two segments of the fast path (path 2)."""
    from pomfret_amd import Config
    from pomfret_amd.synth import SynthSpec, make_batch
    cfg = Config.from_coverage(20, given=False)
    b = make_batch(SynthSpec(n_windows=3, coverage=20, seed=41, gap=450_000))
    sites = _sites(oracle_lib, cfg, b)
    pos, _ = _mask_from_sites(b, sites)
    _, _, removed, paths = _check(oracle_lib, gpu_ctx, cfg, b, pos, "wide", sites=sites)
    assert 2 in paths.tolist() and removed.sum() > 0


# ---- hand-built window: qualifying sites at the places the kernel's index
# arithmetic changes.  110 reads carry a call at every site (40 left
# references, 40 untagged reads, 30 right references, as tests/_cases.t6_range_wrap);
# half the tagged reads of each haplotype call a site methylated, so every
# site has >= 20 calls of each kind (cov_for_selection 4).
P0 = 160_000
SEG = 524_288                      # positions per segment of the fast path
CHUNK = 16_384                     # positions per chunk of the dense path
EDGE = {"pmin": P0, "word_before": P0 + 6399, "word": P0 + 6400, "chunk_before": P0 + CHUNK - 1,
        "chunk": P0 + CHUNK, "seg_last": P0 + SEG - 1, "seg_first": P0 + SEG, "pmax": P0 + SEG + 4000}


def _edge_batch(far=False):
    rng = np.random.default_rng(71)
    s, e = 100_000, 150_000
    sites = set(P0 + 400 * i for i in range(25))                         # pmin, the word boundary P0 + 6400
    sites |= {P0 + 6399, P0 + CHUNK - 1, P0 + CHUNK}
    sites |= set(P0 + CHUNK + 400 * i for i in range(1, 6))
    sites |= set(P0 + SEG - 1 - 400 * i for i in range(0, 8)) | set(P0 + SEG + 400 * i for i in range(0, 11))
    if far:                                                              # a span past two segments: dense, unforced
        sites |= set(P0 + 1_100_000 + 400 * i for i in range(12))
    sites = np.array(sorted(sites), np.int64)
    assert far or (sites[0] == EDGE["pmin"] and sites[-1] == EDGE["pmax"])
    assert all(p in sites for p in EDGE.values())
    meth = rng.random(sites.shape[0]) < 0.5
    end = int(sites[-1]) + 2000
    reads = []
    for i in range(40):
        h = i % 2
        reads.append((60_000, end, h, [(int(p), int(meth[k] ^ h)) for k, p in enumerate(sites)]))
    for i in range(40):
        h = int(rng.integers(0, 2))
        reads.append((110_000 + 500 * i, end, 254, [(int(p), int(meth[k] ^ h)) for k, p in enumerate(sites)]))
    for i in range(30):
        h = i % 2
        reads.append((120_000 + 700 * i, end, h, [(int(p), int(meth[k] ^ h)) for k, p in enumerate(sites)]))
    return _batch_from_reads(s, e, reads), sites


@pytest.mark.parametrize("mode", ["fast", "dense", "dense_unforced"])
def test_masked_edges(oracle_lib, gpu_ctx, monkeypatch, mode):
    """3. Sites at pmin and pmax, on a 64-position word boundary of the bitmap
    and before it, at the last position of segment 1 and the first of segment
    2, on a 16,384-position chunk boundary and before it: each masked alone
    and all together."""
    from pomfret_amd import Config
    cfg = Config.from_coverage(30, given=False)
    if mode == "dense":
        monkeypatch.setenv("PF_K12_DENSE", "1")
    b, sites = _edge_batch(far=mode == "dense_unforced")
    osites = _sites(oracle_lib, cfg, b)
    assert np.array_equal(osites[0], sites)                     # every planted position qualifies
    want = {"fast": {2}, "dense": {3}, "dense_unforced": {3}}[mode]
    masks = [[p] for p in EDGE.values()] + [list(EDGE.values())]
    if mode == "dense_unforced":
        masks = [[int(sites[-1])], list(EDGE.values()) + [int(sites[-1])]]
    for m in masks:
        _, out, removed, _ = _check(oracle_lib, gpu_ctx, cfg, b, m, f"{mode}:{m}", sites=osites, want_paths=want)
        assert removed.tolist() == [len(m)] and out.win_n_sites[0] == len(sites) - len(m)


def test_neutral_masks(oracle_lib, gpu_ctx):
    """4. An empty mask, a mask hitting no site and a cleared mask give the
    unmasked run's bits; a second run under a mask repeats the first; masking
    every site of one window leaves it without sites (decision -1) and the
    other windows as they were."""
    name, cfg, b = BY_NAME["synth30"]
    sites = _sites(oracle_lib, cfg, b)
    allsites = np.concatenate(sites)
    db = gpu_ctx.upload(cfg, b)
    out0 = db.run()
    db.set_mask([])
    _same(out0, db.run(), "empty")
    assert not db.masked_sites().any()
    miss = np.setdiff1d(np.concatenate([allsites + 1, allsites - 1, [0, 5]]), allsites)
    db.set_mask(miss)
    _same(out0, db.run(), "no site hit")
    assert not db.masked_sites().any()
    db.set_mask(allsites[::2])
    m1 = db.run()
    assert db.masked_sites().sum() == len(allsites[::2])
    _same(m1, db.run(), "second run under the mask")
    assert db.masked_sites().sum() == len(allsites[::2])
    db.set_mask(np.zeros(0, np.uint32))
    _same(out0, db.run(), "cleared")
    assert not db.masked_sites().any()
    w = int(np.argmax(out0.win_n_sites))
    db.set_mask(sites[w])
    out = db.run()
    assert out.win_n_sites[w] == 0 and out.decision[w] == -1 and db.masked_sites()[w] == len(sites[w])
    ro = b.win_read_off
    for v in range(b.n_windows):
        if v == w:
            continue
        for f in FIELDS:
            a, g = getattr(out0, f), getattr(out, f)
            if f == "read_hp":
                a, g = a[ro[v]:ro[v + 1]], g[ro[v]:ro[v + 1]]
            else:
                a, g = a[v], g[v]
            assert np.array_equal(a, g), f"window {v}: {f}"
    db.free()
    ref = oracle_lib.methphase(cfg, _nocall(b, [sites[w]] * b.n_windows), n_threads=8)
    _compare(ref, out, "one window emptied")


def test_per_window_ranges(oracle_lib, gpu_ctx):
    """5. win_rng: each window sees its own slice of the array only, one
    window an empty range -- its sites stay although the array holds them."""
    name, cfg, b = BY_NAME["synth30"]
    sites = _sites(oracle_lib, cfg, b)
    order = np.argsort(np.asarray(b.win_start))                  # the array is ascending: windows by position
    pos, rng = [], np.zeros((b.n_windows, 2), np.uint32)
    for w in order.tolist():
        ch = sites[w][::2]
        rng[w] = (len(pos), len(pos) + len(ch))
        pos += ch.tolist()
    assert pos == sorted(set(pos))
    skip = int(order[1])
    rng[skip] = (rng[skip][0], rng[skip][0])                     # empty
    _, out, removed, _ = _check(oracle_lib, gpu_ctx, cfg, b, pos, "win_rng", win_rng=rng, sites=sites)
    assert removed[skip] == 0 and removed.sum() > 0
    # a slice of another window's positions removes nothing
    other = np.roll(rng, 1, axis=0)
    _, _, removed2, _ = _check(oracle_lib, gpu_ctx, cfg, b, pos, "win_rng rolled", win_rng=other, sites=sites)
    assert removed2.sum() == 0


def test_set_mask_argument_checks(oracle_lib, gpu_ctx):
    """6. A refused mask leaves the previous one in force."""
    from pomfret_amd import PomfretError
    name, cfg, b = BY_NAME["synth30"]
    sites = _sites(oracle_lib, cfg, b)
    keep = np.concatenate(sites)[::3]
    keep.sort()
    db = gpu_ctx.upload(cfg, b)
    db.set_mask(keep)
    first = db.run()
    want = db.masked_sites().copy()
    assert want.sum() == len(keep)
    W = b.n_windows
    bad = [dict(pos=[5, 5, 9]), dict(pos=[9, 5]), dict(pos=[1, 2, 1 << 29]),
           dict(pos=[1, 2, 3], win_rng=np.array([[0, 4]] * W)), dict(pos=[1, 2, 3], win_rng=np.array([[2, 1]] * W))]
    for kw in bad:
        with pytest.raises(PomfretError) as ei:
            db.set_mask(**kw)
        lim = kw["pos"][-1] == 1 << 29
        assert ("limit" in str(ei.value)) == lim, str(ei.value)
        again = db.run()
        _same(first, again, f"after refused {kw}")
        assert np.array_equal(db.masked_sites(), want)
    db.free()


def test_one_shot_mask(oracle_lib):
    """methphase_windows(mask=...)."""
    from pomfret_amd import methphase_windows
    name, cfg, b = BY_NAME["synth30"]
    sub = b.select([0, 1])
    sites = _sites(oracle_lib, cfg, sub)
    pos = np.unique(np.concatenate(sites)[::2])
    out = methphase_windows(cfg, sub, device=0, mask=pos)
    _compare(oracle_lib.methphase(cfg, _nocall(sub, [pos] * 2), n_threads=4), out, "one-shot")


def test_record_level_mask(oracle_lib, gpu_ctx):
    """7. A record-level batch (K0 loads the reads on the device): the checker
    is the oracle's loader, the no-call step, then the oracle."""
    from pomfret_amd import Config, LoadConfig
    from pomfret_amd.synth_aln import AlnSpec, make_aln_batch
    cfg, lcfg = Config.from_coverage(30, given=False), LoadConfig()
    aln = make_aln_batch(AlnSpec(n_windows=3, coverage=30, seed=17, len_scale=0.5), workers=1)
    wb, _ = oracle_lib.load_reads(lcfg, aln)
    sites = _sites(oracle_lib, cfg, wb)
    pos, chosen = _mask_from_sites(wb, sites)
    db = gpu_ctx.upload_aln(cfg, aln, lcfg)
    out0 = db.run()
    db.set_mask(pos)
    out = db.run()
    removed = db.masked_sites()
    _same(out, db.run(), "record level, second run")
    db.free()
    _compare(oracle_lib.methphase(cfg, wb, n_threads=4), out0, "record level, unmasked")
    _compare(oracle_lib.methphase(cfg, _nocall(wb, [pos] * wb.n_windows), n_threads=4), out, "record level")
    assert removed.tolist() == [int(np.isin(s, pos).sum()) for s in sites] and removed.sum() > 0
    assert np.array_equal(out0.win_n_sites - out.win_n_sites, removed)


# ---- 8. pipeline: files in, files out

@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """Two contigs, about 1 Mb, 30x, pre-haplotagged reads."""
    from pomfret_amd.synth_aln import AlnSpec
    from tests import _genome
    spec = _genome.GenomeSpec(contigs=(("chr1", 560_000), ("chr2", 440_000)), coverage=30, block_min=40_000,
                              block_max=90_000, short_block_frac=0.0, gap_min=5_000, gap_max=30_000, lead=60_000,
                              seed=23, qual=False, level=1, chunk_reads=400, hp_tags=True,
                              aln=AlnSpec(het_snv_rate=0.001, untag_frac=0.0, mean_len=22_000, sd_len=6_000,
                                          min_len=15_000, max_len=60_000))
    d = tmp_path_factory.mktemp("maskgen")
    return _genome.write_genome(str(d / "g"), spec, workers=4)


REPORT = dict(cov=30, chunk_size=10_000, chunk_stride=30_000)


def _report_cfg(cov, k=3, k_span=5000):
    from pomfret_amd import Config
    sel = cov // 10 + 1
    return Config(k=k, k_span=k_span, cov_for_selection=sel, cov_for_runtime=2 * sel, n_cand=cov // 4 + 1)


def _report_oracle_masked(oracle_lib, bam_path, vcf_path, masks, cov, chunk_size, chunk_stride, want_sites=False):
    """tests/_oracle_pipeline.report_oracle's loop (main_methreport,
    blockjoin.c:4901-5089; -c given) with the no-call step between the loader
    and the worker.  masks: {contig: positions}.  -> report.tsv text (and,
    want_sites, {contig: the unmasked windows' sites})."""
    from pomfret_amd import LoadConfig
    from pomfret_amd.bam import BamFile
    from tests.test_windows import _report_windows_ref
    rows, sites = [], {}
    cfg = _report_cfg(cov)
    with BamFile(bam_path) as bam:
        for c in oracle_lib.vcf_gaps(vcf_path):
            wins = _report_windows_ref(c["abs_start"], c["raw"], chunk_size, chunk_stride)
            if not wins:
                continue
            if bam.tid(c["name"]) < 0:
                dec = [-1] * len(wins)
            else:
                aln, _, _ = bam.fetch_windows(c["name"], [a for a, _ in wins], [b for _, b in wins])
                wb, _ = oracle_lib.load_reads(LoadConfig(), aln)
                if want_sites:
                    sites[c["name"]] = _sites(oracle_lib, cfg, wb)
                m = np.asarray(masks.get(c["name"], []), np.int64)
                dec = oracle_lib.methphase(cfg, _nocall(wb, [m] * wb.n_windows), n_threads=4).decision.tolist()
            for (a, b), d in zip(wins, dec):
                rows.append(f"{c['name']}\t{a}\t{b}\t" + ("correct" if d == 0 else "switch" if d == 1 else "fail") + "\n")
    return ("".join(rows), sites) if want_sites else "".join(rows)


def _write_bed(path, masks, gz=False):
    lines = ["# masked sites\n"]
    for name, pos in masks.items():
        lines += [f"{name}\t{p}\t{p + 1}\n" for p in reversed(list(pos))]       # unsorted on purpose
    lines.append("chrNone\t0\t100\n")
    with (gzip.open(path, "wt") if gz else open(path, "w")) as f:
        f.write("".join(lines))
    return path


@pytest.fixture(scope="module")
def report_masks(oracle_lib, genome):
    """Every second site of every chunk window, and the unmasked report."""
    text0, sites = _report_oracle_masked(oracle_lib, genome["bam"], genome["vcf"], {}, want_sites=True, **REPORT)
    masks = {name: np.unique(np.concatenate([s[::2] for s in per] + [np.zeros(0, np.int64)]))
             for name, per in sites.items()}
    assert sum(len(m) for m in masks.values()) > 50
    return text0, masks


def _cli(*args, timeout=300):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def test_report_files_mask_bed(oracle_lib, gpu_ctx, tmp_path, genome, report_masks):
    """report with --mask-bed: every report.tsv row and the totals equal the
    masked oracle's, through the device fetch, with --host-fetch, and from the
    command line; an empty BED changes nothing."""
    from pomfret_amd.pipeline import report_files
    text0, masks = report_masks
    bed = _write_bed(str(tmp_path / "m.bed.gz"), masks, gz=True)
    ref = _report_oracle_masked(oracle_lib, genome["bam"], genome["vcf"], masks, **REPORT)
    assert ref.count("\n") >= 8
    texts = {}
    for tag, kw in (("dev", {}), ("host", dict(host_fetch=True))):
        out = str(tmp_path / tag)
        res = report_files(genome["bam"], genome["vcf"], out, ctx=gpu_ctx, mask_bed=bed, **REPORT, **kw)
        texts[tag] = open(out + ".report.tsv").read()
        assert texts[tag] == ref, tag
        n = ref.count("\n")
        assert sum(res["counts"].values()) == n
        assert res["counts"] == {k: ref.count("\t" + k + "\n") for k in ("correct", "switch", "fail")}
        assert res["masked_sites"] > 0
    res0 = report_files(genome["bam"], genome["vcf"], str(tmp_path / "plain"), ctx=gpu_ctx, **REPORT)
    assert res0["masked_sites"] == 0
    assert open(str(tmp_path / "plain") + ".report.tsv").read() == text0
    # the command line: the same bytes; -v prints the mask line
    common = ["-c", "30", "--chunk-size", "10000", "--chunk-stride", "30000", "--vcf", genome["vcf"]]
    r = _cli("report", "-v", "-o", str(tmp_path / "cli"), "--mask-bed", bed, *common, genome["bam"])
    assert r.returncode == 0, r.stderr
    assert open(str(tmp_path / "cli") + ".report.tsv", "rb").read() == open(str(tmp_path / "dev") + ".report.tsv", "rb").read()
    assert "positions loaded" in r.stderr and "sites removed" in r.stderr
    empty = tmp_path / "empty.bed"
    empty.write_text("")
    r1 = _cli("report", "-o", str(tmp_path / "cli_e"), "--mask-bed", str(empty), *common, genome["bam"])
    r2 = _cli("report", "-o", str(tmp_path / "cli_n"), *common, genome["bam"])
    assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
    assert open(str(tmp_path / "cli_e") + ".report.tsv", "rb").read() == \
        open(str(tmp_path / "cli_n") + ".report.tsv", "rb").read() == text0.encode()
    assert r1.stdout == r2.stdout


def _methphase_oracle_masked(oracle_lib, bam_path, plan, cfg, masks):
    """Per-window decisions of `plan`'s windows: fetch_windows, load_reads,
    no-call, methphase, contig by contig."""
    from pomfret_amd import LoadConfig
    from pomfret_amd.bam import BamFile
    ws, we, co = plan.windows()
    dec = []
    with BamFile(bam_path) as bam:
        for ci, c in enumerate(plan.gaps()):
            a, b = int(co[ci]), int(co[ci + 1])
            if a == b:
                continue
            aln, _, _ = bam.fetch_windows(c["name"], ws[a:b], we[a:b])
            wb, _ = oracle_lib.load_reads(LoadConfig(), aln)
            m = np.asarray(masks.get(c["name"], []), np.int64)
            dec += oracle_lib.methphase(cfg, _nocall(wb, [m] * wb.n_windows), n_threads=4).decision.tolist()
    return np.asarray(dec, np.int8)


def test_methphase_files_mask(oracle_lib, tmp_path, genome):
    """methphase with a BED of every second site of its windows, on two
    contexts of one device; then --mask-variants (the synthetic genomes keep
    SNVs off CpGs except at block ends, so this route is checked for equality
    with the oracle, not for effect)."""
    from pomfret_amd import Config, Context, LoadConfig
    from pomfret_amd.bam import BamFile
    from pomfret_amd.pipeline import Plan, load_mask, make_opts, methphase_files
    cfg = Config.from_coverage(30, given=True)
    plan = Plan(make_opts(genome["bam"], genome["vcf"], None, cfg))
    ctxs = [Context(0), Context(0)]
    try:
        ws, we, co = plan.windows()
        names = [c["name"] for c in plan.gaps()]
        masks = {}
        with BamFile(genome["bam"]) as bam:
            for ci, name in enumerate(names):
                a, b = int(co[ci]), int(co[ci + 1])
                if a == b:
                    continue
                aln, _, _ = bam.fetch_windows(name, ws[a:b], we[a:b])
                wb, _ = oracle_lib.load_reads(LoadConfig(), aln)
                masks[name] = np.unique(np.concatenate([s[::2] for s in _sites(oracle_lib, cfg, wb)]))
        assert sum(len(m) for m in masks.values()) > 50
        bed = _write_bed(str(tmp_path / "mp.bed"), masks)
        ref = _methphase_oracle_masked(oracle_lib, genome["bam"], plan, cfg, masks)
        res = methphase_files(genome["bam"], genome["vcf"], None, cfg, ctxs=ctxs, job_windows=2, mask_bed=bed)
        assert np.array_equal(res["decision"], ref) and len(ref) >= 6
        assert res["masked_sites"] > 0
        vm = dict(zip(names, load_mask(names, vcf_path=genome["vcf"])))
        assert sum(len(m) for m in vm.values()) == genome["n_snvs"]
        refv = _methphase_oracle_masked(oracle_lib, genome["bam"], plan, cfg, vm)
        resv = methphase_files(genome["bam"], genome["vcf"], None, cfg, ctxs=ctxs, job_windows=2, mask_variants=True)
        assert np.array_equal(resv["decision"], refv)
        # both: the union
        both = {n: np.union1d(masks.get(n, np.zeros(0, np.int64)), vm[n]) for n in names}
        refb = _methphase_oracle_masked(oracle_lib, genome["bam"], plan, cfg, both)
        resb = methphase_files(genome["bam"], genome["vcf"], None, cfg, ctxs=ctxs[:1], host_fetch=True, mask_bed=bed,
                               mask_variants=True)
        assert np.array_equal(resb["decision"], refb)
        assert resb["masked_sites"] >= res["masked_sites"]
    finally:
        plan.close()
        for c in ctxs:
            c.close()
