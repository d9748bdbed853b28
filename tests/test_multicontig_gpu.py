"""Whole-genome-shaped runs on the device (VERDICT r02 "next round" 1 and 6a):
the multi-contig fixture of tests/_fixtures.multi_contig through the product
driver, against the oracle pipeline (tests/_oracle_pipeline.py):

  * methphase with and without -c, pre-haplotagged and -u: decisions, the
    merged first-wins qname table, the -u raw table, GTF/TSV/VCF bytes;
  * the cross-contig behaviour the reference has: per-contig parameters from
    the coverage estimate looked up by name (blockjoin.c:4358-4390, 4537-4539),
    the per-contig first-wins tables merged in contig order (4579-4595), the
    -u raw table shared by every contig (1880), prev_group_ID never reset so
    later contigs get abs_start 0 -> PS 0 and a skipped first GTF block
    (1406-1410, 2743);
  * `report` with the per-contig estimate read by VCF contig index
    (covs[i_ref], 5046) and with -c;
  * two contexts of one device (the multi-GPU work queue, pf_pipeline.c
    run_on_devices) byte-identical to one;
  * BASELINE configs[3]'s shape at small scale (tests/_genome): -u without -c
    on a genome whose windows share reads, with merged gaps whose dropped
    intervals go through the rescue, against the oracle pipeline and against
    the CPU port of the driver (the bench's e2e_u comparison).
"""
import numpy as np
import pytest

from tests import _fixtures as fx
from tests._oracle_pipeline import methphase_files_oracle, report_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc_tagged(tmp_path_factory):
    return fx.multi_contig(tmp_path_factory.mktemp("mct"), untagged=False)


@pytest.fixture(scope="module")
def mc_untagged(tmp_path_factory):
    return fx.multi_contig(tmp_path_factory.mktemp("mcu"), untagged=True)


def _outputs(prefix):
    return (open(prefix + ".mp.gtf").read(), open(prefix + ".mp.tsv").read(), open(prefix + ".mp.vcf", "rb").read())


def _check_quirks(ref, recs_by):
    """The fixture really exercises the cross-contig paths."""
    gtf = [ln.split("\t") for ln in ref["gtf"].splitlines()]
    # later contigs: abs_start 0, so their first block (start 0) is skipped
    for name in ("chrB", "chrC"):
        assert all(f[3] != "0" for f in gtf if f[0] == name)
    assert any(f[0] == "chrA" for f in gtf)
    vcf = ref["vcf"].split(b"\n")
    assert any(ln.startswith(b"chrC\t") and ln.endswith(b":0") for ln in vcf)       # PS 0
    # a qname joined on both chrA and chrC: the table keeps chrA's (contig order)
    dec = ref["decision"]
    assert (dec >= 0).sum() >= 3 and (dec < 0).sum() >= 2
    names_c = {r.qname for r in recs_by["chrC"]}
    names_a = {r.qname for r in recs_by["chrA"]}
    assert names_a & names_c & set(ref["qname_hp"])


@pytest.mark.parametrize("given", [True, False], ids=["c30", "estimate"])
@pytest.mark.parametrize("untagged", [False, True], ids=["tagged", "u"])
def test_multicontig_methphase(oracle_lib, gpu_ctx, tmp_path, mc_tagged, mc_untagged, untagged, given):
    from pomfret_amd import Config
    from pomfret_amd.pipeline import methphase_files
    bam, vcf, recs_by, _ = mc_untagged if untagged else mc_tagged
    cfg = Config.from_coverage(30, given=True) if given else None
    out = str(tmp_path / "o")
    res = methphase_files(bam, vcf, out, cfg, ctx=gpu_ctx, untagged=untagged, tsv=True, job_windows=2)
    ref = methphase_files_oracle(bam, vcf, cfg, untagged=untagged, recs_by_contig=recs_by)
    assert np.array_equal(res["decision"], ref["decision"])
    assert res["qname_hp"] == ref["qname_hp"]
    assert list(res["qname_hp"]) == list(ref["qname_hp"])          # insertion (merge) order too
    assert res["raw_hp"] == ref["raw_hp"]
    gtf, tsv, vcf_b = _outputs(out)
    assert gtf == ref["gtf"] and tsv == ref["tsv"] and vcf_b == ref["vcf"]
    _check_quirks(ref, recs_by)
    if untagged:
        assert len(ref["raw_hp"]) > 0


def test_multicontig_plan_parameters(oracle_lib, gpu_ctx, mc_tagged):
    """No -c: each contig's job parameters come from the device coverage
    estimate of that contig, looked up by name (the header order differs from
    the VCF's), est/10+1, 2x, est/4+1 with the clamps (4358-4390)."""
    from pomfret_amd import Config
    from pomfret_amd.bam import BamFile
    from pomfret_amd.pipeline import JOB_WINDOWS, Plan, make_opts
    bam, vcf, _, _ = mc_tagged
    with BamFile(bam) as b:
        covs = b.estimate_coverage()
        tids = {n: b.tid(n) for n in fx.MULTI_VCF_ORDER}
    assert len(set(covs)) >= 3
    plan = Plan(make_opts(bam, vcf, None, None, ctxs=[gpu_ctx], job_windows=2))
    try:
        seen = set()
        for j in range(plan.n_jobs(JOB_WINDOWS)):
            info = plan.job_info(JOB_WINDOWS, j)
            want = Config.from_coverage(int(covs[tids[info["contig_name"]]]), given=False)
            got = info["cfg"]
            assert (got.cov_for_selection, got.cov_for_runtime, got.n_cand) == \
                (want.cov_for_selection, want.cov_for_runtime, want.n_cand), info["contig_name"]
            seen.add(info["contig_name"])
        assert seen == set(fx.MULTI_VCF_ORDER)
        assert plan.n_jobs(JOB_WINDOWS) >= 4
    finally:
        plan.close()


@pytest.mark.parametrize("cov", [0, 30], ids=["estimate", "c30"])
def test_multicontig_report(oracle_lib, gpu_ctx, tmp_path, mc_tagged, cov):
    """`report` over every contig: the estimate is read by VCF contig index
    (covs[i_ref], 5046, so chrA gets chrD's), chunk windows from abs_start 0
    on the later contigs; rows and totals equal the oracle's."""
    from pomfret_amd.pipeline import report_files
    bam, vcf, _, _ = mc_tagged
    out = str(tmp_path / "rep")
    res = report_files(bam, vcf, out, cov=cov, chunk_size=10_000, chunk_stride=25_000, ctx=gpu_ctx)
    text = open(out + ".report.tsv").read()
    assert text == report_oracle(bam, vcf, cov, 10_000, 25_000)
    assert sum(res["counts"].values()) == text.count("\n")
    assert {ln.split("\t")[0] for ln in text.splitlines()} == set(fx.MULTI_VCF_ORDER)


@pytest.mark.parametrize("untagged", [False, True], ids=["tagged", "u"])
def test_two_contexts_one_device(gpu_ctx, tmp_path, mc_tagged, mc_untagged, untagged):
    """Two contexts on device 0 drive the in-process multi-GPU path: one host
    thread per context claiming jobs from one queue (and -u jobs), per-context
    staging buffers.  Outputs are byte-identical to the one-context run."""
    from pomfret_amd import Config, Context
    from pomfret_amd.pipeline import methphase_files
    bam, vcf, _, _ = mc_untagged if untagged else mc_tagged
    cfg = Config.from_coverage(30, given=True)
    one = methphase_files(bam, vcf, str(tmp_path / "one"), cfg, ctx=gpu_ctx, untagged=untagged, tsv=True,
                          job_windows=1)
    ctxs = [Context(0), Context(0)]
    try:
        two = methphase_files(bam, vcf, str(tmp_path / "two"), cfg, ctxs=ctxs, untagged=untagged, tsv=True,
                              job_windows=1)
    finally:
        for c in ctxs:
            c.close()
    assert np.array_equal(one["decision"], two["decision"])
    assert list(one["qname_hp"].items()) == list(two["qname_hp"].items())
    assert one["raw_hp"] == two["raw_hp"]
    assert _outputs(str(tmp_path / "one")) == _outputs(str(tmp_path / "two"))


def test_untagged_prepass_in_pieces(oracle_lib, gpu_ctx, tmp_path, mc_untagged, monkeypatch):
    """The -u pre-pass fetches each contig in position pieces of bounded
    compressed size (a 60x chromosome is tens of GB); forced to
    64 KiB pieces here, the reads are taken once each, in BAM order, with the
    K4 cursor chain carried across pieces: the raw table and every output
    equal the oracle pipeline's."""
    from pomfret_amd import Config
    from pomfret_amd.pipeline import methphase_files
    bam, vcf, recs_by, _ = mc_untagged
    monkeypatch.setenv("PF_FETCH_PIECE_BYTES", str(64 << 10))
    cfg = Config.from_coverage(30, given=True)
    out = str(tmp_path / "p")
    res = methphase_files(bam, vcf, out, cfg, ctx=gpu_ctx, untagged=True, tsv=True, job_windows=2)
    ref = methphase_files_oracle(bam, vcf, cfg, untagged=True, recs_by_contig=recs_by)
    assert res["raw_hp"] == ref["raw_hp"] and len(ref["raw_hp"]) > 0
    assert np.array_equal(res["decision"], ref["decision"])
    assert _outputs(out) == (ref["gtf"], ref["tsv"], ref["vcf"])
    # one contig directly: the same reads, tags and order as a one-piece fetch
    from pomfret_amd.bam import BamFile, vcf_known_vars
    kv = vcf_known_vars(vcf, "chrC")
    with BamFile(bam) as b:
        hp_p, qn_p, info_p = b.haptag_device(gpu_ctx, "chrC", kv)
        monkeypatch.delenv("PF_FETCH_PIECE_BYTES")
        hp_1, qn_1, info_1 = b.haptag_device(gpu_ctx, "chrC", kv)
    assert qn_p == qn_1 and np.array_equal(hp_p, hp_1)
    assert info_p["attempts"] > info_1["attempts"]                 # several pieces ran
    prim = [r for r in recs_by["chrC"] if not (r.flag & (4 | 256 | 2048))]
    assert qn_1 == [r.qname for r in prim]


@pytest.fixture(scope="module")
def genome_small(tmp_path_factory):
    from tests import _genome
    d = tmp_path_factory.mktemp("gen")
    return _genome.write_genome(str(d / "g"), _genome.small_spec(), workers=4, keep_recs=True)


@pytest.mark.parametrize("job_windows", [0, 3], ids=["default_jobs", "jobs3"])
def test_genome_untagged_estimate(oracle_lib, gpu_ctx, tmp_path, genome_small, job_windows):
    """`methphase -u` without -c on a 4-contig genome (reads uniform over
    each contig, adjacent windows sharing reads, short blocks merged away):
    decisions, the -u raw table, the merged first-wins table and the
    GTF/TSV/VCF bytes (dropped-interval rescue included) equal the oracle
    pipeline's; the CPU port of the driver writes the same bytes."""
    from pomfret_amd.pipeline import methphase_files
    from tests._oracle_pipeline import methphase_files_port
    g = genome_small
    out = str(tmp_path / "o")
    res = methphase_files(g["bam"], g["vcf"], out, None, ctx=gpu_ctx, untagged=True, tsv=True,
                          job_windows=job_windows)
    ref = methphase_files_oracle(g["bam"], g["vcf"], None, untagged=True, recs_by_contig=g["recs_by_contig"])
    assert np.array_equal(res["decision"], ref["decision"])
    assert res["raw_hp"] == ref["raw_hp"] and len(ref["raw_hp"]) > 1000
    assert list(res["qname_hp"].items()) == list(ref["qname_hp"].items())
    assert _outputs(out) == (ref["gtf"], ref["tsv"], ref["vcf"])
    dec = ref["decision"]
    assert (dec >= 0).sum() >= 5 and len(dec) >= 15
    assert ref["counts"][1] > 0                                  # rescued dropped-interval variants
    port, _ = methphase_files_port(g["bam"], g["vcf"], str(tmp_path / "p"), None, untagged=True, threads=4,
                                   tsv=True)
    assert _outputs(str(tmp_path / "p")) == _outputs(out)


def _dist_worker(rank, world, port, tmp, untagged):
    """One rank of methphase_files_dist on device 0 (gloo for the gathers):
    no runner, the rank's jobs run on the device."""
    import json
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pomfret_amd import Context
        from pomfret_amd.pipeline import methphase_files_dist
        ctx = Context(0)
        try:
            res = methphase_files_dist(os.path.join(tmp, "m.bam"), os.path.join(tmp, "m.vcf"),
                                       os.path.join(tmp, "dist"), None, untagged=untagged, tsv=True, job_windows=2,
                                       ctx=ctx)
        finally:
            ctx.close()
        with open(os.path.join(tmp, f"res{rank}.json"), "w") as f:
            json.dump(dict(decision=res["decision"].tolist(), qname_hp=list(res["qname_hp"].items()),
                           raw_hp=res["raw_hp"]), f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("untagged", [False, True], ids=["tagged", "u"])
def test_two_ranks_on_one_device(gpu_ctx, tmp_path, untagged):
    """VERDICT r02 "next round" 6b: methphase_files_dist with two gloo ranks,
    both on device 0 and no runner (each rank's LPT shard of window jobs and
    -u jobs on the device, the -u tables all-gathered, the window results
    gathered to the writer): decisions, both first-wins tables and the
    GTF/TSV/VCF bytes equal the single-process run, without -c."""
    import json
    import socket
    import torch.multiprocessing as mp
    from pomfret_amd.pipeline import methphase_files
    fx.multi_contig(tmp_path, untagged=untagged)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dist_worker, args=(2, port, str(tmp_path), untagged), nprocs=2, join=True)
    one = methphase_files(str(tmp_path / "m.bam"), str(tmp_path / "m.vcf"), str(tmp_path / "one"), None, ctx=gpu_ctx,
                          untagged=untagged, tsv=True, job_windows=2)
    for r in range(2):
        got = json.load(open(tmp_path / f"res{r}.json"))
        assert got["decision"] == one["decision"].tolist()
        assert [tuple(x) for x in got["qname_hp"]] == list(one["qname_hp"].items())
        assert got["raw_hp"] == one["raw_hp"]
    assert _outputs(str(tmp_path / "dist")) == _outputs(str(tmp_path / "one"))
    assert (one["decision"] >= 0).sum() >= 3


@pytest.mark.parametrize("steal", [True, False], ids=["steal", "nosteal"])
def test_untagged_window_jobs_follow_the_arenas(gpu_ctx, tmp_path, genome_small, monkeypatch, steal):
    """The -u pre-pass keeps each contig's inflated arena on the device that
    fetched it; window jobs are queued per device by that arena and a device
    steals from another's queue only when its own and the shared one are
    empty (VERDICT r03 "next round" 6; blockjoin.c:1841-1898, 4350-4426).
    Rehearsed on one GPU with PF_FETCH_CACHE_SCOPE=ctx (an arena serves only
    the context that kept it, and every context is a device of its own): the
    outputs equal the one-context run byte for byte; every window fetch is an
    arena hit or a miss, the misses are the stolen jobs (their compressed
    bytes re-read), and with stealing off every fetch hits."""
    from pomfret_amd import Context
    from pomfret_amd.pipeline import methphase_files
    g = genome_small
    one = methphase_files(g["bam"], g["vcf"], str(tmp_path / "one"), None, ctx=gpu_ctx, untagged=True, tsv=True,
                          job_windows=3)
    monkeypatch.setenv("PF_FETCH_CACHE_SCOPE", "ctx")
    if not steal:
        monkeypatch.setenv("PF_JOB_STEAL", "0")
    ctxs = [Context(0), Context(0)]
    try:
        two = methphase_files(g["bam"], g["vcf"], str(tmp_path / "two"), None, ctxs=ctxs, untagged=True, tsv=True,
                              job_windows=3)
    finally:
        for c in ctxs:
            c.close()
    assert np.array_equal(one["decision"], two["decision"])
    assert list(one["qname_hp"].items()) == list(two["qname_hp"].items())
    assert one["raw_hp"] == two["raw_hp"]
    assert _outputs(str(tmp_path / "one")) == _outputs(str(tmp_path / "two"))
    st = two["stats"]
    n_fetch = st["windows"]["n_fetch"]
    assert n_fetch > 4 and st["arena_hits"] + st["arena_misses"] == n_fetch
    assert st["arena_misses"] == st["steals"]
    assert (st["reread_bytes"] > 0) == (st["arena_misses"] > 0)
    if not steal:
        assert st["steals"] == 0 and st["arena_hits"] == n_fetch


@pytest.mark.parametrize("shape", ["separate", "dense"])
def test_untagged_piece_arenas(oracle_lib, gpu_ctx, tmp_path, monkeypatch, shape):
    """A chromosome-scale contig (VERDICT r04 "next round" 2), at test scale:
    the -u pre-pass fetches it in position pieces (forced small) and keeps
    every piece's inflated arena; the plan places the piece bounds between the
    windows' fetch regions and cuts the window jobs there, so every window
    fetch is served by a kept piece (no file read, no inflate).  "separate":
    one 3 Mb contig whose windows' fetch regions leave room for the bounds;
    "dense": the 4-contig genome whose regions overlap end to end, so a bound
    falls inside them and the piece before it fetches past the bound over the
    windows starting in it.  Outputs equal the one-piece run, the run without
    arenas and the oracle pipeline (blockjoin.c:1841-1898, 4350-4426).
    "separate" then runs twice under an arena budget of half the contig's
    inflated bytes: 2 of the 4 window fetches hit and 2 miss, in both runs."""
    import os
    from tests import _genome
    from pomfret_amd.pipeline import methphase_files
    spec = _genome.pieces_spec() if shape == "separate" else _genome.small_spec()
    g = _genome.write_genome(str(tmp_path / "p"), spec, workers=4, keep_recs=True)
    size = os.path.getsize(g["bam"])
    piece = size // 4 if shape == "separate" else size // 10
    runs = {}
    for name, env in (("one", {}), ("pieces", {"PF_FETCH_PIECE_BYTES": str(piece)}),
                      ("nocache", {"PF_FETCH_PIECE_BYTES": str(piece), "PF_FETCH_CACHE": "0"})):
        for k in ("PF_FETCH_PIECE_BYTES", "PF_FETCH_CACHE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = str(tmp_path / name)
        runs[name] = (methphase_files(g["bam"], g["vcf"], out, None, ctx=gpu_ctx, untagged=True, tsv=True,
                                      job_windows=4), _outputs(out))
    ref = methphase_files_oracle(g["bam"], g["vcf"], None, untagged=True, recs_by_contig=g["recs_by_contig"])
    for name, (res, outs) in runs.items():
        assert np.array_equal(res["decision"], ref["decision"]), name
        assert res["raw_hp"] == ref["raw_hp"], name
        assert outs == (ref["gtf"], ref["tsv"], ref["vcf"]), name
    st = runs["pieces"][0]["stats"]
    n_fetch = st["windows"]["n_fetch"]
    assert st["haptag"]["n_fetch"] == len(spec.contigs) and n_fetch >= 3
    assert st["arena_hits"] == n_fetch and st["arena_misses"] == 0 and st["reread_bytes"] == 0
    assert runs["nocache"][0]["stats"]["arena_hits"] == 0
    assert (ref["decision"] >= 0).sum() >= 2
    if shape != "separate":
        return
    # A budget of half the contig's inflated bytes (PF_ARENA_KEEP_MAX, as
    # tools/genome_scale.py sets it): some pieces are kept and some are not
    # (observed: 2 hits, 2 misses, 18,371,950 bytes re-read), and a second run
    # in the same process does exactly as the first, because the first gave
    # its whole budget back when it cleared its cache.
    monkeypatch.delenv("PF_FETCH_CACHE")
    monkeypatch.setenv("PF_FETCH_PIECE_BYTES", str(piece))
    monkeypatch.setenv("PF_ARENA_KEEP_MAX", str(st["haptag"]["inflated_bytes"] // 2))
    capped = []
    for name in ("cap1", "cap2"):
        out = str(tmp_path / name)
        res = methphase_files(g["bam"], g["vcf"], out, None, ctx=gpu_ctx, untagged=True, tsv=True, job_windows=4)
        assert _outputs(out) == runs["nocache"][1], name
        capped.append({k: res["stats"][k] for k in ("arena_hits", "arena_misses", "reread_bytes")})
    print(f"\n[arena budget] inflated {st['haptag']['inflated_bytes']} bytes, half kept: {capped}")
    assert capped[0]["arena_hits"] > 0 and capped[0]["arena_misses"] > 0
    assert capped[1] == capped[0]
