"""`hapmeth --dmr-rank` end to end on the device: pf_hapmeth_run_rank
(hapmeth_files, the CLI) over a haplotagged fixture BAM, against text built on
the CPU: the regions of the literal region reference, the host fetch with
those regions as the windows, the oracle's loader, the literal rank reference
(tests/_rank_ref.py) and pomfret_amd.rank_p, the library's host function, which
tests/test_ranktest.py pins to scipy.  Every comparison is on bytes; in every
run the .hapmeth.bed and the region file are the text a run without --dmr-rank
writes.

The --dmr fixture is test_hapmeth_perm_gpu.py's (coverage 12, min_delta_pct
30); the --regions one is test_hapmeth_regions_gpu.py's BED over its BAM.  The
reference gives, and the fixture asserts:

    min_sites  min_calls  regions  tested  untested  distinct rank_p  AUC > 0.5  AUC < 0.5  AUC = 0.5
            2          1       22      22         0               22         12         10          0
            2          3       22      10        12                8          3          5          2
            1          1      279     279         0              147        150        129          0
"""
import os
import subprocess

import pytest

from pomfret_amd.abi import DmrConfig

from tests import _fixtures as fx
from tests._perm_ref import perm_ref_batch
from tests._rank_ref import HEAD as KHEADER
from tests._rank_ref import bh_ref, rank_ref_batch, rank_text
from tests._regions_ref import eligible
from tests.test_dmr_gpu import _dmr_ref
from tests.test_hapmeth_dmr_gpu import HEADER, LCFG, _dmr_text
from tests.test_hapmeth_perm_gpu import N_PERM, _cfg, _perm_text
from tests.test_hapmeth_regions_gpu import CFG as RCFG
from tests.test_hapmeth_regions_gpu import HMM, _bed_regions, _records
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (min_sites, min_calls) -> regions, tested, untested, distinct rank_p, AUC above / below / exactly 0.5
TABLE = {(2, 1): (22, 22, 0, 22, 12, 10, 0), (2, 3): (22, 10, 12, 8, 3, 5, 2), (1, 1): (279, 279, 0, 147, 150, 129, 0)}


def _rank_recs(ref, regs):
    """(start, end) -> the record of window k of a rank_ref_batch result."""
    return {reg: dict({k: ref[k][w].tolist() for k in ("n_reads", "n_short", "cls")}, u2=int(ref["u2"][w]),
                      ties=int(ref["ties"][w]), status=int(ref["status"][w]), chrom="chrS", start=reg[0], end=reg[1])
            for w, reg in enumerate(regs)}


def _figures(text):
    body = [x.split("\t") for x in text.splitlines()[1:]]
    tested = [x for x in body if x[15] != "."]
    auc = [float(x[13]) for x in tested]
    return (len(body), len(tested), len(body) - len(tested), len({x[15] for x in tested}), len([a for a in auc if a > 0.5]),
            len([a for a in auc if a < 0.5]), len([a for a in auc if a == 0.5]))


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_rank")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, coverage=12, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
        wb, _ = oracle_lib.load_reads(LCFG, one)
        win_off, pos, cnt = _pile_ref(wb)
        # the second pass on the CPU: the regions (min_sites 1 holds them all) are the windows
        regs = [(r["start"], r["end"]) for r in _dmr_ref(pos, cnt, _cfg(1))["all"]]
        per, _, _ = bf.fetch_windows("chrS", [s for s, _ in regs], [e for _, e in regs], readback=0)
    pb, _ = oracle_lib.load_reads(LCFG, per)
    by_mc = {mc: _rank_recs(rank_ref_batch(pb, mc), regs) for mc in (1, 3)}
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, fisher_exact(c[0], c[1], c[2], c[3])[3]))
    dmr = {ms: _dmr_text(pos, cnt, _cfg(ms)) for ms in (1, 2)}

    def rank(ms, mc, max_p=1.0):
        keys = [(int(c[1]), int(c[2])) for c in (x.split("\t") for x in dmr[ms].splitlines()[1:]) if float(c[10]) <= max_p]
        return rank_text([by_mc[mc][k] for k in keys], False)
    texts = {key: rank(*key) for key in TABLE}
    for key, exp in TABLE.items():
        assert _figures(texts[key]) == exp, (key, _figures(texts[key]))
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", text="".join(lines), dmr=dmr, rank=texts, rank_of=rank, pb=pb,
                regs=regs, n_per=per.n_recs)


def _run(case, name, min_sites=2, min_calls=1, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=_cfg(min_sites), dmr_rank=True,
                        dmr_rank_min_calls=min_calls, **kw)
    assert open(res["path"]).read() == case["text"]
    assert res["rank_path"] == str(case["tmp"] / name) + ".hapmeth.rank.tsv"
    return res, open(res["dmr_path"]).read(), open(res["rank_path"]).read()


@pytest.mark.parametrize("min_sites,min_calls", sorted(TABLE))
def test_file_equals_cpu_text(case, min_sites, min_calls):
    res, dmr, rank = _run(case, f"a{min_sites}_{min_calls}", min_sites, min_calls)
    assert rank == case["rank"][(min_sites, min_calls)] and rank.startswith(KHEADER)
    assert dmr == case["dmr"][min_sites] and "n_tested" not in res
    n, tested, untested = TABLE[(min_sites, min_calls)][:3]
    assert (res["rank_tested"], res["rank_untested"], res["n_regions"]) == (tested, untested, n) and res["rank_ms_kernels"] > 0
    assert all(x.endswith("\t.") for x in rank.splitlines()[1:])              # found regions get no rank_q
    if min_sites == 1:
        assert res["rank_records"] == case["n_per"]      # every region was a window of the second pass


def test_other_files_are_the_bytes_without_rank(case):
    from pomfret_amd.pipeline import hapmeth_files
    plain = hapmeth_files(case["bam"], str(case["tmp"] / "plain"), region=case["region"], dmr=_cfg(2))
    assert "rank_path" not in plain and not os.path.exists(str(case["tmp"] / "plain") + ".hapmeth.rank.tsv")
    res, dmr, _ = _run(case, "with", 2, 3)
    assert open(plain["path"], "rb").read() == open(res["path"], "rb").read()
    assert open(plain["dmr_path"], "rb").read() == open(res["dmr_path"], "rb").read() == dmr.encode()


def test_with_dmr_perm(case):
    """Both tests on the one fetched batch: the region file as in the permutation test, the rank file the same bytes."""
    pr = perm_ref_batch(case["pb"], N_PERM, 1)
    tests = {reg: (int(pr["n_reads"][k][0]), int(pr["n_reads"][k][1]), int(pr["hits"][k]), int(pr["status"][k]))
             for k, reg in enumerate(case["regs"])}
    res, dmr, rank = _run(case, "perm", 2, 1, dmr_perm=N_PERM)
    assert dmr == _perm_text(case["dmr"][2], tests) and rank == case["rank"][(2, 1)]
    assert res["n_tested"] + res["n_untested"] == 22 and res["perm_records"] == res["rank_records"] > 0


def test_host_fetch_same_bytes(case):
    _, dmr, rank = _run(case, "h", 2, 3, host_fetch=True, threads=2)
    assert rank == case["rank"][(2, 3)] and dmr == case["dmr"][2]


@pytest.mark.parametrize("chunk,min_sites", [(7_000, 1), (33_333, 2), (100_000, 2)])
def test_chunk_size_same_bytes(case, chunk, min_sites):
    # job_windows 5 cuts the second pass into several jobs as well
    _, dmr, rank = _run(case, f"c{chunk}_{min_sites}", min_sites, 1, chunk_size=chunk, job_windows=5)
    assert rank == case["rank"][(min_sites, 1)] and dmr == case["dmr"][min_sites]


def test_max_p_is_the_matching_subset(case):
    res, dmr, rank = _run(case, "p", 1, 1, dmr_max_p=0.01)
    exp = case["rank_of"](1, 1, 0.01)
    full = case["rank"][(1, 1)].splitlines(keepends=True)
    assert 1 < len(exp.splitlines()) < len(full) and set(exp.splitlines(keepends=True)) <= set(full)
    assert rank == exp and res["n_regions"] == len(exp.splitlines()) - 1 == res["rank_tested"] + res["rank_untested"]
    assert res["rank_records"] < case["n_per"]


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3",
                        "--dmr-delta", "30", "--dmr-gap", "1000", "--dmr-min-sites", "2", "--dmr-rank",
                        "--dmr-rank-min-calls", "3", case["bam"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.bed").read() == case["text"]
    assert open(out + ".hapmeth.dmr.bed").read() == case["dmr"][2]
    assert open(out + ".hapmeth.rank.tsv").read() == case["rank"][(2, 3)]
    assert "rank test: 10 regions tested (at least 3 calls a read), 12 without a test" in r.stderr and "rank kernels" in r.stderr
    assert "22 regions written to %s.hapmeth.rank.tsv, 10 of them with a rank-sum p-value" % out in r.stderr
    # the default of --dmr-rank-min-calls is 3
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3", "--dmr-delta", "30",
                        "--dmr-gap", "1000", "--dmr-min-sites", "2", "--dmr-rank", case["bam"]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.rank.tsv").read() == case["rank"][(2, 3)]


# ---- --regions: rank_q
@pytest.fixture(scope="module")
def given(tmp_path_factory, oracle_lib):
    from pomfret_amd.bam import BamFile
    from tests._dmr_hmm_ref import hmm_ref
    tmp = tmp_path_factory.mktemp("hapmeth_rank_regions")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, len_scale=0.3)
    hi = int(aln.pos.max()) + 60_000
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [int(aln.pos.min())], [hi], readback=0)
        wb, _ = oracle_lib.load_reads(LCFG, one)
        win_off, pos, cnt = _pile_ref(wb)
        bed = _bed_regions(hmm_ref(pos, cnt, RCFG, HMM)["kept"], pos, cnt, int(aln.pos.min()), hi)
        rec = _records(bed, pos, cnt, hi)
        regs = sorted({(r["start"], r["end"]) for r in rec if eligible(r, RCFG, 1.0)})
        per, _, _ = bf.fetch_windows("chrS", [s for s, _ in regs], [e for _, e in regs], readback=0)
    pb, _ = oracle_lib.load_reads(LCFG, per)
    by = _rank_recs(rank_ref_batch(pb, 3), regs)
    path = str(tmp / "given.bed")
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%d\t%s\n" % r for r in bed))
    # the pass takes the eligible regions in the file's order, a repeated region each time
    order = [by[(r["start"], r["end"])] for r in rec if eligible(r, RCFG, 1.0)]
    text = rank_text(order, True)
    body = [x.split("\t") for x in text.splitlines()[1:]]
    tested = [x for x in body if x[15] != "."]
    assert len(tested) >= 5 and any(x[16] != x[15] for x in tested) and len(body) > len(regs)
    return dict(tmp=tmp, bam=bam, bed=path, region=f"chrS:1-{hi}", text=text, order=order)


def test_regions_rank_q(given):
    from pomfret_amd import rank_p
    from pomfret_amd.pipeline import hapmeth_files
    outs = {}
    for name, kw in (("r", {}), ("rp", dict(dmr_perm=N_PERM, job_windows=7)), ("rh", dict(host_fetch=True, chunk_size=33_333))):
        res = hapmeth_files(given["bam"], str(given["tmp"] / name), region=given["region"], dmr=RCFG, regions=given["bed"],
                            dmr_rank=True, **kw)
        outs[name] = res
        assert open(res["rank_path"]).read() == given["text"], name
        assert res["rank_tested"] + res["rank_untested"] == len(given["order"])
    assert open(outs["r"]["path"], "rb").read() == open(outs["rp"]["path"], "rb").read()
    # rank_q against the Python Benjamini-Hochberg loop, from the file's own integers
    tested = [r["status"] == 0 for r in given["order"]]
    p = [rank_p(r["u2"], r["n_reads"][0], r["n_reads"][1], r["ties"])[2] if t else 1.0 for r, t in zip(given["order"], tested)]
    q = bh_ref(p, tested)
    col = [x.split("\t")[16] for x in open(outs["r"]["rank_path"]).read().splitlines()[1:]]
    assert col == ["%.6g" % v if t else "." for v, t in zip(q, tested)]
    # the regions file without --dmr-rank is the same bytes
    plain = hapmeth_files(given["bam"], str(given["tmp"] / "plain"), region=given["region"], dmr=RCFG, regions=given["bed"])
    assert open(plain["regions_path"], "rb").read() == open(outs["r"]["regions_path"], "rb").read()
    assert not os.path.exists(str(given["tmp"] / "plain") + ".hapmeth.rank.tsv")


def test_regions_cli(given):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(given["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", given["region"], "--regions", given["bed"], "--dmr-min-cov", "5",
                        "--dmr-delta", "40", "--dmr-min-sites", "2", "--dmr-rank", given["bam"]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.rank.tsv").read() == given["text"] and ".hapmeth.rank.tsv" in r.stderr


def test_a_bad_bed_leaves_no_rank_file(given):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import hapmeth_files
    bad = str(given["tmp"] / "bad.bed")
    with open(bad, "w") as f:
        f.write("chrS\t10\t20\nchrS\t30\t20\n")
    out = str(given["tmp"] / "bad")
    for bed in (bad, str(given["tmp"] / "absent.bed")):
        with pytest.raises(PomfretError):
            hapmeth_files(given["bam"], out, region=given["region"], regions=bed, dmr_rank=True)
        for ext in ("bed", "regions.bed", "rank.tsv", "dmr.bed"):
            assert not os.path.exists(out + ".hapmeth." + ext)
