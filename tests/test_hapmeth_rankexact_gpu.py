"""`hapmeth --dmr-rank --dmr-rank-exact` end to end on the device:
pf_hapmeth_run_rank_exact (hapmeth_files, the CLI) over test_hapmeth_rank_gpu.py's
two fixtures (--dmr at coverage 12, --regions over its BED), against text built
on the CPU: the regions of the literal references, the host fetch with those
regions as the windows, the oracle's loader, the rank reference and the exact
reference (tests/_rankexact_ref.py).  Every comparison is on bytes: the rank
file, its first 17 columns against a run without the option, and every other
file against such a run.

The references give, and the fixtures assert (min_calls 1 for --dmr, 3 for
--regions; "apart": exact regions whose exact_p and rank_p differ by more than
a factor of 2):

    fixture    max_reads  regions  exact  over max_reads  no best_p  apart
    --dmr             64      279    279               0          0     74
    --dmr              8      279     35             244          0     10
    --regions         64       44     36               1          7     23
    --regions          8       44      8              29          7      0
"""
import os
import subprocess

import pytest

from tests import _fixtures as fx
from tests._rank_ref import rank_ref_batch
from tests._rankexact_ref import HEAD_EXTRA, rank_exact_text, rankexact_ref_batch
from tests._regions_ref import eligible
from tests.test_dmr_gpu import _dmr_ref
from tests.test_hapmeth_dmr_gpu import LCFG, _dmr_text
from tests.test_hapmeth_perm_gpu import N_PERM, _cfg
from tests.test_hapmeth_rank_gpu import KHEADER, _rank_recs
from tests.test_hapmeth_regions_gpu import CFG as RCFG
from tests.test_hapmeth_regions_gpu import HMM, _bed_regions, _records
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (fixture, max_reads) -> lines, exact, over max_reads, lines without a best_p, exact and a factor of 2 from rank_p
TABLE = {("dmr", 64): (279, 279, 0, 0, 74), ("dmr", 8): (279, 35, 244, 0, 10),
         ("regions", 64): (44, 36, 1, 7, 23), ("regions", 8): (44, 8, 29, 7, 0)}
assert TABLE[("dmr", 64)][4] >= 1 and TABLE[("regions", 64)][4] >= 1 and TABLE[("dmr", 8)][2] >= 1


def _exact_recs(pb, regs, min_calls, max_reads):
    """(start, end) -> the rank record of the region's window with the exact test's two, total and exact_status."""
    recs = _rank_recs(rank_ref_batch(pb, min_calls), regs)
    x = rankexact_ref_batch(pb, min_calls, max_reads)
    for w, reg in enumerate(regs):
        assert int(x["u2"][w]) == recs[reg]["u2"] and x["n_reads"][w].tolist() == recs[reg]["n_reads"]
        recs[reg].update(two=int(x["two"][w]), total=int(x["total"][w]), exact_status=int(x["status"][w]))
    return recs


def _figures(text, recs):
    body = [x.split("\t") for x in text.splitlines()[1:]]
    exact = [x for x in body if x[17] != "."]
    apart = [x for x in exact if not 0.5 <= float(x[17]) / float(x[15]) <= 2.0]
    assert len(body) == len(recs) and all((x[17] != ".") == (r["exact_status"] == 0) for x, r in zip(body, recs))
    return len(body), len(exact), len([r for r in recs if r["exact_status"] == 2]), len([x for x in body if x[18] == "."]), len(apart)


def build_case(tmp, oracle_lib):
    """test_hapmeth_rank_gpu's --dmr fixture, min_sites 1 and min_calls 1: every found region is a line."""
    from pomfret_amd.bam import BamFile
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, coverage=12, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
        wb, _ = oracle_lib.load_reads(LCFG, one)
        win_off, pos, cnt = _pile_ref(wb)
        regs = [(r["start"], r["end"]) for r in _dmr_ref(pos, cnt, _cfg(1))["all"]]
        per, _, _ = bf.fetch_windows("chrS", [s for s, _ in regs], [e for _, e in regs], readback=0)
    pb, _ = oracle_lib.load_reads(LCFG, per)
    keys = [(int(c[1]), int(c[2])) for c in (x.split("\t") for x in _dmr_text(pos, cnt, _cfg(1)).splitlines()[1:])]
    texts = {}
    for mx in (64, 8):
        by = _exact_recs(pb, regs, 1, mx)
        texts[mx] = rank_exact_text([by[k] for k in keys], False)
        assert _figures(texts[mx], [by[k] for k in keys]) == TABLE[("dmr", mx)], (mx, _figures(texts[mx], [by[k] for k in keys]))
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", text=texts)


def build_given(tmp, oracle_lib):
    """test_hapmeth_rank_gpu's --regions fixture, min_calls 3: best_q is Benjamini-Hochberg over best_p."""
    from pomfret_amd.bam import BamFile
    from tests._dmr_hmm_ref import hmm_ref
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
    path = str(tmp / "given.bed")
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%d\t%s\n" % r for r in bed))
    texts = {}
    for mx in (64, 8):
        by = _exact_recs(pb, regs, 3, mx)
        order = [by[(r["start"], r["end"])] for r in rec if eligible(r, RCFG, 1.0)]
        texts[mx] = rank_exact_text(order, True)
        assert _figures(texts[mx], order) == TABLE[("regions", mx)], (mx, _figures(texts[mx], order))
    return dict(tmp=tmp, bam=bam, bed=path, region=f"chrS:1-{hi}", text=texts)


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    return build_case(tmp_path_factory.mktemp("hapmeth_rankexact"), oracle_lib)


@pytest.fixture(scope="module")
def given(tmp_path_factory, oracle_lib):
    return build_given(tmp_path_factory.mktemp("hapmeth_rankexact_regions"), oracle_lib)


def _files(res):
    return {k: open(res[k], "rb").read() for k in sorted(res) if k.endswith("path") and k != "rank_path" and res[k]}


def _first17(text):
    return "".join("\t".join(x.split("\t")[:17]) + "\n" for x in text.splitlines())


@pytest.mark.parametrize("mx", [64, 8])
def test_dmr_file_equals_cpu_text(case, mx):
    from pomfret_amd.pipeline import hapmeth_files
    kw = dict(region=case["region"], dmr=_cfg(1), dmr_rank=True, dmr_rank_min_calls=1, dmr_perm=N_PERM, assign=None,
              tag_check=True)
    plain = hapmeth_files(case["bam"], str(case["tmp"] / f"plain{mx}"), **kw)
    res = hapmeth_files(case["bam"], str(case["tmp"] / f"x{mx}"), rank_exact=True, rank_exact_max=mx, **kw)
    rank = open(res["rank_path"]).read()
    assert rank == case["text"][mx] and rank.startswith(KHEADER.rstrip("\n") + HEAD_EXTRA + "\n")
    assert _first17(rank) == open(plain["rank_path"]).read()
    n, exact, over = TABLE[("dmr", mx)][:3]
    assert (res["rank_exact"], res["rank_exact_over"], res["rank_tested"] + res["rank_untested"]) == (exact, over, n)
    assert res["rank_exact_ms_kernels"] > 0 and "rank_exact" not in plain
    # .hapmeth.bed, the region file, the permutation columns in it and the tag-check files: the bytes without the option
    a, b = _files(plain), _files(res)
    assert sorted(a) == sorted(b) and len(a) >= 3 and all(a[k] == b[k] for k in a), [k for k in a if a[k] != b[k]]
    if mx == 8:
        assert over >= 1


def test_dmr_with_assign_same_other_files(case):
    from pomfret_amd.abi import AssignConfig
    from pomfret_amd.pipeline import hapmeth_files
    kw = dict(region=case["region"], dmr=_cfg(1), dmr_rank=True, dmr_rank_min_calls=1, assign=AssignConfig(), job_windows=5,
              chunk_size=33_333)
    plain = hapmeth_files(case["bam"], str(case["tmp"] / "aplain"), **kw)
    res = hapmeth_files(case["bam"], str(case["tmp"] / "ax"), rank_exact=True, **kw)
    assert open(res["rank_path"]).read() == case["text"][64]            # several jobs in the second pass: the same bytes
    a, b = _files(plain), _files(res)
    assert "assign_path" in a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)


@pytest.mark.parametrize("mx", [64, 8])
def test_regions_best_q(given, mx):
    from pomfret_amd.pipeline import hapmeth_files
    kw = dict(region=given["region"], dmr=RCFG, regions=given["bed"], dmr_rank=True)
    plain = hapmeth_files(given["bam"], str(given["tmp"] / f"plain{mx}"), **kw)
    res = hapmeth_files(given["bam"], str(given["tmp"] / f"x{mx}"), rank_exact=True, rank_exact_max=mx, **kw)
    rank = open(res["rank_path"]).read()
    assert rank == given["text"][mx] and _first17(rank) == open(plain["rank_path"]).read()
    n, exact, over = TABLE[("regions", mx)][:3]
    assert (res["rank_exact"], res["rank_exact_over"]) == (exact, over)
    a, b = _files(plain), _files(res)
    assert "regions_path" in a and sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    cols = [x.split("\t") for x in rank.splitlines()[1:]]
    assert all((c[19] == ".") == (c[18] == ".") for c in cols) and any(c[19] not in (".", c[16]) for c in cols)


def test_cli(case, given):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    base = [exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3", "--dmr-delta", "30",
            "--dmr-gap", "1000", "--dmr-min-sites", "1", "--dmr-rank", "--dmr-rank-min-calls", "1"]
    r = subprocess.run(base + ["--dmr-rank-exact", "--dmr-rank-exact-max", "8", case["bam"]], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.rank.tsv").read() == case["text"][8]
    n, exact, over = TABLE[("dmr", 8)][:3]
    assert "%d of them with an exact p-value, %d with more than 8 counted reads" % (exact, over) in r.stderr
    assert "exact rank test: %d regions with an exact p-value (at most 8 reads), %d over the limit" % (exact, over) in r.stderr
    r = subprocess.run(base + ["--dmr-rank-exact", case["bam"]], capture_output=True, text=True, timeout=120)     # default 64
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.rank.tsv").read() == case["text"][64]
    out = str(given["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", given["region"], "--regions", given["bed"], "--dmr-min-cov", "5",
                        "--dmr-delta", "40", "--dmr-min-sites", "2", "--dmr-rank", "--dmr-rank-exact", given["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.rank.tsv").read() == given["text"][64]


@pytest.mark.parametrize("args,word", [
    (["--dmr", "--dmr-rank-exact"], "--dmr-rank-exact needs --dmr-rank"),
    (["--dmr", "--dmr-rank", "--dmr-rank-exact", "--dmr-rank-exact-max", "1"], "bad --dmr-rank-exact-max"),
    (["--dmr", "--dmr-rank", "--dmr-rank-exact", "--dmr-rank-exact-max", "65"], "bad --dmr-rank-exact-max")])
def test_cli_errors(case, args, word):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "err")
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"]] + args + [case["bam"]], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and word in r.stderr and not os.path.exists(out + ".hapmeth.rank.tsv")
