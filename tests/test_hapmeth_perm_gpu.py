"""`hapmeth --dmr --dmr-perm` end to end on the device: pf_hapmeth_run_perm
(hapmeth_files, the CLI) over a haplotagged fixture BAM, against text built
on the CPU: the regions of the literal region reference, the host fetch with
those regions as the windows, the oracle's loader, and the literal permutation
reference (tests/_perm_ref.py).  Every comparison is on bytes; in every run the
.hapmeth.bed is the text a run without --dmr writes, and without dmr_perm the
region file is the one without the three columns.

The fixture is test_hapmeth_dmr_gpu.py's at coverage 12 instead of 30 and
min_delta_pct 30 instead of 50.  At 30x and delta 50 the reference gives every
region of min_sites 2 the smallest possible perm_p (0 hits of 99: 0.01), so
one value only; at 12x and delta 30 it gives 22 such regions six distinct
values, and 279 regions of min_sites 1 with more.
"""
import os
import subprocess

import pytest

from pomfret_amd.abi import DmrConfig

from tests import _fixtures as fx
from tests._perm_ref import perm_ref_batch
from tests.test_dmr_gpu import _dmr_ref
from tests.test_hapmeth_dmr_gpu import DHEADER, HEADER, LCFG, _dmr_text
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHEADER = DHEADER[:-1] + "\treads_h1\treads_h2\tperm_p\n"
N_PERM = 99


def _cfg(min_sites):
    return DmrConfig(min_cov=3, min_delta_pct=30, max_gap=1000, min_sites=min_sites)


def _perm_text(dmr_text, tests, n_perm=N_PERM):
    """dmr_text's lines with the three columns; tests: (start, end) -> (reads_h1, reads_h2, hits, status)."""
    lines = [PHEADER]
    for x in dmr_text.splitlines()[1:]:
        c = x.split("\t")
        h1, h2, hits, status = tests[(int(c[1]), int(c[2]))]
        lines.append("%s\t%d\t%d\t%s\n" % (x, h1, h2, "%.6g" % ((hits + 1) / (n_perm + 1)) if status == 0 else "."))
    return "".join(lines)


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_perm")
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
    tests = {}
    for seed in (1, 2):
        ref = perm_ref_batch(pb, N_PERM, seed)
        tests[seed] = {reg: (int(ref["n_reads"][k][0]), int(ref["n_reads"][k][1]), int(ref["hits"][k]), int(ref["status"][k]))
                       for k, reg in enumerate(regs)}
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, fisher_exact(c[0], c[1], c[2], c[3])[3]))
    dmr, perm = {}, {}
    for ms in (1, 2):
        dmr[ms] = _dmr_text(pos, cnt, _cfg(ms))
        perm[ms] = _perm_text(dmr[ms], tests[1])
        ps = [x.split("\t")[13] for x in perm[ms].splitlines()[1:]]
        assert len([p for p in ps if p != "."]) >= 10 and len({p for p in ps if p != "."}) >= 2
        body = dmr[ms].splitlines()[1:]
        assert any("h1>h2" in x for x in body) and any("h1<h2" in x for x in body)
    kept = [x for x in dmr[1].splitlines()[1:] if float(x.split("\t")[10]) <= 0.01]
    assert 0 < len(kept) < len(dmr[1].splitlines()) - 1     # dmr_max_p 0.01 keeps a proper subset
    assert len(dmr[2]) < len(dmr[1])
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", text="".join(lines), dmr=dmr, perm=perm,
                perm_seed2=_perm_text(dmr[2], tests[2]), n_per=per.n_recs)


def _run(case, name, min_sites=2, dmr_perm=N_PERM, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=_cfg(min_sites),
                        dmr_perm=dmr_perm, **kw)
    assert open(res["path"]).read() == case["text"]
    return res, open(res["dmr_path"]).read()


@pytest.mark.parametrize("min_sites", [1, 2])
def test_file_equals_cpu_text(case, min_sites):
    res, text = _run(case, f"a{min_sites}", min_sites)
    assert text == case["perm"][min_sites]
    ps = [x.split("\t")[13] for x in text.splitlines()[1:]]
    assert res["n_tested"] == len([p for p in ps if p != "."]) and res["n_untested"] == ps.count(".")
    assert res["n_regions"] == len(ps) and res["perm_ms_kernels"] > 0
    if min_sites == 1:
        assert res["perm_records"] == case["n_per"]      # every region was a window of the second pass


def test_without_dmr_perm_same_region_file(case):
    res, text = _run(case, "plain", 2, dmr_perm=0)
    assert text == case["dmr"][2] and "n_tested" not in res


def test_host_fetch_same_bytes(case):
    _, text = _run(case, "h", host_fetch=True, threads=2)
    assert text == case["perm"][2]


@pytest.mark.parametrize("chunk,min_sites", [(7_000, 1), (33_333, 2), (100_000, 2)])
def test_chunk_size_same_bytes(case, chunk, min_sites):
    # job_windows 5 cuts the second pass into several jobs as well
    _, text = _run(case, f"c{chunk}_{min_sites}", min_sites, chunk_size=chunk, job_windows=5)
    assert text == case["perm"][min_sites]


def test_max_p_is_the_matching_subset(case):
    res, text = _run(case, "p", 1, dmr_max_p=0.01)
    full = case["perm"][1].splitlines(keepends=True)
    exp = [full[0]] + [x for x in full[1:] if float(x.split("\t")[10]) <= 0.01]
    assert 1 < len(exp) < len(full) and text == "".join(exp) and res["n_regions"] == len(exp) - 1
    assert res["n_tested"] + res["n_untested"] == len(exp) - 1 and res["perm_records"] < case["n_per"]


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3",
                        "--dmr-delta", "30", "--dmr-gap", "1000", "--dmr-min-sites", "2", "--dmr-perm", str(N_PERM),
                        "--dmr-seed", "1", case["bam"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.bed").read() == case["text"]
    assert open(out + ".hapmeth.dmr.bed").read() == case["perm"][2]
    assert "regions tested" in r.stderr and "permutation kernels" in r.stderr


def test_seed_changes_perm_p_only(case):
    _, text = _run(case, "s2", 2, dmr_seed=2)
    assert text == case["perm_seed2"] and text != case["perm"][2]
    a, b = case["perm"][2].splitlines(), text.splitlines()
    assert len(a) == len(b) and all(x.split("\t")[:13] == y.split("\t")[:13] for x, y in zip(a, b))
