"""`hapmeth --dmr --dmr-hmm` end to end on the device: pf_hapmeth_run_hmm
(hapmeth_files, the CLI) over test_hapmeth_dmr_gpu.py's haplotagged fixture BAM
against text built on the CPU: the host fetch of one window spanning the reads,
the oracle's loader, the literal pileup reference, the literal model reference
(tests/_dmr_hmm_ref.py) with its pooled-delta filter, and the Fisher test.
Every comparison is on bytes; in every run the .hapmeth.bed is the text a run
without --dmr writes, and a run without dmr_hmm writes the threshold rule's
region file as before.

On this fixture (14,424 sites, 2,432 informative at min_cov 5, four chains at
gap 1000) the model at its defaults has 140 runs, 46 of them with 5 CpGs and
more.  The pooled-delta filter at 40 % keeps 7 of those 46, fewer than 10 per
direction, so min_sites is 2 here: 32 kept regions, 20 h1>h2 and 12 h1<h2, the
longest of 9 CpGs (asserted on the reference text before any device run).
"""
import os
import subprocess

import pytest

from pomfret_amd.abi import AssignConfig, DmrConfig, HmmConfig

from tests import _fixtures as fx
from tests._assign_ref import assign_lines, assign_ref_batch
from tests._dmr_hmm_ref import hmm_ref
from tests._perm_ref import perm_ref_batch
from tests._tagcheck_ref import region_lines, tagcheck_lines, tagcheck_ref_batch
from tests.test_hapmeth_assign_gpu import _assign_text
from tests.test_hapmeth_dmr_gpu import DHEADER, HEADER, LCFG, _dmr_text
from tests.test_hapmeth_perm_gpu import _perm_text
from tests.test_hapmeth_tagcheck_gpu import _texts
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=1000, min_sites=2)
HMM = HmmConfig()
RULE = AssignConfig()                            # 3 bits, 2 calls: --assign's and --tag-check's defaults
N_PERM = 99


def _hmm_text(kept):
    from pomfret_amd import fisher_exact
    lines = [DHEADER]
    for r in kept:
        m1, u1, m2, u2 = r["sum"]
        lines.append("chrS\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%.4f\t%.6g\n" % (
            r["start"], r["end"], r["n_sites"], "h1>h2" if r["sign"] > 0 else "h1<h2", m1, u1, m2, u2,
            m1 / (m1 + u1) - m2 / (m2 + u2), fisher_exact(m1, u1, m2, u2)[3]))
    return "".join(lines)


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_dmr_hmm")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
        wb, _ = oracle_lib.load_reads(LCFG, one)
        win_off, pos, cnt = _pile_ref(wb)
        ref = hmm_ref(pos, cnt, CFG, HMM)
        # the second pass on the CPU: the kept regions are the windows
        regs = [(r["start"], r["end"]) for r in ref["kept"]]
        per, qnames, _ = bf.fetch_windows("chrS", [s for s, _ in regs], [e for _, e in regs], readback=0)
    pb, rec_read = oracle_lib.load_reads(LCFG, per)
    qname_of_read = {int(r): qnames[i] for i, r in enumerate(rec_read.tolist()) if r != 0xFFFFFFFF}
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, fisher_exact(c[0], c[1], c[2], c[3])[3]))
    dmr = _hmm_text(ref["kept"])
    body = dmr.splitlines()[1:]
    assert len([x for x in body if "h1>h2" in x]) >= 10 and len([x for x in body if "h1<h2" in x]) >= 10
    assert len(ref["all"]) > len(ref["kept"]) and max(r["n_sites"] for r in ref["kept"]) >= 5
    threshold = _dmr_text(pos, cnt, CFG)
    assert threshold != dmr
    # the three second-pass features on the model's regions
    pr = perm_ref_batch(pb, N_PERM, 1)
    perm = _perm_text(dmr, {reg: (int(pr["n_reads"][k][0]), int(pr["n_reads"][k][1]), int(pr["hits"][k]), int(pr["status"][k]))
                            for k, reg in enumerate(regs)})
    bits = int(round(RULE.min_llr * 65536))
    ar = assign_ref_batch(pb, CFG.min_cov, RULE.min_calls, bits)
    tr = tagcheck_ref_batch(pb, CFG.min_cov, RULE.min_calls, bits)
    a_per, t_per = {}, {}
    for w, reg in enumerate(regs):
        a_per[reg] = assign_lines(dict(ar, win_read_off=ar["win_read_off"][w:w + 2]), "chrS", [reg[0]], [reg[1]], qname_of_read)
        one_w = dict(tr, win_read_off=tr["win_read_off"][w:w + 2], win_n=tr["win_n"][w:w + 1])
        t_per[reg] = (tagcheck_lines(one_w, "chrS", [reg[0]], [reg[1]], qname_of_read), region_lines(one_w, "chrS", [reg[0]], [reg[1]]))
    assign, tagcheck = _assign_text(dmr, a_per), _texts(dmr, t_per)
    assert len(assign.splitlines()) > 10 and len(tagcheck[0].splitlines()) > 10
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", text="".join(lines), dmr=dmr, threshold=threshold, ref=ref,
                perm=perm, assign=assign, tagcheck=tagcheck)


def _run(case, name, hmm=HMM, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=CFG, dmr_hmm=hmm, **kw)
    assert res["dmr_path"] == str(case["tmp"] / name) + ".hapmeth.dmr.bed"
    assert open(res["path"]).read() == case["text"]          # the text a run without --dmr writes
    return res, open(res["dmr_path"]).read()


def test_file_equals_cpu_text(case):
    res, text = _run(case, "a")
    assert text == case["dmr"]
    ref = case["ref"]
    assert res["n_regions"] == len(ref["kept"]) and res["n_informative"] == ref["n_informative"]
    assert res["n_chains"] == ref["n_chains"] and res["hmm_ms_kernels"] > 0 and res["dmr_ms_kernels"] >= res["hmm_ms_kernels"]


def test_without_dmr_hmm_the_threshold_rules_file(case):
    res, text = _run(case, "plain", hmm=None)
    assert text == case["threshold"] and "n_chains" not in res and "hmm_ms_kernels" not in res


@pytest.mark.parametrize("chunk", [7_000, 33_333, 100_000])
def test_chunk_size_same_bytes(case, chunk):
    res, text = _run(case, f"c{chunk}", chunk_size=chunk, job_windows=5)
    assert text == case["dmr"] and res["n_windows"] >= 1 and res["n_chains"] == case["ref"]["n_chains"]


def test_host_fetch_same_bytes(case):
    _, text = _run(case, "h", host_fetch=True, threads=2)
    assert text == case["dmr"]


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    base = [exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "5", "--dmr-delta", "40",
            "--dmr-gap", "1000", "--dmr-min-sites", "2", "--dmr-hmm"]
    for extra in ([], ["--dmr-hmm-site-cost", "2", "--dmr-hmm-switch", "8.0"]):
        r = subprocess.run(base + extra + [case["bam"]], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert open(out + ".hapmeth.bed").read() == case["text"]
        assert open(out + ".hapmeth.dmr.bed").read() == case["dmr"]
        assert "%d chains, %d regions, model kernels" % (case["ref"]["n_chains"], len(case["ref"]["kept"])) in r.stderr


def test_other_costs_other_regions(case):
    """The two costs reach the kernels: site cost 1 against the reference at site cost 1."""
    h = HmmConfig(site_cost=1.0, switch=8.0)
    ref = hmm_ref(*_pile(case), CFG, h)
    _, text = _run(case, "s1", hmm=h)
    assert text == _hmm_text(ref["kept"]) != case["dmr"]


def _pile(case):
    rows = [x.split("\t") for x in case["text"].splitlines()[1:]]
    return [int(c[1]) for c in rows], [[int(v) for v in c[3:9]] for c in rows]


def test_with_perm_assign_and_tag_check(case):
    """The second pass works on the model's regions: the first eleven columns
    are the plain run's bytes, the perm columns, the assign lines and the
    tag-check lines those of the references run on these regions."""
    res, text = _run(case, "all", dmr_perm=N_PERM, assign=RULE, tag_check=True)
    assert text == case["perm"]
    assert "".join("\t".join(x.split("\t")[:11]) + "\n" for x in text.splitlines()) == case["dmr"]
    assert open(res["assign_path"]).read() == case["assign"]
    assert (open(res["tagcheck_path"]).read(), open(res["tagcheck_regions_path"]).read()) == case["tagcheck"]
    assert res["n_tested"] + res["n_untested"] == res["n_regions"] == len(case["ref"]["kept"])
    assert res["n_chains"] == case["ref"]["n_chains"]
    # tag-check alone names the rule without turning --assign on
    res, text = _run(case, "tc", tag_check=True)
    assert text == case["dmr"] and "assign_path" not in res
    assert (open(res["tagcheck_path"]).read(), open(res["tagcheck_regions_path"]).read()) == case["tagcheck"]
    assert not os.path.exists(str(case["tmp"] / "tc") + ".hapmeth.assign.tsv")
