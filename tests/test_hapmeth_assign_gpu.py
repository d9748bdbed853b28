"""`hapmeth --dmr --assign` end to end on the device: pf_hapmeth_run_assign
(hapmeth_files, the CLI) over a haplotagged fixture BAM, against text built on
the CPU: the regions of the literal region reference, the host fetch with those
regions as the windows, the oracle's loader, and the literal assignment
reference (tests/_assign_ref.py).  Every comparison is on bytes; in every run
the .hapmeth.bed and the .hapmeth.dmr.bed are the text a run without --assign
writes.

The fixture is test_hapmeth_perm_gpu.py's at coverage 30: at 12x the reference
text does not hold enough lines of each kind (1, 2 and "."); the conditions are
asserted on the reference text before any device run.
"""
import os
import subprocess

import numpy as np
import pytest

from pomfret_amd.abi import AssignConfig, DmrConfig

from tests import _fixtures as fx
from tests._assign_ref import HEADER as AHEADER
from tests._assign_ref import assign_lines, assign_ref_batch
from tests.test_dmr_gpu import _dmr_ref
from tests.test_hapmeth_dmr_gpu import HEADER, LCFG, _dmr_text
from tests.test_pileup_gpu import _cfg as _batch_cfg
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (min_sites, bits, calls) -> the least number of lines of each kind in the reference text
SETS = {(1, 2.0, 1): 20, (2, 3.0, 2): 5}
MIN_COV = 3


def _cfg(min_sites):
    return DmrConfig(min_cov=MIN_COV, min_delta_pct=30, max_gap=1000, min_sites=min_sites)


def _acfg(bits, calls):
    return AssignConfig(min_calls=calls, min_llr=bits)


def _assign_text(dmr_text, per_region):
    """The assign file of the regions of dmr_text, in its order; per_region: (start, end) -> lines."""
    out = [AHEADER]
    for x in dmr_text.splitlines()[1:]:
        c = x.split("\t")
        out += per_region[(int(c[1]), int(c[2]))]
    return "".join(out)


def _kinds(text):
    hp = [x.split("\t")[6] for x in text.splitlines()[1:]]
    return hp.count("1"), hp.count("2"), hp.count(".")


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_assign")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, coverage=30, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
        wb, _ = oracle_lib.load_reads(LCFG, one)
        win_off, pos, cnt = _pile_ref(wb)
        # the second pass on the CPU: the regions (min_sites 1 holds them all) are the windows
        regs = [(r["start"], r["end"]) for r in _dmr_ref(pos, cnt, _cfg(1))["all"]]
        per, qnames, _ = bf.fetch_windows("chrS", [s for s, _ in regs], [e for _, e in regs], readback=0)
    pb, rec_read = oracle_lib.load_reads(LCFG, per)
    qname_of_read = {int(r): qnames[i] for i, r in enumerate(rec_read.tolist()) if r != 0xFFFFFFFF}
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, fisher_exact(c[0], c[1], c[2], c[3])[3]))
    dmr, text = {}, {}
    for (ms, bits, calls), least in SETS.items():
        ref = assign_ref_batch(pb, MIN_COV, calls, int(round(bits * 65536)))
        per_region = {}
        for w, reg in enumerate(regs):
            one_w = dict(ref, win_read_off=ref["win_read_off"][w:w + 2])
            per_region[reg] = assign_lines(one_w, "chrS", [reg[0]], [reg[1]], qname_of_read)
        dmr[ms] = _dmr_text(pos, cnt, _cfg(ms))
        text[ms] = _assign_text(dmr[ms], per_region)
        kinds = _kinds(text[ms])
        assert min(kinds) >= least, (ms, bits, calls, kinds)
        if ms == 1:
            per_region_1 = per_region
    kept = [x for x in dmr[1].splitlines()[1:] if float(x.split("\t")[10]) <= 0.01]
    assert 0 < len(kept) < len(dmr[1].splitlines()) - 1     # dmr_max_p 0.01 keeps a proper subset
    text_p = _assign_text("".join([dmr[1].splitlines(keepends=True)[0]] + [x + "\n" for x in kept]), per_region_1)
    assert AHEADER != text_p != text[1]
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", text="".join(lines), dmr=dmr, assign=text,
                assign_p=text_p, n_per=per.n_recs, per=per, pb=pb)


def _run(case, name, key=(2, 3.0, 2), assign=True, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    ms, bits, calls = key
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=_cfg(ms),
                        assign=_acfg(bits, calls) if assign else None, **kw)
    assert open(res["path"]).read() == case["text"]
    dmr_text = open(res["dmr_path"]).read()
    if not kw.get("dmr_perm") and "dmr_max_p" not in kw:
        assert dmr_text == case["dmr"][ms]           # the region file of a run without --assign
    return res, (open(res["assign_path"]).read() if assign else None), dmr_text


@pytest.mark.parametrize("key", sorted(SETS))
def test_file_equals_cpu_text(case, key):
    res, text, _ = _run(case, "a%d" % key[0], key)
    assert res["assign_path"] == str(case["tmp"] / ("a%d" % key[0])) + ".hapmeth.assign.tsv"
    assert text == case["assign"][key[0]]
    h1, h2, dot = _kinds(text)
    assert res["n_assign_lines"] == h1 + h2 + dot and res["n_assigned"] == h1 + h2
    assert (res["n_assigned_h1"], res["n_assigned_h2"]) == (h1, h2) and res["assign_ms_kernels"] > 0
    if key[0] == 1:
        assert res["assign_records"] == case["n_per"]    # every region was a window of the second pass


def test_without_assign_no_file_no_keys(case):
    res, _, _ = _run(case, "plain", assign=False)
    assert not os.path.exists(str(case["tmp"] / "plain") + ".hapmeth.assign.tsv")
    assert not [k for k in res if "assign" in k]


def test_with_dmr_perm_both_unchanged(case):
    """One second pass serves both: the assign file is the one without
    --dmr-perm, the region file the one of --dmr-perm alone."""
    res, text, dmr_both = _run(case, "both", dmr_perm=99)
    res_p, _, dmr_perm = _run(case, "perm", assign=False, dmr_perm=99)
    assert text == case["assign"][2] and dmr_both == dmr_perm and "perm_p" in dmr_both.splitlines()[0]
    assert res["n_tested"] == res_p["n_tested"] and res["perm_records"] == res_p["perm_records"] == res["assign_records"]


def test_host_fetch_same_bytes(case):
    _, text, _ = _run(case, "h", host_fetch=True, threads=2)
    assert text == case["assign"][2]


@pytest.mark.parametrize("chunk,ms", [(7_000, 1), (33_333, 2), (100_000, 2)])
def test_chunk_size_same_bytes(case, chunk, ms):
    # job_windows 5 cuts the second pass into several jobs as well
    key = [k for k in SETS if k[0] == ms][0]
    _, text, _ = _run(case, f"c{chunk}_{ms}", key, chunk_size=chunk, job_windows=5)
    assert text == case["assign"][ms]


def test_max_p_is_the_kept_regions_lines(case):
    res, text, _ = _run(case, "p", (1, 2.0, 1), dmr_max_p=0.01)
    assert text == case["assign_p"] and res["n_assign_lines"] == len(text.splitlines()) - 1
    assert res["assign_records"] < case["n_per"]


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3",
                        "--dmr-delta", "30", "--dmr-gap", "1000", "--dmr-min-sites", "2", "--assign",
                        "--assign-min-llr", "3", "--assign-min-calls", "2", case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.bed").read() == case["text"]
    assert open(out + ".hapmeth.dmr.bed").read() == case["dmr"][2]
    assert open(out + ".hapmeth.assign.tsv").read() == case["assign"][2]
    h1, h2, dot = _kinds(case["assign"][2])
    assert f"{h1 + h2 + dot} candidate reads scored, {h1 + h2} assigned ({h1} h1 / {h2} h2)" in r.stderr
    assert "assign kernels" in r.stderr
    # the defaults are 3 bits and 2 calls
    out = str(case["tmp"] / "cli_d")
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3", "--dmr-delta", "30",
                        "--dmr-gap", "1000", "--dmr-min-sites", "2", "--assign", case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.assign.tsv").read() == case["assign"][2]


def _agreement(own, hidden, res):
    """(assigned, of those with their own tag back) over the hidden reads."""
    new = np.asarray(res["hp"])[hidden]
    done = new < 2
    return int(done.sum()), int((new[done] == own[hidden][done]).sum())


def test_hidden_tag_agreement(case, gpu_ctx):
    """A record, not a threshold: every third tagged read of the second pass's
    batch is hidden (254) and assigned at 2.0 bits / 1 call from the rest; how
    many get their own tag back.  Device and reference agree on the figure,
    which profiles/assign/README.md records."""
    pb = case["pb"]
    own = np.asarray(pb.read_hp, np.uint8)
    tagged = np.flatnonzero(own < 2)
    hidden = tagged[::3]
    hp = own.copy()
    hp[hidden] = 254
    ref = assign_ref_batch(pb, MIN_COV, 1, 2 << 16, hp=hp)
    db = gpu_ctx.upload_aln(_batch_cfg(), case["per"], LCFG)
    try:
        got = db.assign(AssignConfig(min_cov=MIN_COV, min_calls=1, min_llr=2.0), read_hp=hp)
    finally:
        db.free()
    a_ref, a_got = _agreement(own, hidden, ref), _agreement(own, hidden, got)
    scored = int((np.asarray(ref["n_used"])[hidden] > 0).sum())
    print(f"hidden-tag agreement: {hidden.size} hidden reads, {scored} scored, {a_ref[0]} assigned, {a_ref[1]} with their own tag")
    assert a_got == a_ref and np.array_equal(got["hp"], ref["hp"]) and np.array_equal(got["llr"], ref["llr"])
