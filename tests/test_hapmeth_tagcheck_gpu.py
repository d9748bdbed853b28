"""`hapmeth --dmr --tag-check` end to end on the device: pf_hapmeth_run_tagcheck
(hapmeth_files, the CLI) over a haplotagged fixture BAM, against text built on
the CPU: the regions of the literal region reference, the host fetch with those
regions as the windows, the oracle's loader, and the literal tag-check reference
(tests/_tagcheck_ref.py).  Every comparison is on bytes; the files of the other
features are the ones a run without --tag-check writes.

The fixture is test_hapmeth_assign_gpu.py's (coverage 30).  The reference text
is asserted to hold lines of all three verdicts (ok, flip, ".") at both
threshold sets before any device run.
"""
import os
import subprocess

import pytest

from pomfret_amd.abi import AssignConfig, DmrConfig

from tests import _fixtures as fx
from tests._tagcheck_ref import HEADER as THEADER
from tests._tagcheck_ref import REGIONS_HEADER, region_lines, tagcheck_lines, tagcheck_ref_batch
from tests.test_dmr_gpu import _dmr_ref
from tests.test_hapmeth_dmr_gpu import LCFG, _dmr_text
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (min_sites, bits, calls) -> the least number of lines of each verdict in the reference text: every verdict
# occurs.  (2, 3.0, 2) are the CLI's defaults, where the reference has 421 ok, 4 flip and 106 undecided lines;
# at (1, 2.0, 1) it has 6,966, 334 and 648
SETS = {(1, 2.0, 1): 100, (2, 3.0, 2): 1}
MIN_COV = 3
SUFFIXES = (".hapmeth.tagcheck.tsv", ".hapmeth.tagcheck.regions.tsv")


def _cfg(min_sites):
    return DmrConfig(min_cov=MIN_COV, min_delta_pct=30, max_gap=1000, min_sites=min_sites)


def _texts(dmr_text, per_region):
    """The two files for the regions of dmr_text, in its order; per_region: (start, end) -> (read lines, region line)."""
    reads, regions = [THEADER], [REGIONS_HEADER]
    for x in dmr_text.splitlines()[1:]:
        c = x.split("\t")
        reads += per_region[(int(c[1]), int(c[2]))][0]
        regions += per_region[(int(c[1]), int(c[2]))][1]
    return "".join(reads), "".join(regions)


def _kinds(text):
    v = [x.split("\t")[7] for x in text.splitlines()[1:]]
    return v.count("ok"), v.count("flip"), v.count(".")


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_tagcheck")
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
    dmr, text, per_region_of = {}, {}, {}
    for (ms, bits, calls), least in SETS.items():
        ref = tagcheck_ref_batch(pb, MIN_COV, calls, int(round(bits * 65536)))
        per_region = {}
        for w, reg in enumerate(regs):
            one_w = dict(ref, win_read_off=ref["win_read_off"][w:w + 2], win_n=ref["win_n"][w:w + 1])
            per_region[reg] = (tagcheck_lines(one_w, "chrS", [reg[0]], [reg[1]], qname_of_read),
                               region_lines(one_w, "chrS", [reg[0]], [reg[1]]))
        dmr[ms] = _dmr_text(pos, cnt, _cfg(ms))
        text[ms] = _texts(dmr[ms], per_region)
        per_region_of[ms] = per_region
        kinds = _kinds(text[ms][0])
        assert min(kinds) >= least, (ms, bits, calls, kinds)
        assert len(text[ms][1].splitlines()) == len(dmr[ms].splitlines())       # one line per region
        print(f"tag check at {bits} bits / {calls} call(s), min_sites {ms}: ok {kinds[0]}, flip {kinds[1]}, undecided {kinds[2]}, "
              f"concordance {kinds[0] / (kinds[0] + kinds[1]):.4f}")
    kept = [x for x in dmr[1].splitlines()[1:] if float(x.split("\t")[10]) <= 0.01]
    assert 0 < len(kept) < len(dmr[1].splitlines()) - 1     # dmr_max_p 0.01 keeps a proper subset
    text_p = _texts("".join([dmr[1].splitlines(keepends=True)[0]] + [x + "\n" for x in kept]), per_region_of[1])
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", dmr=dmr, text=text, text_p=text_p, n_per=per.n_recs)


def _run(case, name, key=(2, 3.0, 2), tag_check=True, assign=False, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    ms, bits, calls = key
    rule = AssignConfig(min_calls=calls, min_llr=bits)
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=_cfg(ms),
                        assign=rule if assign else None, tag_check=(True if assign else rule) if tag_check else False, **kw)
    out = dict(res=res, bed=open(res["path"]).read(), dmr=open(res["dmr_path"]).read())
    if assign:
        out["assign"] = open(res["assign_path"]).read()
    if tag_check:
        out["text"] = (open(res["tagcheck_path"]).read(), open(res["tagcheck_regions_path"]).read())
    return out


@pytest.fixture(scope="module")
def plain(case):
    """Runs without --tag-check: their files are what every other run must leave unchanged."""
    return {(a, p): _run(case, f"plain_{int(a)}_{p}", tag_check=False, assign=a, dmr_perm=p) for a in (False, True) for p in (0, 99)}


@pytest.mark.parametrize("key", sorted(SETS))
def test_files_equal_cpu_text(case, key):
    r = _run(case, "t%d" % key[0], key)
    res = r["res"]
    assert res["tagcheck_path"] == str(case["tmp"] / ("t%d" % key[0])) + SUFFIXES[0]
    assert res["tagcheck_regions_path"] == str(case["tmp"] / ("t%d" % key[0])) + SUFFIXES[1]
    assert r["text"][0] == case["text"][key[0]][0] and r["text"][1] == case["text"][key[0]][1]
    assert r["dmr"] == case["dmr"][key[0]]
    ok, flip, dot = _kinds(r["text"][0])
    assert res["n_tagcheck_lines"] == ok + flip + dot and res["n_tagcheck_regions"] == len(r["text"][1].splitlines()) - 1
    assert sum(res["tagcheck_ok"]) == ok and sum(res["tagcheck_flip"]) == flip and sum(res["tagcheck_undecided"]) == dot
    hp_ok = [x.split("\t")[4] for x in r["text"][0].splitlines()[1:] if x.endswith("\tok")]
    assert res["tagcheck_ok"] == [hp_ok.count("1"), hp_ok.count("2")]
    assert res["tagcheck_concordance"] == ok / (ok + flip) and res["tagcheck_ms_kernels"] > 0
    assert not [k for k in res if "assign" in k]         # the rule alone turns --assign not on
    assert not os.path.exists(str(case["tmp"] / ("t%d" % key[0])) + ".hapmeth.assign.tsv")
    if key[0] == 1:
        assert res["tagcheck_records"] == case["n_per"]  # every region was a window of the second pass


def test_no_option_no_files_no_keys(case, plain):
    for (a, p), r in plain.items():
        for s in SUFFIXES:
            assert not os.path.exists(str(case["tmp"] / f"plain_{int(a)}_{p}") + s)
        assert not [k for k in r["res"] if "tagcheck" in k]


@pytest.mark.parametrize("assign,perm", [(False, 99), (True, 0), (True, 99)])
def test_with_perm_and_assign_everything_unchanged(case, plain, assign, perm):
    """One second pass serves all three: the tag-check files are the ones of
    --tag-check alone; the .bed, the region file with its perm columns and the
    assign file are byte-identical to a run without --tag-check."""
    r = _run(case, f"all_{int(assign)}_{perm}", assign=assign, dmr_perm=perm)
    base = plain[(assign, perm)]
    assert r["text"] == case["text"][2]
    assert r["bed"] == base["bed"] == plain[(False, 0)]["bed"] and r["dmr"] == base["dmr"]
    assert ("perm_p" in r["dmr"].splitlines()[0]) == bool(perm)
    if assign:
        assert r["assign"] == base["assign"] and r["res"]["n_assign_lines"] == base["res"]["n_assign_lines"]
        assert r["res"]["assign_records"] == r["res"]["tagcheck_records"]
    if perm:
        assert r["res"]["perm_records"] == r["res"]["tagcheck_records"] == base["res"]["perm_records"]


def test_host_fetch_same_bytes(case):
    assert _run(case, "h", host_fetch=True, threads=2)["text"] == case["text"][2]


@pytest.mark.parametrize("chunk,ms", [(7_000, 1), (33_333, 2)])
def test_chunk_size_same_bytes(case, chunk, ms):
    # job_windows 5 cuts the second pass into several jobs as well
    key = [k for k in SETS if k[0] == ms][0]
    assert _run(case, f"c{chunk}_{ms}", key, chunk_size=chunk, job_windows=5)["text"] == case["text"][ms]


def test_max_p_is_the_kept_regions_lines(case):
    r = _run(case, "p", (1, 2.0, 1), dmr_max_p=0.01)
    assert r["text"] == case["text_p"] and r["res"]["n_tagcheck_regions"] == len(case["text_p"][1].splitlines()) - 1
    assert r["res"]["tagcheck_records"] < case["n_per"]


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    base = [exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3", "--dmr-delta", "30",
            "--dmr-gap", "1000"]
    r = subprocess.run(base + ["--dmr-min-sites", "1", "--tag-check", "--assign-min-llr", "2", "--assign-min-calls", "1", case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.dmr.bed").read() == case["dmr"][1]
    assert (open(out + SUFFIXES[0]).read(), open(out + SUFFIXES[1]).read()) == case["text"][1]
    assert not os.path.exists(out + ".hapmeth.assign.tsv")
    ok, flip, dot = _kinds(case["text"][1][0])
    assert f"{ok + flip + dot} tagged reads scored, {ok} ok" in r.stderr and f"{flip} flip" in r.stderr
    assert f"{dot} undecided, concordance {ok / (ok + flip):.4f}" in r.stderr and "tag-check kernels" in r.stderr
    # the defaults are 3 bits and 2 calls, with --assign beside it or without
    for extra in ([], ["--assign"]):
        r = subprocess.run(base + ["--dmr-min-sites", "2", "--tag-check"] + extra + [case["bam"]], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert (open(out + SUFFIXES[0]).read(), open(out + SUFFIXES[1]).read()) == case["text"][2]
        assert os.path.exists(out + ".hapmeth.assign.tsv") == bool(extra)
    # no region passes --dmr-max-p 0: the headers alone, and no concordance to print, not a zero
    out = str(case["tmp"] / "cli_none")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3", "--dmr-delta", "30",
                        "--dmr-gap", "1000", "--dmr-max-p", "0", "--tag-check", case["bam"]], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert (open(out + SUFFIXES[0]).read(), open(out + SUFFIXES[1]).read()) == (THEADER, REGIONS_HEADER)
    assert "0 tagged reads scored, 0 ok" in r.stderr and "concordance n/a" in r.stderr
