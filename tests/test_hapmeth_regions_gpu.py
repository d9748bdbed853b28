"""`hapmeth --regions` end to end on the device: pf_hapmeth_run_regions
(hapmeth_files, the CLI) over test_hapmeth_dmr_hmm_gpu.py's haplotagged fixture
BAM against text built on the CPU: the host fetch of one window spanning the
reads, the oracle's loader, the literal pileup reference, the literal region
reference and writer (tests/_regions_ref.py), and the permutation, assign and
tag-check references on the eligible regions' windows.  Every comparison is on
bytes; in every run the .hapmeth.bed is the text a run without regions writes.

The BED is made here from the model reference's own regions of the fixture (32
kept ones, 20 h1>h2 and 12 h1<h2: test_hapmeth_dmr_hmm_gpu.py), so at least 10
tested regions in each direction hold by construction (asserted on the
reference text before any device run), plus widened copies, overlapping pairs,
a duplicate, regions without an informative site, an empty one, one on a contig
the BAM does not have, one past the run's range and one over 1,000,000 bases,
written in shuffled order.
"""
import os
import subprocess

import numpy as np
import pytest

from pomfret_amd.abi import AssignConfig, DmrConfig, HmmConfig

from tests import _fixtures as fx
from tests._assign_ref import assign_lines, assign_ref_batch
from tests._dmr_hmm_ref import hmm_ref
from tests._perm_ref import perm_ref_batch
from tests._regions_ref import HEADER as RHEADER
from tests._regions_ref import eligible, region_ref, regions_text
from tests._tagcheck_ref import region_lines, tagcheck_lines, tagcheck_ref_batch
from tests.test_hapmeth_assign_gpu import AHEADER
from tests.test_hapmeth_dmr_gpu import HEADER, LCFG
from tests.test_hapmeth_dmr_hmm_gpu import _hmm_text
from tests.test_hapmeth_tagcheck_gpu import REGIONS_HEADER, THEADER
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=1000, min_sites=2)
HMM = HmmConfig()
RULE = AssignConfig()
N_PERM = 99
FIELDS = ("n_cpg", "n_sites", "n_pos", "n_neg", "sum", "evidence")


def _bed_regions(kept, pos, cnt, lo, hi):
    """(chrom, start, end, name) in the order they are written."""
    reg = [("chrS", r["start"], r["end"], "hmm%d" % k) for k, r in enumerate(kept)]
    reg += [("chrS", r["start"] - 50, r["end"] + 50, "wide%d" % k) for k, r in enumerate(kept[:6])]
    for k in range(8, 14, 2):                                  # overlapping pairs: two neighbours, and a shifted copy
        reg += [("chrS", kept[k]["start"], kept[k + 1]["end"], "pair%d" % k),
                ("chrS", kept[k]["start"] + 1, kept[k]["end"] + 30, "shift%d" % k)]
    reg += [("chrS", kept[3]["start"], kept[3]["end"], "again")]
    # no informative site: between two neighbouring informative sites with a site between them, and before every site
    inf = [i for i, c in enumerate(cnt.reshape(-1, 6).tolist()) if c[0] + c[1] >= CFG.min_cov and c[2] + c[3] >= CFG.min_cov]
    gaps = [(a, b) for a, b in zip(inf, inf[1:]) if b - a > 1]
    a, b = gaps[len(gaps) // 2]
    reg += [("chrS", int(pos[a]) + 1, int(pos[b]), "covered_no_difference"), ("chrS", 10, 5000, "nothing_here"),
            ("chrS", int(pos[a]), int(pos[a]), "empty")]
    reg += [("chrNope", 5, 500, "unknown"), ("chrS", hi - 10, hi + 10, "outside"), ("chrS", 0, hi, "long")]
    order = np.random.default_rng(4).permutation(len(reg))
    return [reg[i] for i in order]


def _records(bed, pos, cnt, hi):
    """The kept regions' records, in the file's order."""
    keep = sorted((r for r in bed if r[0] == "chrS" and r[2] <= hi), key=lambda r: (r[1], r[2]))
    sums = region_ref(pos, cnt, CFG, [r[1] for r in keep], [r[2] for r in keep])
    return [dict({k: (sums[k][i].tolist() if k == "sum" else int(sums[k][i])) for k in FIELDS}, chrom="chrS", start=r[1],
                 end=r[2], name=r[3]) for i, r in enumerate(keep)]


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_regions")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    assert hi > 1_000_000                         # the run's range [0, hi) holds a region too long to test
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
        wb, _ = oracle_lib.load_reads(LCFG, one)
        win_off, pos, cnt = _pile_ref(wb)
        model = hmm_ref(pos, cnt, CFG, HMM)
        bed = _bed_regions(model["kept"], pos, cnt, lo, hi)
        rec = _records(bed, pos, cnt, hi)
        # the second pass on the CPU: every region that can be eligible under some option of these tests
        regs = sorted({(r["start"], r["end"]) for r in rec if eligible(r, CFG, 1.0)})
        per, qnames, _ = bf.fetch_windows("chrS", [s for s, _ in regs], [e for _, e in regs], readback=0)
    pb, rec_read = oracle_lib.load_reads(LCFG, per)
    qname_of_read = {int(r): qnames[i] for i, r in enumerate(rec_read.tolist()) if r != 0xFFFFFFFF}
    path = str(tmp / "given.bed")
    with open(path, "w") as f:
        f.write("# candidates\ntrack name=given\n")
        f.write("".join("%s\t%d\t%d\t%s\n" % r for r in bed).rstrip("\n"))      # no final newline
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, fisher_exact(c[0], c[1], c[2], c[3])[3]))
    pr = perm_ref_batch(pb, N_PERM, 1)
    tests = {reg: (int(pr["n_reads"][k][0]), int(pr["n_reads"][k][1]), int(pr["hits"][k]), int(pr["status"][k]))
             for k, reg in enumerate(regs)}
    bits = int(round(RULE.min_llr * 65536))
    ar = assign_ref_batch(pb, CFG.min_cov, RULE.min_calls, bits)
    tr = tagcheck_ref_batch(pb, CFG.min_cov, RULE.min_calls, bits)
    a_per, t_per = {}, {}
    for w, reg in enumerate(regs):
        a_per[reg] = assign_lines(dict(ar, win_read_off=ar["win_read_off"][w:w + 2]), "chrS", [reg[0]], [reg[1]], qname_of_read)
        one_w = dict(tr, win_read_off=tr["win_read_off"][w:w + 2], win_n=tr["win_n"][w:w + 1])
        t_per[reg] = (tagcheck_lines(one_w, "chrS", [reg[0]], [reg[1]], qname_of_read), region_lines(one_w, "chrS", [reg[0]], [reg[1]]))
    c = dict(tmp=tmp, bam=bam, bed=path, region=f"chrS:1-{hi}", lo=lo, hi=hi, text="".join(lines), rec=rec, model=model,
             tests=tests, a_per=a_per, t_per=t_per, plain=regions_text(rec))
    # the reference text holds what the tests are about, before any device run
    body = [x.split("\t") for x in _expected(c)[0].splitlines()[1:]]
    tested = [x for x in body if x[19] != "."]
    assert len([x for x in tested if x[8] == "h1>h2"]) >= 10 and len([x for x in tested if x[8] == "h1<h2"]) >= 10
    assert any(x[3] == "long" and x[17:] == [".", ".", ".", "."] and x[14] != "." for x in body)
    assert any(x[3] == "covered_no_difference" and int(x[4]) > 0 and x[5] == "0" for x in body)
    assert not any(x[3] in ("unknown", "outside") for x in body) and len(body) == len(bed) - 2
    assert [(int(x[1]), int(x[2])) for x in body] == sorted((int(x[1]), int(x[2])) for x in body)
    return c


def _expected(case, max_p=1.0, breaks=()):
    """(regions text with the permutation columns, assign text, (tag-check texts))."""
    el = [eligible(r, CFG, max_p, breaks) for r in case["rec"]]
    perm = [case["tests"][(r["start"], r["end"])] if e else None for r, e in zip(case["rec"], el)]
    text = regions_text(case["rec"], perm=perm, n_perm=N_PERM, breaks={"chrS": list(breaks)})
    keys = [(r["start"], r["end"]) for r, e in zip(case["rec"], el) if e]
    assign = "".join([AHEADER] + [x for k in keys for x in case["a_per"][k]])
    reads = "".join([THEADER] + [x for k in keys for x in case["t_per"][k][0]])
    regions = "".join([REGIONS_HEADER] + [x for k in keys for x in case["t_per"][k][1]])
    return text, assign, (reads, regions)


def _run(case, name, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=CFG, regions=case["bed"], **kw)
    assert res["regions_path"] == str(case["tmp"] / name) + ".hapmeth.regions.bed" and "dmr_path" not in res
    assert not os.path.exists(str(case["tmp"] / name) + ".hapmeth.dmr.bed")
    assert open(res["path"]).read() == case["text"]          # the text a run without regions writes
    return res, open(res["regions_path"]).read()


def test_file_equals_cpu_text(case):
    res, text = _run(case, "a")
    assert text == case["plain"] and text.startswith(RHEADER + "\n")
    assert res["n_regions"] == len(case["rec"]) and res["n_regions_unknown_contig"] == 1 and res["n_regions_outside"] == 1
    assert res["n_regions_split"] == 0 and res["n_tested"] == 0 and res["n_untested"] == 0 and res["regions_ms_kernels"] > 0


@pytest.mark.parametrize("jw", [3, 0])
@pytest.mark.parametrize("chunk", [7_000, 33_333, 100_000])
def test_chunk_size_and_job_size_same_bytes(case, chunk, jw):
    res, text = _run(case, f"c{chunk}_{jw}", chunk_size=chunk, job_windows=jw)
    assert text == case["plain"] and res["n_windows"] >= 1


def test_host_fetch_same_bytes(case):
    _, text = _run(case, "h", host_fetch=True, threads=2, chunk_size=33_333)
    assert text == case["plain"]


def test_whole_contig_keeps_the_region_past_the_range(case):
    """Without a range nothing is outside: the region past the reads is a line of zeros."""
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / "w"), dmr=CFG, regions=case["bed"], chunk_size=1_000_000)
    assert res["n_regions"] == len(case["rec"]) + 1 and res["n_regions_outside"] == 0
    got = open(res["regions_path"]).read().splitlines(keepends=True)
    extra = [x for x in got if x.split("\t")[3] == "outside"]
    assert len(extra) == 1 and extra[0].split("\t")[4:8] == ["0", "0", "0", "0"]
    assert "".join(x for x in got if x not in extra) == case["plain"]
    assert open(res["path"]).read() == case["text"]


def test_with_perm_assign_and_tag_check(case):
    exp, assign, tagcheck = _expected(case)
    res, text = _run(case, "all", dmr_perm=N_PERM, assign=RULE, tag_check=True, job_windows=7)
    assert text == exp
    assert "".join("\t".join(x.split("\t")[:17]) + "\n" for x in text.splitlines()) == case["plain"]
    assert [x.split("\t")[20] for x in text.splitlines()] == [x.split("\t")[20] for x in exp.splitlines()]       # perm_q
    assert open(res["assign_path"]).read() == assign
    assert (open(res["tagcheck_path"]).read(), open(res["tagcheck_regions_path"]).read()) == tagcheck
    n_p = len([x for x in exp.splitlines()[1:] if x.split("\t")[19] != "."])
    assert res["n_tested"] == n_p and res["n_tested"] + res["n_untested"] == res["n_regions"] == len(case["rec"])
    assert len(assign.splitlines()) > 10 and len(tagcheck[0].splitlines()) > 10
    # the same with the host fetch and another cut
    _, text = _run(case, "allh", dmr_perm=N_PERM, host_fetch=True, chunk_size=33_333)
    assert text == exp


def test_max_p_and_min_sites_choose_what_is_tested(case):
    from pomfret_amd.pipeline import hapmeth_files
    exp, assign, _ = _expected(case, max_p=1e-4)
    assert exp != _expected(case)[0] and len([x for x in exp.splitlines()[1:] if x.split("\t")[19] != "."]) >= 5
    res, text = _run(case, "p", dmr_perm=N_PERM, dmr_max_p=1e-4, assign=RULE)
    assert text == exp and open(res["assign_path"]).read() == assign
    # min_sites above every region: nothing is tested, every line stays
    res = hapmeth_files(case["bam"], str(case["tmp"] / "ms"), region=case["region"], regions=case["bed"], dmr_perm=N_PERM,
                        dmr=DmrConfig(min_cov=5, min_delta_pct=40, max_gap=1000, min_sites=100_000))
    assert open(res["regions_path"]).read() == regions_text(case["rec"], perm=[None] * len(case["rec"]), n_perm=N_PERM)
    assert res["n_tested"] == 0 and res["n_untested"] == len(case["rec"])


def test_phase_blocks_split_a_region(case):
    """--dmr-blocks: a block ends inside one of the model's regions; it, and
    every given region around that point, is split and untested."""
    r = case["model"]["kept"][10]
    cut = r["start"] + 1                          # 1-based end of the first block: a break right of the first member
    blocks = [(case["lo"] + 1, cut), (cut + 1, case["hi"])]
    gtf = str(case["tmp"] / "blocks.gtf")
    with open(gtf, "w") as f:
        for bs, be in blocks:
            f.write(f'chrS\tPhasing\texon\t{bs}\t{be}\t.\t+\t.\tgene_id "{bs}"; transcript_id "{bs}.1";\n')
    breaks = sorted(x for bs, be in blocks for x in (bs - 1, be))
    exp, assign, tagcheck = _expected(case, breaks=breaks)
    rows = {x.split("\t")[3]: x.rstrip("\n").split("\t") for x in exp.splitlines()[1:]}
    assert rows["hmm10"][16:] == ["split", ".", ".", ".", "."] and rows["hmm9"][16] == "ok" and rows["long"][16] == "split"
    n_split = len([x for x in exp.splitlines()[1:] if x.split("\t")[16] == "split"])
    assert n_split >= 3                           # the region, the pair that starts with it, the long one
    res, text = _run(case, "b", dmr_perm=N_PERM, tag_check=True, dmr_blocks=gtf, chunk_size=33_333)
    assert text == exp and res["n_regions_split"] == n_split
    assert (open(res["tagcheck_path"]).read(), open(res["tagcheck_regions_path"]).read()) == tagcheck


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    exp, assign, tagcheck = _expected(case)
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--regions", case["bed"], "--dmr-min-cov", "5",
                        "--dmr-delta", "40", "--dmr-min-sites", "2", "--dmr-perm", str(N_PERM), "--assign", "--tag-check",
                        case["bam"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.bed").read() == case["text"] and open(out + ".hapmeth.regions.bed").read() == exp
    assert open(out + ".hapmeth.assign.tsv").read() == assign
    assert (open(out + ".hapmeth.tagcheck.tsv").read(), open(out + ".hapmeth.tagcheck.regions.tsv").read()) == tagcheck
    assert not os.path.exists(out + ".hapmeth.dmr.bed")
    assert "given regions: %d written (0 split by a phase block), 1 on contigs the BAM does not have, 1 outside" % \
        len(case["rec"]) in r.stderr
    assert "%d regions written to %s.hapmeth.regions.bed" % (len(case["rec"]), out) in r.stderr
    # without the permutation columns
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--regions", case["bed"], "--dmr-min-sites", "2",
                        case["bam"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.regions.bed").read() == case["plain"]


def test_a_bad_bed_fails_the_run_and_leaves_no_file(case):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import hapmeth_files
    bad = str(case["tmp"] / "bad.bed")
    with open(bad, "w") as f:
        f.write("chrS\t10\t20\nchrS\t30\t20\n")
    out = str(case["tmp"] / "bad")
    for bed in (bad, str(case["tmp"] / "absent.bed")):
        with pytest.raises(PomfretError):
            hapmeth_files(case["bam"], out, region=case["region"], regions=bed, dmr_perm=N_PERM, assign=RULE, tag_check=True)
        for ext in ("bed", "regions.bed", "assign.tsv", "tagcheck.tsv", "tagcheck.regions.tsv", "dmr.bed"):
            assert not os.path.exists(out + ".hapmeth." + ext)


def test_without_regions_the_dmr_files_as_before(case):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / "d"), region=case["region"], dmr=CFG, dmr_hmm=HMM)
    assert open(res["dmr_path"]).read() == _hmm_text(case["model"]["kept"]) and "regions_path" not in res
    assert open(res["path"]).read() == case["text"] and res["n_regions"] == len(case["model"]["kept"])
    assert not os.path.exists(str(case["tmp"] / "d") + ".hapmeth.regions.bed")
