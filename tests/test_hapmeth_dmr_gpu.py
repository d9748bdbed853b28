"""`hapmeth --dmr` end to end on the device: pf_hapmeth_run (hapmeth_files, the
CLI) over a haplotagged fixture BAM against the text built on the CPU from the
host fetch of one window spanning the reads, the oracle's loader, the literal
pileup reference, the literal region reference and the Fisher test.  Every
comparison is on bytes, and in every run the .hapmeth.bed is the text a run
without --dmr writes.

This fixture's haplotype-specific sites are scattered: at min_cov 3, delta 50,
gap 1000 a few hundred runs of both directions, none longer than 3.  Long runs
are tests/test_dmr_gpu.py's part.
"""
import os
import subprocess

import pytest

from pomfret_amd.abi import DmrConfig, LoadConfig

from tests import _fixtures as fx
from tests.test_dmr_gpu import _dmr_ref
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "#chrom\tstart\tend\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tother_meth\tother_unmeth\tasm_p\n"
DHEADER = "#chrom\tstart\tend\tn_sites\tdir\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta\tpooled_p\n"
LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)      # hapmeth's defaults


def _cfg(min_sites):
    return DmrConfig(min_cov=3, min_delta_pct=50, max_gap=1000, min_sites=min_sites)


def _dmr_text(pos, cnt, cfg, breaks=()):
    from pomfret_amd import fisher_exact
    lines = [DHEADER]
    for r in _dmr_ref(pos, cnt, cfg, breaks)["all"]:
        if r["n_sites"] < cfg.min_sites:
            continue
        m1, u1, m2, u2 = r["sum"]
        lines.append("chrS\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%.4f\t%.6g\n" % (
            r["start"], r["end"], r["n_sites"], "h1>h2" if r["sign"] > 0 else "h1<h2", m1, u1, m2, u2,
            m1 / (m1 + u1) - m2 / (m2 + u2), fisher_exact(m1, u1, m2, u2)[3]))
    return "".join(lines)


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_dmr")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
    wb, _ = oracle_lib.load_reads(LCFG, one)
    win_off, pos, cnt = _pile_ref(wb)
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, fisher_exact(c[0], c[1], c[2], c[3])[3]))
    dmr = {}
    for ms in (1, 2):
        dmr[ms] = _dmr_text(pos, cnt, _cfg(ms))
        body = dmr[ms].splitlines()[1:]
        assert len(body) >= 10 and any("h1>h2" in x for x in body) and any("h1<h2" in x for x in body)
    assert len(dmr[2]) < len(dmr[1])             # min_sites drops something
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", lo=lo, hi=hi, text="".join(lines), dmr=dmr,
                pos=pos, cnt=cnt)


def _run(case, name, min_sites=2, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], dmr=_cfg(min_sites), **kw)
    assert res["path"] == str(case["tmp"] / name) + ".hapmeth.bed"
    assert res["dmr_path"] == str(case["tmp"] / name) + ".hapmeth.dmr.bed"
    assert open(res["path"]).read() == case["text"]
    return res, open(res["dmr_path"]).read()


@pytest.mark.parametrize("min_sites", [1, 2])
def test_file_equals_cpu_text(case, min_sites):
    res, text = _run(case, f"a{min_sites}", min_sites)
    assert text == case["dmr"][min_sites]
    assert res["n_regions"] == len(text.splitlines()) - 1 and res["n_informative"] > 100 and res["dmr_ms_kernels"] > 0


def test_without_dmr_no_region_file(case):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / "plain"), region=case["region"])
    assert open(res["path"]).read() == case["text"] and "dmr_path" not in res
    assert not os.path.exists(str(case["tmp"] / "plain") + ".hapmeth.dmr.bed")


def test_host_fetch_same_bytes(case):
    _, text = _run(case, "h", host_fetch=True, threads=2)
    assert text == case["dmr"][2]


@pytest.mark.parametrize("chunk,min_sites", [(7_000, 1), (7_000, 2), (33_333, 2), (100_000, 2)])
def test_chunk_size_same_bytes(case, chunk, min_sites):
    res, text = _run(case, f"c{chunk}_{min_sites}", min_sites, chunk_size=chunk, job_windows=5)
    assert text == case["dmr"][min_sites]
    assert res["n_windows"] >= 1


def test_max_p_drops_lines(case):
    res, text = _run(case, "p", 1, dmr_max_p=0.01)
    full = case["dmr"][1].splitlines(keepends=True)
    exp = [full[0]] + [x for x in full[1:] if float(x.split("\t")[10]) <= 0.01]
    assert 1 < len(exp) < len(full) and text == "".join(exp) and res["n_regions"] == len(exp) - 1


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3",
                        "--dmr-delta", "50", "--dmr-gap", "1000", "--dmr-min-sites", "2", case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.bed").read() == case["text"]
    assert open(out + ".hapmeth.dmr.bed").read() == case["dmr"][2]
    assert "regions written" in r.stderr and "region kernels" in r.stderr


def test_phase_blocks_break_regions(case):
    """--dmr-blocks: a block boundary between the two members of a region."""
    two = [r for r in _dmr_ref(case["pos"], case["cnt"], _cfg(1))["all"] if r["n_sites"] == 2]
    cut = two[len(two) // 2]["start"] + 1        # 1-based end of the first block: the break right of the first member
    blocks = [(case["lo"] + 1, cut), (cut + 1, case["hi"])]
    gtf = str(case["tmp"] / "blocks.gtf")
    with open(gtf, "w") as f:
        for bs, be in blocks:
            f.write(f'chrS\tPhasing\texon\t{bs}\t{be}\t.\t+\t.\tgene_id "{bs}"; transcript_id "{bs}.1";\n')
        f.write(f'chrOther\tPhasing\texon\t1\t{cut - 5}\t.\t+\t.\tgene_id "1"; transcript_id "1.1";\n')
    breaks = sorted(x for bs, be in blocks for x in (bs - 1, be))
    for ms, kw in ((1, dict(chunk_size=7_000, job_windows=5)), (2, dict())):
        exp = _dmr_text(case["pos"], case["cnt"], _cfg(ms), breaks)
        assert exp != case["dmr"][ms]
        _, text = _run(case, f"b{ms}", ms, dmr_blocks=gtf, **kw)
        assert text == exp
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "clib")
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--dmr", "--dmr-min-cov", "3", "--dmr-delta", "50",
                        "--dmr-gap", "1000", "--dmr-min-sites", "1", "--dmr-blocks", gtf, case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.dmr.bed").read() == _dmr_text(case["pos"], case["cnt"], _cfg(1), breaks)
    # a block file that cannot be read fails the run and leaves no file
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import hapmeth_files
    with pytest.raises(PomfretError):
        hapmeth_files(case["bam"], str(case["tmp"] / "nb"), region=case["region"], dmr=_cfg(1),
                      dmr_blocks=str(case["tmp"] / "absent.gtf"))
    assert not os.path.exists(str(case["tmp"] / "nb") + ".hapmeth.bed")
    assert not os.path.exists(str(case["tmp"] / "nb") + ".hapmeth.dmr.bed")
