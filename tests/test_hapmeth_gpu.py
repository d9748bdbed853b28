"""`hapmeth` end to end on the device: pf_hapmeth_main (hapmeth_files, the
CLI) over a haplotagged fixture BAM against the text built on the CPU from
the host fetch of one window spanning the reads, the oracle's loader, the
literal pileup reference and the Fisher test.  Every comparison is on bytes.
"""
import os
import subprocess

import numpy as np
import pytest

from pomfret_amd.abi import LoadConfig

from tests import _fixtures as fx
from tests.test_pileup_gpu import _pile_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "#chrom\tstart\tend\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tother_meth\tother_unmeth\tasm_p\n"
LCFG = LoadConfig(min_mapq=10, min_len=0, qual_lo=100, qual_hi=156)      # hapmeth's defaults


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd import fisher_exact
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    with BamFile(bam) as bf:
        one, _, _ = bf.fetch_windows("chrS", [lo], [hi], readback=0)
    assert one.n_recs > 100
    wb, _ = oracle_lib.load_reads(LCFG, one)
    assert len(set(wb.read_hp.tolist())) >= 3    # both haplotypes and untagged reads
    win_off, pos, cnt = _pile_ref(wb)
    lines = [HEADER]
    for p, c in zip(pos.tolist(), cnt.reshape(-1, 6).tolist()):
        two = fisher_exact(c[0], c[1], c[2], c[3])[3]
        lines.append("chrS\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (p, p + 1, *c, two))
    assert len(lines) > 1000
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", text="".join(lines), n_sites=len(pos))


def _run(case, name, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), **kw)
    assert res["path"] == str(case["tmp"] / name) + ".hapmeth.bed"
    return res, open(res["path"]).read()


def test_file_equals_cpu_text(case):
    res, text = _run(case, "a", region=case["region"])
    assert text == case["text"]
    assert res["n_sites"] == case["n_sites"] and res["n_records"] > 0 and res["ms_kernels"] > 0


def test_host_fetch_same_bytes(case):
    _, text = _run(case, "h", region=case["region"], host_fetch=True, threads=2)
    assert text == case["text"]


@pytest.mark.parametrize("chunk", [7_000, 33_333, 100_000])
def test_chunk_size_same_bytes(case, chunk):
    res, text = _run(case, f"c{chunk}", region=case["region"], chunk_size=chunk, job_windows=5)
    assert text == case["text"]
    assert res["n_windows"] >= 1


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], case["bam"]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.bed").read() == case["text"]
    assert "sites" in r.stderr and "pileup kernels" in r.stderr


def test_whole_bam_skips_empty_windows(case):
    res, text = _run(case, "w")
    assert res["n_skipped"] > 0 and res["n_windows"] == 2000          # 200 Mb of 100 kb windows
    assert text == case["text"]
