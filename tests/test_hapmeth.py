"""hapmeth's host side: the BED writer's bytes, the ctypes mirrors' layout and
the CLI's argument handling.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import _fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
HEADER = "#chrom\tstart\tend\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tother_meth\tother_unmeth\tasm_p\n"


def _pile():
    """Two windows; the second site has no haplotype-2 call, the third a
    clear allele-specific split."""
    return dict(win_off=np.array([0, 2, 3], np.uint64), pos=np.array([10, 99, 5000], np.uint32),
                cnt=np.array([[[3, 1], [2, 2], [0, 1]],
                              [[4, 0], [0, 0], [7, 7]],
                              [[12, 0], [0, 11], [1, 0]]], np.uint32))


def test_writer_bytes(tmp_path):
    from pomfret_amd import fisher_exact
    from pomfret_amd.pipeline import write_hapmeth
    p = str(tmp_path / "o.bed")
    write_hapmeth(p, "chr7", _pile(), header=True)
    p1 = "%.6g" % fisher_exact(3, 1, 2, 2)[3]
    p3 = "%.6g" % fisher_exact(12, 0, 0, 11)[3]
    assert p1 == "1" and p3 == "7.39602e-07"         # 1 / C(23, 12) = 1 / 1,352,078
    exp = (HEADER + f"chr7\t10\t11\t3\t1\t2\t2\t0\t1\t{p1}\n" + "chr7\t99\t100\t4\t0\t0\t0\t7\t7\t1\n"
           + f"chr7\t5000\t5001\t12\t0\t0\t11\t1\t0\t{p3}\n")
    assert open(p).read() == exp
    # header=False appends; a window range selects its sites
    write_hapmeth(p, "chrQ", _pile(), header=False, w0=1, w1=2)
    assert open(p).read() == exp + f"chrQ\t5000\t5001\t12\t0\t0\t11\t1\t0\t{p3}\n"
    write_hapmeth(p, "chr7", _pile(), header=True, w0=0, w1=0)
    assert open(p).read() == HEADER


def test_writer_refuses_bad_ranges(tmp_path):
    import pytest
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import write_hapmeth
    with pytest.raises(PomfretError):
        write_hapmeth(str(tmp_path / "x.bed"), "c", _pile(), w0=0, w1=3)
    with pytest.raises(PomfretError):
        write_hapmeth(str(tmp_path / "nodir" / "x.bed"), "c", _pile())


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import PfHapmethOpts, PfHapmethStats, PfPileup
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pf_pileup_t),'
                   'offsetof(pf_pileup_t, n_sites), offsetof(pf_pileup_t, win_off), offsetof(pf_pileup_t, pos),'
                   'offsetof(pf_pileup_t, cnt), offsetof(pf_pileup_t, ms_kernels), sizeof(pf_hapmeth_opts_t),'
                   'offsetof(pf_hapmeth_opts_t, load), offsetof(pf_hapmeth_opts_t, verbose),'
                   'sizeof(pf_hapmeth_stats_t), offsetof(pf_hapmeth_stats_t, ms_kernels));return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    exp = [C.sizeof(PfPileup), PfPileup.n_sites.offset, PfPileup.win_off.offset, PfPileup.pos.offset,
           PfPileup.cnt.offset, PfPileup.ms_kernels.offset, C.sizeof(PfHapmethOpts), PfHapmethOpts.load.offset,
           PfHapmethOpts.verbose.offset, C.sizeof(PfHapmethStats), PfHapmethStats.ms_kernels.offset]
    assert got == exp


def test_cli_argument_errors(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-o", str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::" in r.stderr and "missing bam" in r.stderr
    r = subprocess.run([EXE, "hapmeth", "-o", str(tmp_path / "o"), str(tmp_path / "absent.bam")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "[E::" in r.stderr and "absent.bam" in r.stderr
    assert not os.path.exists(str(tmp_path / "o") + ".hapmeth.bed")
    r = subprocess.run([EXE, "frobnicate"], capture_output=True, text=True)
    assert r.returncode == 1 and "unknown subcommand" in r.stderr
    r = subprocess.run([EXE, "help"], capture_output=True, text=True)
    assert "hapmeth" in r.stderr
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1 and "--chunk-size" in r.stderr and "de tag" in r.stderr


def test_cli_fails_loudly_without_a_device(tmp_path):
    aln, recs, bam, vcf = fx.tagged(tmp_path, n_windows=1, len_scale=0.3)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, bam], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 1 and "[E::" in r.stderr and "failed" in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "-r", "chrNope:1-10", bam], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 1 and "bad region" in r.stderr
