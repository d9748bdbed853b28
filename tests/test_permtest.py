"""hapmeth --dmr-perm's host side: the new structs' layout, the writer's bytes
(pf_write_dmr_perm) and its argument checks, the entry point's and the CLI's
option checks, and the reference's own known answers.  No GPU."""
import ctypes as C
import os
import subprocess

import pytest

from tests._perm_ref import perm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
HEADER = "#chrom\tstart\tend\tn_sites\tdir\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta\tpooled_p\n"
PHEADER = HEADER[:-1] + "\treads_h1\treads_h2\tperm_p\n"

FLAT = ([3] * 7, [2] * 7)
# (m, u, tags, ws, we, n_perm, seed) -> (hits, status): the issue's table
KNOWN = {
    "split": (([30] * 20 + [0] * 20, [0] * 20 + [30] * 20, [0] * 20 + [1] * 20, 5, 900, 999, 1), (0, 0)),
    "flat": ((*FLAT, [0, 0, 0, 1, 1, 1, 1], 5, 900, 50, 1), (50, 0)),
    "one-sided": ((*FLAT, [0] * 7, 5, 900, 50, 1), (0, 1)),
    "1v1": (([4, 0], [0, 4], [0, 1], 0, 1, 64, 3), (64, 0)),
    "2v1": (([4, 0, 0], [0, 4, 4], [0, 1, 1], 0, 1, 300, 3), (105, 0)),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_reference_known_answers(name):
    (m, u, tags, ws, we, n_perm, seed), exp = KNOWN[name]
    assert perm_ref(ws, we, m, u, tags, n_perm, seed) == exp


def _regions():
    return dict(start=[100, 5000, 7000], end=[161, 5040, 7010], n_sites=[6, 5, 9], sign=[1, -1, 1],
                sum=[[12, 0, 0, 11], [0, 5, 5, 0], [30, 2, 3, 40]], open=[0, 0, 0])


def _perm():
    return dict(n_reads=[[4, 5], [7, 0], [4097, 12]], hits=[0, 0, 0], status=[0, 1, 2], n_perm=99, seed=1)


def test_writer_bytes(tmp_path):
    from pomfret_amd import fisher_exact
    from pomfret_amd.pipeline import write_dmr_perm
    p = str(tmp_path / "o.dmr.bed")
    write_dmr_perm(p, "chr7", _regions(), _perm())
    p3 = "%.6g" % fisher_exact(30, 2, 3, 40)[3]
    exp = [PHEADER, "chr7\t100\t161\t6\th1>h2\t12\t0\t0\t11\t1.0000\t7.39602e-07\t4\t5\t0.01\n",
           "chr7\t5000\t5040\t5\th1<h2\t0\t5\t5\t0\t-1.0000\t0.00793651\t7\t0\t.\n",
           f"chr7\t7000\t7010\t9\th1>h2\t30\t2\t3\t40\t0.8677\t{p3}\t4097\t12\t.\n"]
    assert open(p).read() == "".join(exp)
    # (hits + 1) / (n_perm + 1) as %.6g; max_p drops the second line and keeps each region's own window
    perm = dict(n_reads=[[4, 5], [7, 1], [40, 12]], hits=[32, 5, 998], status=[0, 0, 0], n_perm=999, seed=7)
    write_dmr_perm(p, "chrQ", _regions(), perm, max_p=1e-3, header=False)
    tail = [exp[1].replace("chr7", "chrQ").replace("\t0.01\n", "\t%.6g\n" % (33 / 1000)),
            exp[3].replace("chr7", "chrQ").replace("\t4097\t12\t.\n", "\t40\t12\t%.6g\n" % (999 / 1000))]
    assert tail[0].endswith("\t4\t5\t0.033\n") and tail[1].endswith("\t40\t12\t0.999\n")
    assert open(p).read() == "".join(exp) + "".join(tail)
    # no region: the header alone, with the three names
    write_dmr_perm(p, "chr7", dict(start=[], end=[], n_sites=[], sign=[], sum=[], open=[]),
                   dict(n_reads=[], hits=[], status=[], n_perm=99))
    assert open(p).read() == PHEADER


def test_first_eleven_columns_are_write_dmr(tmp_path):
    from pomfret_amd.pipeline import write_dmr, write_dmr_perm
    a, b = str(tmp_path / "a.bed"), str(tmp_path / "b.bed")
    for max_p in (1.0, 1e-3):
        write_dmr(a, "chr7", _regions(), max_p=max_p)
        write_dmr_perm(b, "chr7", _regions(), _perm(), max_p=max_p)
        la, lb = open(a).read().splitlines(), open(b).read().splitlines()
        assert len(la) == len(lb) > 1
        for x, y in zip(la, lb):
            cols = y.split("\t")
            assert len(cols) == 14 and "\t".join(cols[:11]) == x


def test_writer_argument_errors(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import write_dmr_perm
    p = str(tmp_path / "o.dmr.bed")
    write_dmr_perm(p, "c", _regions(), _perm())
    before = open(p).read()
    with pytest.raises(PomfretError, match=r"\(-1\)"):                     # no perm
        write_dmr_perm(p, "c", _regions(), None, header=False)
    short = dict(n_reads=[[4, 5], [7, 0]], hits=[0, 0], status=[0, 1], n_perm=99)
    with pytest.raises(PomfretError, match=r"\(-1\)"):                     # fewer windows than runs
        write_dmr_perm(p, "c", _regions(), short, header=False)
    big = _regions()
    big["sum"][2] = [2 ** 31, 2, 3, 40]
    with pytest.raises(PomfretError, match="limit"):
        write_dmr_perm(p, "c", big, _perm(), header=False)
    assert open(p).read() == before                                        # nothing written
    with pytest.raises(PomfretError):
        write_dmr_perm(str(tmp_path / "nodir" / "x.bed"), "c", _regions(), _perm())


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import PfHapmethDmrStats, PfHapmethOpts, PfHapmethPerm, PfHapmethPermStats, PfHapmethStats, PfPerm
    src = tmp_path / "l.c"
    names = ["sizeof(pf_perm_t)", "offsetof(pf_perm_t, n_perm)", "offsetof(pf_perm_t, seed)",
             "offsetof(pf_perm_t, n_reads)", "offsetof(pf_perm_t, sum)", "offsetof(pf_perm_t, hits)",
             "offsetof(pf_perm_t, status)", "offsetof(pf_perm_t, ms_kernels)", "sizeof(pf_hapmeth_perm_t)",
             "offsetof(pf_hapmeth_perm_t, seed)", "sizeof(pf_hapmeth_perm_stats_t)",
             "offsetof(pf_hapmeth_perm_stats_t, n_untested)", "offsetof(pf_hapmeth_perm_stats_t, n_records)",
             "offsetof(pf_hapmeth_perm_stats_t, ms_kernels)", "sizeof(pf_hapmeth_opts_t)", "sizeof(pf_hapmeth_stats_t)",
             "sizeof(pf_hapmeth_dmr_stats_t)", "PF_PERM_MAX_READS", "PF_PERM_MAX_PERM"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    exp = [C.sizeof(PfPerm), PfPerm.n_perm.offset, PfPerm.seed.offset, PfPerm.n_reads.offset, PfPerm.sum.offset,
           PfPerm.hits.offset, PfPerm.status.offset, PfPerm.ms_kernels.offset, C.sizeof(PfHapmethPerm),
           PfHapmethPerm.seed.offset, C.sizeof(PfHapmethPermStats), PfHapmethPermStats.n_untested.offset,
           PfHapmethPermStats.n_records.offset, PfHapmethPermStats.ms_kernels.offset, C.sizeof(PfHapmethOpts),
           C.sizeof(PfHapmethStats), C.sizeof(PfHapmethDmrStats), 4096, 1_000_000]
    assert got == exp
    assert C.sizeof(PfHapmethOpts) == 64 and C.sizeof(PfHapmethStats) == 40   # grown by nothing


def test_perm_needs_dmr(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import DmrConfig, LoadConfig, PfHapmethDmr, PfHapmethOpts, PfHapmethPerm
    from pomfret_amd.pipeline import _bind, hapmeth_files
    out = str(tmp_path / "o")
    with pytest.raises(PomfretError):
        hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=None, dmr_perm=9)
    # the entry point itself: perm without dmr, and n_perm 0 / past the limit with dmr, before the BAM is opened
    L = _bind()
    o = PfHapmethOpts(b"absent.bam", out.encode(), None, 0, 0, LoadConfig(min_len=0).to_c(), 1, 0, 0, 0)
    d = PfHapmethDmr(DmrConfig().to_c(), 1.0, None)
    assert L.pf_hapmeth_run_perm(C.byref(o), None, C.byref(PfHapmethPerm(9, 1)), None, None, None) == -1
    assert L.pf_hapmeth_run_perm(C.byref(o), C.byref(d), C.byref(PfHapmethPerm(0, 1)), None, None, None) == -1
    assert L.pf_hapmeth_run_perm(C.byref(o), C.byref(d), C.byref(PfHapmethPerm(1_000_001, 1)), None, None, None) == -1
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")


@pytest.mark.parametrize("args,word", [
    (["--dmr-perm", "99"], "need --dmr"), (["--dmr-seed", "4"], "need --dmr"),
    (["--dmr", "--dmr-perm", "-1"], "--dmr-perm"), (["--dmr", "--dmr-perm", "1000001"], "--dmr-perm"),
    (["--dmr", "--dmr-perm", "9x"], "--dmr-perm"), (["--dmr", "--dmr-perm", "9", "--dmr-seed", "-2"], "--dmr-seed"),
    (["--dmr", "--dmr-perm", "9", "--dmr-seed", "4294967296"], "--dmr-seed")])
def test_cli_option_errors(tmp_path, args, word):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")


def test_cli_help_and_valid_line(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1 and "--dmr-perm" in r.stderr and "--dmr-seed" in r.stderr and "perm_p" in r.stderr
    # a valid line gets as far as the BAM, and leaves neither file behind
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--dmr", "--dmr-perm", "999", "--dmr-seed", "5",
                        str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")
