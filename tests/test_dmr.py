"""hapmeth --dmr's host side: the stitching accumulator on hand-made parts,
the BED writer's bytes, the new structs' layout and the CLI's option checks.
No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pomfret_amd.abi import DmrConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
HEADER = "#chrom\tstart\tend\tn_sites\tdir\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta\tpooled_p\n"
LEFT, RIGHT = 1, 2
CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=100, min_sites=3)


def _part(runs, n_informative):
    """runs: (start, end, n_sites, sign, open); each member counts (10, 0, 0, 10) or its mirror."""
    return dict(start=[r[0] for r in runs], end=[r[1] for r in runs], n_sites=[r[2] for r in runs],
                sign=[r[3] for r in runs],
                sum=[[10 * r[2], 0, 0, 10 * r[2]] if r[3] > 0 else [0, 10 * r[2], 10 * r[2], 0] for r in runs],
                open=[r[4] for r in runs], n_informative=n_informative)


def _stitch(parts, cfg=CFG, breaks=None):
    from pomfret_amd.pipeline import dmr_stitch
    r = dmr_stitch(parts, cfg, breaks)
    assert not r["open"].any()
    return [tuple(int(x) for x in t) for t in zip(r["start"], r["end"], r["n_sites"], r["sign"])], r


def test_run_split_over_three_parts():
    parts = [_part([(10, 51, 2, 1, LEFT | RIGHT)], 2), _part([(100, 141, 2, 1, LEFT | RIGHT)], 2),
             _part([(200, 201, 1, 1, LEFT), (900, 950, 4, -1, RIGHT)], 6)]
    runs, r = _stitch(parts)
    assert runs == [(10, 201, 5, 1), (900, 950, 4, -1)]
    assert r["sum"].tolist() == [[50, 0, 0, 50], [0, 40, 40, 0]] and r["n_informative"] == 10
    # nothing to stitch; parts without a run
    assert _stitch([])[0] == [] and _stitch([_part([], 0), _part([], 3)])[0] == []


def test_empty_part_leaves_the_carry_open():
    a, b = _part([(10, 51, 2, 1, LEFT | RIGHT)], 2), _part([(120, 131, 2, 1, LEFT | RIGHT)], 2)
    assert _stitch([a, _part([], 0), _part([], 0), b])[0] == [(10, 131, 4, 1)]
    assert _stitch([_part([], 0), a, b, _part([], 0)])[0] == [(10, 131, 4, 1)]


def test_first_informative_site_outside_a_run_closes_the_carry():
    a = _part([(10, 51, 3, 1, LEFT | RIGHT)], 3)
    # the next part starts with a site of no direction: informative sites, no open-left run
    assert _stitch([a, _part([], 1)])[0] == [(10, 51, 3, 1)]
    assert _stitch([a, _part([(60, 71, 3, 1, RIGHT)], 4)])[0] == [(10, 51, 3, 1), (60, 71, 3, 1)]
    # the other direction closes it as well
    assert _stitch([a, _part([(60, 71, 3, -1, LEFT | RIGHT)], 3)])[0] == [(10, 51, 3, 1), (60, 71, 3, -1)]


def test_break_at_b_and_at_a():
    a, b = _part([(10, 51, 3, 1, LEFT | RIGHT)], 3), _part([(80, 91, 3, 1, LEFT | RIGHT)], 3)
    assert _stitch([a, b], breaks=[80])[0] == [(10, 51, 3, 1), (80, 91, 3, 1)]      # at b: a < x <= b
    assert _stitch([a, b], breaks=[51])[0] == [(10, 51, 3, 1), (80, 91, 3, 1)]
    assert _stitch([a, b], breaks=[50])[0] == [(10, 91, 6, 1)]                     # at a, the last member
    assert _stitch([a, b], breaks=[5, 10, 50, 81, 90, 4000])[0] == [(10, 91, 6, 1)]
    from pomfret_amd import PomfretError
    with pytest.raises(PomfretError):
        _stitch([a, b], breaks=[80, 50])


def test_gap_of_max_gap_and_one_more():
    a = _part([(10, 51, 3, 1, LEFT | RIGHT)], 3)                                   # last member at 50
    assert _stitch([a, _part([(150, 161, 3, 1, LEFT | RIGHT)], 3)])[0] == [(10, 161, 6, 1)]
    assert _stitch([a, _part([(151, 161, 3, 1, LEFT | RIGHT)], 3)])[0] == [(10, 51, 3, 1), (151, 161, 3, 1)]


def test_min_sites_only_at_close():
    one = [_part([(10 + 50 * k, 11 + 50 * k, 1, 1, LEFT | RIGHT)], 1) for k in range(3)]
    assert _stitch(one)[0] == [(10, 111, 3, 1)]                                    # 1 + 1 + 1 reaches min_sites
    assert _stitch(one[:2])[0] == []                                               # closed by the flush with 2
    # an open-left run below min_sites that joins nothing is dropped, one that joins is kept
    tail = _part([(300, 301, 1, 1, LEFT), (400, 431, 3, -1, 0), (500, 511, 2, 1, RIGHT)], 7)
    assert _stitch(one[:2] + [tail])[0] == [(400, 431, 3, -1)]
    assert _stitch(one[:2] + [_part([(160, 161, 1, 1, LEFT), (400, 431, 3, -1, RIGHT)], 5)])[0] == \
        [(10, 161, 3, 1), (400, 431, 3, -1)]


def test_parts_out_of_order_are_refused():
    from pomfret_amd import PomfretError
    a, b = _part([(10, 51, 3, 1, LEFT | RIGHT)], 3), _part([(40, 91, 3, 1, LEFT | RIGHT)], 3)
    with pytest.raises(PomfretError):
        _stitch([a, b])


def _regions():
    return dict(start=[100, 5000, 7000], end=[161, 5040, 7010], n_sites=[6, 5, 9], sign=[1, -1, 1],
                sum=[[12, 0, 0, 11], [0, 5, 5, 0], [30, 2, 3, 40]], open=[0, 0, 0])


def test_writer_bytes(tmp_path):
    from pomfret_amd import fisher_exact
    from pomfret_amd.pipeline import write_dmr
    p = str(tmp_path / "o.dmr.bed")
    write_dmr(p, "chr7", _regions())
    # 1 / C(23, 12); 2 / C(10, 5): the mirrored table is as likely; the third through the library
    p3 = "%.6g" % fisher_exact(30, 2, 3, 40)[3]
    exp = [HEADER, "chr7\t100\t161\t6\th1>h2\t12\t0\t0\t11\t1.0000\t7.39602e-07\n",
           "chr7\t5000\t5040\t5\th1<h2\t0\t5\t5\t0\t-1.0000\t0.00793651\n",
           f"chr7\t7000\t7010\t9\th1>h2\t30\t2\t3\t40\t0.8677\t{p3}\n"]                # 30/32 - 3/43 = 0.86773
    assert open(p).read() == "".join(exp)
    # max_p drops the second; header=False appends
    write_dmr(p, "chrQ", _regions(), max_p=1e-3, header=False)
    assert open(p).read() == "".join(exp) + (exp[1] + exp[3]).replace("chr7", "chrQ")
    write_dmr(p, "chr7", dict(start=[], end=[], n_sites=[], sign=[], sum=[], open=[]))
    assert open(p).read() == HEADER


def test_writer_refuses_a_pooled_sum_above_int32(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import write_dmr
    p = str(tmp_path / "o.dmr.bed")
    write_dmr(p, "c", _regions())
    before = open(p).read()
    big = _regions()
    big["sum"][2] = [2 ** 31, 2, 3, 40]
    with pytest.raises(PomfretError, match="limit"):
        write_dmr(p, "c", big, header=False)
    assert open(p).read() == before                                               # nothing written
    big["sum"][2] = [2 ** 31 - 1, 2, 3, 40]
    write_dmr(p, "c", big)
    assert "\t2147483647\t" in open(p).read()
    with pytest.raises(PomfretError):
        write_dmr(str(tmp_path / "nodir" / "x.bed"), "c", _regions())


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import (DMR_RUN_DTYPE, PfDmr, PfDmrCfg, PfDmrRun, PfHapmethDmr, PfHapmethDmrStats,
                                 PfHapmethOpts, PfHapmethStats)
    src = tmp_path / "l.c"
    names = ["sizeof(pf_dmr_cfg_t)", "offsetof(pf_dmr_cfg_t, min_sites)", "sizeof(pf_dmr_run_t)",
             "offsetof(pf_dmr_run_t, sign)", "offsetof(pf_dmr_run_t, sum)", "offsetof(pf_dmr_run_t, open)",
             "sizeof(pf_dmr_t)", "offsetof(pf_dmr_t, runs)", "offsetof(pf_dmr_t, n_informative)",
             "offsetof(pf_dmr_t, ms_kernels)", "offsetof(pf_dmr_t, ms_upload)", "sizeof(pf_hapmeth_dmr_t)",
             "offsetof(pf_hapmeth_dmr_t, max_p)", "offsetof(pf_hapmeth_dmr_t, blocks_path)",
             "sizeof(pf_hapmeth_dmr_stats_t)", "offsetof(pf_hapmeth_dmr_stats_t, ms_kernels)",
             "sizeof(pf_hapmeth_opts_t)", "sizeof(pf_hapmeth_stats_t)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    exp = [C.sizeof(PfDmrCfg), PfDmrCfg.min_sites.offset, C.sizeof(PfDmrRun), PfDmrRun.sign.offset, PfDmrRun.sum.offset,
           PfDmrRun.open.offset, C.sizeof(PfDmr), PfDmr.runs.offset, PfDmr.n_informative.offset, PfDmr.ms_kernels.offset,
           PfDmr.ms_upload.offset, C.sizeof(PfHapmethDmr), PfHapmethDmr.max_p.offset, PfHapmethDmr.blocks_path.offset,
           C.sizeof(PfHapmethDmrStats), PfHapmethDmrStats.ms_kernels.offset, C.sizeof(PfHapmethOpts),
           C.sizeof(PfHapmethStats)]
    assert got == exp
    assert DMR_RUN_DTYPE.itemsize == C.sizeof(PfDmrRun) == 56
    assert [DMR_RUN_DTYPE.fields[k][1] for k in ("sign", "sum", "open")] == \
        [PfDmrRun.sign.offset, PfDmrRun.sum.offset, PfDmrRun.open.offset]
    assert C.sizeof(PfHapmethOpts) == 64 and C.sizeof(PfHapmethStats) == 40       # as before --dmr


def test_defaults():
    c = DmrConfig()
    assert (c.min_cov, c.min_delta_pct, c.max_gap, c.min_sites) == (5, 40, 500, 5)


@pytest.mark.parametrize("args,word", [
    (["--dmr", "--dmr-min-cov", "0"], "--dmr-min-cov"), (["--dmr", "--dmr-min-cov", "7x"], "--dmr-min-cov"),
    (["--dmr", "--dmr-delta", "0"], "--dmr-delta"), (["--dmr", "--dmr-delta", "101"], "--dmr-delta"),
    (["--dmr", "--dmr-gap", "-3"], "--dmr-gap"), (["--dmr", "--dmr-min-sites", "0"], "--dmr-min-sites"),
    (["--dmr", "--dmr-max-p", "1.5"], "--dmr-max-p"), (["--dmr", "--dmr-max-p", "p"], "--dmr-max-p"),
    (["--dmr-gap", "100"], "need --dmr"), (["--dmr-blocks", "b.gtf"], "need --dmr")])
def test_cli_option_errors(tmp_path, args, word):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")


def test_cli_help_and_missing_value(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1
    for opt in ("--dmr ", "--dmr-min-cov", "--dmr-delta", "--dmr-gap", "--dmr-min-sites", "--dmr-max-p", "--dmr-blocks"):
        assert opt in r.stderr
    assert "ranking score, not a calibrated p-value" in r.stderr
    r = subprocess.run([EXE, "hapmeth", "-o", str(tmp_path / "o"), "x.bam", "--dmr", "--dmr-gap"], capture_output=True,
                       text=True)
    assert r.returncode == 1 and "[E::parse_cli_hapmeth]" in r.stderr
    # a valid --dmr line gets as far as the BAM, and leaves neither file behind
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--dmr", "--dmr-delta", "50", "--dmr-max-p", "0.01",
                        str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")
