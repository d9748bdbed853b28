"""hapmeth --assign's host side: the Q16 log2 (pf_ilog2_q16) and the site
weights against the literal reference tests/_assign_ref.py, the writer's bytes
(pf_write_assign), the new structs' layout, and the entry point's and the CLI's
option checks.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests._assign_ref import HEADER, assign_ref_batch, ilog2_q16, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
TOP = 131_072                                    # the largest argument: n + 2 with both counts at 65,535
KNOWN = {1: 0, 2: 65536, 3: 103872, 7: 183982, 65537: 1048577}


def test_log2_known_values():
    from pomfret_amd import lib
    for x, v in KNOWN.items():
        assert lib().pf_ilog2_q16(x) == v and ilog2_q16(x) == v, x


def test_log2_monotone_and_tight():
    """Monotone, never above floor(65536 * log2 x) and at most 1 below it, the
    library's and the reference's value the same: x = 1 .. 131,072."""
    from pomfret_amd import lib
    f = lib().pf_ilog2_q16
    got = np.array([f(x) for x in range(1, TOP + 1)], np.int64)
    x = np.arange(1, TOP + 1)
    exact = np.array([math.floor(65536 * math.log2(int(v))) for v in x], np.int64)
    # the floor of a double: math.log2 is exact at powers of two, and elsewhere 65536 * log2 x is irrational
    assert (np.diff(got) >= 0).all()
    assert (got <= exact).all() and (got >= exact - 1).all()
    for v in list(range(1, 5000)) + [65535, 65536, 65537, 100_000, TOP - 1, TOP]:
        assert ilog2_q16(v) == int(got[v - 1]), v


def _lib_weights(m1, u1, m2, u2):
    from pomfret_amd import lib
    w = (C.c_int32 * 2)()
    lib().pf_assign_site_weights(m1, u1, m2, u2, w)
    return w[0], w[1]


def test_hand_checked_site():
    """m1=5, u1=0, m2=0, u2=5: L(6) - L(7) - L(1) + L(7) = L(6)."""
    assert ilog2_q16(6) == 169408
    assert weights(5, 0, 0, 5) == (169408, -169408) and _lib_weights(5, 0, 0, 5) == (169408, -169408)
    rng = np.random.default_rng(1)
    for c in rng.integers(0, 65536, (200, 4)).tolist() + [[65535] * 4, [0, 65535, 65535, 0], [0, 0, 0, 0]]:
        assert _lib_weights(*c) == weights(*c), c


def _one_window(sites, cand_calls):
    """A window [100, 200): tagged reads that give each position of `sites` its
    (m1, u1, m2, u2), and one untagged read with cand_calls."""
    from tests.test_pileup_gpu import _calls_batch
    reads = []
    for h in (0, 1):
        depth = max(c[2 * h] + c[2 * h + 1] for c in sites.values())
        for k in range(depth):
            calls = []
            for p, c in sites.items():
                m, u = c[2 * h], c[2 * h + 1]
                if k < m + u:
                    calls.append((p, 0 if k < m else 1))
            reads.append((h, calls))
    reads.append((254, cand_calls))
    return _calls_batch([(100, 200, reads)])


def test_reference_hand_checked_and_symmetric_sites():
    """The reference itself: the hand-checked site scores +-L(6); a symmetric
    site (3, 3, 3, 3) adds 0 to S but 1 to n_used."""
    sites = {110: (5, 0, 0, 5), 120: (3, 3, 3, 3)}
    assert weights(3, 3, 3, 3) == (0, 0)
    for calls, S, n, tag in [([(110, 0)], 169408, 1, 0), ([(110, 1)], -169408, 1, 1), ([(120, 0)], 0, 1, 254),
                             ([(110, 0), (120, 1)], 169408, 2, 0), ([(110, 2), (120, 1), (130, 0)], 0, 1, 254)]:
        ref = assign_ref_batch(_one_window(sites, calls), 3, 1, 65536)
        assert (int(ref["llr"][-1]), int(ref["n_used"][-1]), int(ref["hp"][-1])) == (S, n, tag), calls
        assert ref["win_n"].tolist() == [[1, tag == 0, tag == 1]]
        assert ref["hp"][:-1].tolist() == [0] * 6 + [1] * 6 and not ref["n_used"][:-1].any()


def _result():
    """Two windows, six reads: a tagged read, a candidate without an informative call, and every kind of line."""
    return dict(win_read_off=[0, 4, 6], n_used=[0, 3, 0, 1, 12, 2], llr=[0, 3 * 65536 + 32768, 0, -1, -(7 << 16) - 6554, 0],
                hp=[1, 0, 254, 254, 1, 254], win_n=[[2, 1, 0], [2, 0, 1]])


def test_writer_bytes(tmp_path):
    from pomfret_amd.pipeline import write_assign
    p = str(tmp_path / "o.assign.tsv")
    names = ["t0", "readA", "idle", "readB/1", "r-neg", "zero"]
    n = write_assign(p, "chr7", _result(), [100, 5000], [161, 5040], names)
    exp = [HEADER, "readA\tchr7\t100\t161\t3\t3.5000\t1\n", "readB/1\tchr7\t100\t161\t1\t-0.0000\t.\n",
           "r-neg\tchr7\t5000\t5040\t12\t-7.1000\t2\n", "zero\tchr7\t5000\t5040\t2\t0.0000\t.\n"]
    assert n == 4 and open(p).read() == "".join(exp)
    # appended, with the reads' records permuted: the qname is the record's
    n = write_assign(p, "chrQ", _result(), [100, 5000], [161, 5040], names[::-1], rec_of_read=[5, 4, 3, 2, 1, 0], header=False)
    assert n == 4 and open(p).read() == "".join(exp) + "".join(x.replace("chr7", "chrQ") for x in exp[1:])
    # an empty result and no result: the header alone
    empty = dict(win_read_off=[0], n_used=[], llr=[], hp=[], win_n=[])
    assert write_assign(p, "chr7", empty, [], [], []) == 0 and open(p).read() == HEADER
    assert write_assign(p, "chr7", None, [], [], []) == 0 and open(p).read() == HEADER


def test_writer_argument_errors(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import write_assign
    p = str(tmp_path / "o.assign.tsv")
    names = ["a", "b", "c", "d", "e", "f"]
    write_assign(p, "c", _result(), [1, 2], [3, 4], names)
    before = open(p).read()
    bad = _result()
    bad["win_read_off"] = [0, 4, 7]                      # past the reads
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        write_assign(p, "c", bad, [1, 2], [3, 4], names + ["g"], header=False)
    bad["win_read_off"] = [0, 5, 4]                      # descending
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        write_assign(p, "c", bad, [1, 2], [3, 4], names, header=False)
    assert open(p).read() == before                      # nothing written
    with pytest.raises(PomfretError):
        write_assign(str(tmp_path / "nodir" / "x.tsv"), "c", _result(), [1, 2], [3, 4], names)


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import (PfAssign, PfAssignCfg, PfHapmethAssign, PfHapmethAssignStats, PfHapmethOpts,
                                 PfHapmethPermStats, PfHapmethStats)
    src = tmp_path / "l.c"
    names = ["sizeof(pf_assign_cfg_t)", "offsetof(pf_assign_cfg_t, min_calls)", "offsetof(pf_assign_cfg_t, min_llr_q16)",
             "sizeof(pf_assign_t)", "offsetof(pf_assign_t, n_reads)", "offsetof(pf_assign_t, win_read_off)",
             "offsetof(pf_assign_t, n_used)", "offsetof(pf_assign_t, llr)", "offsetof(pf_assign_t, hp)",
             "offsetof(pf_assign_t, win_n)", "offsetof(pf_assign_t, ms_kernels)", "sizeof(pf_hapmeth_assign_t)",
             "offsetof(pf_hapmeth_assign_t, min_calls)", "sizeof(pf_hapmeth_assign_stats_t)",
             "offsetof(pf_hapmeth_assign_stats_t, n_h1)", "offsetof(pf_hapmeth_assign_stats_t, n_h2)",
             "offsetof(pf_hapmeth_assign_stats_t, n_records)", "offsetof(pf_hapmeth_assign_stats_t, ms_kernels)",
             "sizeof(pf_hapmeth_opts_t)", "sizeof(pf_hapmeth_stats_t)", "sizeof(pf_hapmeth_perm_stats_t)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    exp = [C.sizeof(PfAssignCfg), PfAssignCfg.min_calls.offset, PfAssignCfg.min_llr_q16.offset, C.sizeof(PfAssign),
           PfAssign.n_reads.offset, PfAssign.win_read_off.offset, PfAssign.n_used.offset, PfAssign.llr.offset,
           PfAssign.hp.offset, PfAssign.win_n.offset, PfAssign.ms_kernels.offset, C.sizeof(PfHapmethAssign),
           PfHapmethAssign.min_calls.offset, C.sizeof(PfHapmethAssignStats), PfHapmethAssignStats.n_h1.offset,
           PfHapmethAssignStats.n_h2.offset, PfHapmethAssignStats.n_records.offset,
           PfHapmethAssignStats.ms_kernels.offset, C.sizeof(PfHapmethOpts), C.sizeof(PfHapmethStats),
           C.sizeof(PfHapmethPermStats)]
    assert got == exp
    assert C.sizeof(PfHapmethOpts) == 64 and C.sizeof(PfHapmethStats) == 40 and C.sizeof(PfHapmethPermStats) == 32


def test_assign_config_q16():
    from pomfret_amd.abi import AssignConfig
    assert AssignConfig().min_llr_q16 == 196608 and AssignConfig().min_calls == 2
    assert AssignConfig(min_llr=2.0).to_c().min_llr_q16 == 131072 and AssignConfig(min_llr=64).min_llr_q16 == 1 << 22


def test_assign_needs_dmr(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import AssignConfig, LoadConfig, PfHapmethAssign, PfHapmethOpts
    from pomfret_amd.pipeline import _bind, hapmeth_files
    out = str(tmp_path / "o")
    with pytest.raises(PomfretError):
        hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=None, assign=AssignConfig())
    # the entry point itself, before the BAM is opened
    L = _bind()
    o = PfHapmethOpts(b"absent.bam", out.encode(), None, 0, 0, LoadConfig(min_len=0).to_c(), 1, 0, 0, 0)
    assert L.pf_hapmeth_run_assign(C.byref(o), None, None, C.byref(PfHapmethAssign(196608, 2, 0)), None, None, None, None) == -1
    for suffix in (".hapmeth.bed", ".hapmeth.dmr.bed", ".hapmeth.assign.tsv"):
        assert not os.path.exists(out + suffix)


@pytest.mark.parametrize("args,word", [
    (["--assign"], "--assign needs --dmr"), (["--dmr", "--assign-min-llr", "2"], "need --assign"),
    (["--dmr", "--assign-min-calls", "3"], "need --assign"),
    (["--dmr", "--assign", "--assign-min-llr", "0"], "--assign-min-llr"),
    (["--dmr", "--assign", "--assign-min-llr", "65"], "--assign-min-llr"),
    (["--dmr", "--assign", "--assign-min-llr", "-1"], "--assign-min-llr"),
    (["--dmr", "--assign", "--assign-min-llr", "3x"], "--assign-min-llr"),
    (["--dmr", "--assign", "--assign-min-llr", "nan"], "--assign-min-llr"),
    (["--dmr", "--assign", "--assign-min-calls", "0"], "--assign-min-calls"),
    (["--dmr", "--assign", "--assign-min-calls", "65536"], "--assign-min-calls"),
    (["--dmr", "--assign", "--assign-min-calls", "2.5"], "--assign-min-calls")])
def test_cli_option_errors(tmp_path, args, word):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    for suffix in (".hapmeth.bed", ".hapmeth.dmr.bed", ".hapmeth.assign.tsv"):
        assert not os.path.exists(out + suffix)


def test_cli_help_and_valid_line(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1
    for word in ("--assign ", "--assign-min-llr", "--assign-min-calls", "odds of 8:1", ".hapmeth.assign.tsv"):
        assert word in r.stderr, word
    # a valid line (the bounds included) gets as far as the BAM, and leaves no file behind
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--dmr", "--assign", "--assign-min-llr", "64", "--assign-min-calls",
                        "65535", str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
    for suffix in (".hapmeth.bed", ".hapmeth.dmr.bed", ".hapmeth.assign.tsv"):
        assert not os.path.exists(out + suffix)
