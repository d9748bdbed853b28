"""hapmeth --tag-check's host side: the four leave-one-out weights of a site
(pf_tagcheck_site_weights, the function the kernel runs) against the per-entry
definition of tests/_tagcheck_ref.py, the two writers' bytes, the structs'
layout, the option checks, and a simulation that documents why the check leaves
the read's own entry out.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests._tagcheck_ref import (HEADER, REGIONS_HEADER, entry_weight, region_lines, tagcheck_lines, tagcheck_ref_batch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
SUFFIXES = (".hapmeth.bed", ".hapmeth.dmr.bed", ".hapmeth.assign.tsv", ".hapmeth.tagcheck.tsv", ".hapmeth.tagcheck.regions.tsv")


def _lib_weights(cnt, min_cov):
    from pomfret_amd import lib
    w, u = (C.c_int32 * 4)(), (C.c_uint8 * 2)()
    lib().pf_tagcheck_site_weights(*cnt, min_cov, w, u)
    return list(w), list(u)


def _check_site(cnt, min_cov):
    """Every (tag, category) an entry can have at this site: the table's weight
    and flag are the definition's; where no such entry exists the weight is 0."""
    w, u = _lib_weights(cnt, min_cov)
    for h in (0, 1):
        n_h = cnt[2 * h] + cnt[2 * h + 1]
        for c in (0, 1):
            if cnt[2 * h + c] == 0:
                assert w[2 * h + c] == 0, (cnt, min_cov, h, c)
                continue
            ref = entry_weight(cnt, h, c, min_cov)
            assert bool(u[h]) == (ref is not None), (cnt, min_cov, h, c)
            assert w[2 * h + c] == (ref or 0), (cnt, min_cov, h, c)
        if n_h == 0:
            assert not u[h]


def test_table_equals_definition_small_counts():
    for cnt in itertools.product(range(7), repeat=4):
        for min_cov in (0, 1, 3):
            _check_site(list(cnt), min_cov)


def test_table_equals_definition_random_counts():
    rng = np.random.default_rng(2)
    cases = rng.integers(0, 65536, (300, 4)).tolist() + rng.integers(0, 40, (300, 4)).tolist()
    cases += [[65535] * 4, [0, 65535, 65535, 0], [1, 0, 0, 1], [65535, 0, 1, 0]]
    for cnt in cases:
        for min_cov in (1, 5, 30):
            _check_site(cnt, min_cov)
    assert max(abs(x) for cnt in cases for x in _lib_weights(cnt, 1)[0]) < 1 << 22


def test_hand_checked_site():
    """m1=5, u1=0, m2=0, u2=5, a meth entry of tag 0 taken out: L(5) - L(6) - L(1) + L(7);
    with min_cov 5 that entry is not usable (4 left), with 4 it is."""
    from tests._assign_ref import ilog2_q16 as L
    w, u = _lib_weights([5, 0, 0, 5], 4)
    assert u == [1, 1] and w == [L(5) - L(6) + L(7), 0, 0, -(L(5) - L(6) + L(7))]
    assert _lib_weights([5, 0, 0, 5], 5) == ([0, 0, 0, 0], [0, 0])
    assert _lib_weights([6, 0, 0, 5], 5)[1] == [1, 0]       # the boundary on one haplotype only
    # a count of exactly 1: L(1) = 0
    assert _lib_weights([1, 3, 2, 2], 1)[0][0] == L(1) - L(5) - L(3) + L(6) == entry_weight([1, 3, 2, 2], 0, 0, 1)


def _result():
    """Two windows, seven reads: an untagged read, a tagged one without a usable call, and every kind of line."""
    return dict(win_read_off=[0, 4, 7], n_used=[0, 3, 0, 1, 12, 2, 5], llr=[0, 3 * 65536 + 32768, 0, -1, -(7 << 16) - 6554, 0, 1 << 18],
                verdict=[255, 0, 255, 2, 0, 2, 1], hp=[254, 0, 1, 0, 1, 0, 1],
                win_n=[[[2, 2, 1, 0], [1, 0, 0, 0]], [[1, 1, 0, 0], [2, 2, 1, 1]]])


def test_writer_bytes(tmp_path):
    from pomfret_amd.pipeline import write_tagcheck
    p, pr = str(tmp_path / "o.tagcheck.tsv"), str(tmp_path / "o.tagcheck.regions.tsv")
    names = ["u0", "readA", "idle", "readB/1", "r-neg", "zero", "sw"]
    n = write_tagcheck(p, pr, "chr7", _result(), [100, 5000], [161, 5040], names)
    exp = [HEADER, "readA\tchr7\t100\t161\t1\t3\t3.5000\tok\n", "readB/1\tchr7\t100\t161\t1\t1\t-0.0000\t.\n",
           "r-neg\tchr7\t5000\t5040\t2\t12\t-7.1000\tok\n", "zero\tchr7\t5000\t5040\t1\t2\t0.0000\t.\n",
           "sw\tchr7\t5000\t5040\t2\t5\t4.0000\tflip\n"]
    expr = [REGIONS_HEADER, "chr7\t100\t161\t2\t2\t1\t0\t1\t0\t0\t0\n", "chr7\t5000\t5040\t1\t1\t0\t0\t2\t2\t1\t1\n"]
    assert n == (5, 2) and open(p).read() == "".join(exp) and open(pr).read() == "".join(expr)
    # the reference's text functions say the same
    q = dict(enumerate(names))
    assert tagcheck_lines(_result(), "chr7", [100, 5000], [161, 5040], q) == exp[1:]
    assert region_lines(_result(), "chr7", [100, 5000], [161, 5040]) == expr[1:]
    # appended, with the reads' records permuted: the qname is the record's
    n = write_tagcheck(p, pr, "chrQ", _result(), [100, 5000], [161, 5040], names[::-1], rec_of_read=[6, 5, 4, 3, 2, 1, 0], header=False)
    assert n == (5, 2) and open(p).read() == "".join(exp) + "".join(x.replace("chr7", "chrQ") for x in exp[1:])
    assert open(pr).read() == "".join(expr) + "".join(x.replace("chr7", "chrQ") for x in expr[1:])
    # an empty result and no result: the headers alone
    empty = dict(win_read_off=[0], n_used=[], llr=[], verdict=[], hp=[], win_n=[])
    assert write_tagcheck(p, pr, "chr7", empty, [], [], []) == (0, 0) and open(p).read() == HEADER
    assert open(pr).read() == REGIONS_HEADER
    os.remove(p), os.remove(pr)
    assert write_tagcheck(p, pr, "chr7", None, [], [], []) == (0, 0) and open(p).read() == HEADER
    assert open(pr).read() == REGIONS_HEADER


def test_writer_argument_errors(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import write_tagcheck
    p = str(tmp_path / "o.tagcheck.tsv")
    names = list("abcdefg")
    write_tagcheck(p, None, "c", _result(), [1, 2], [3, 4], names)
    before = open(p).read()
    bad = _result()
    bad["win_read_off"] = [0, 4, 8]                      # past the reads
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        write_tagcheck(p, None, "c", bad, [1, 2], [3, 4], names + ["h"], header=False)
    bad["win_read_off"] = [0, 5, 4]                      # descending
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        write_tagcheck(p, None, "c", bad, [1, 2], [3, 4], names, header=False)
    assert open(p).read() == before                      # nothing written
    with pytest.raises(PomfretError):
        write_tagcheck(str(tmp_path / "nodir" / "x.tsv"), None, "c", _result(), [1, 2], [3, 4], names)


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import (PfAssign, PfHapmethAssign, PfHapmethAssignStats, PfHapmethOpts, PfHapmethTagcheck,
                                 PfHapmethTagcheckStats, PfTagcheck)
    T, S = PfTagcheck, PfHapmethTagcheckStats
    names = ["sizeof(pf_tagcheck_t)"] + ["offsetof(pf_tagcheck_t, %s)" % f for f, _ in T._fields_]
    names += ["sizeof(pf_hapmeth_tagcheck_t)", "sizeof(pf_hapmeth_tagcheck_stats_t)"]
    names += ["offsetof(pf_hapmeth_tagcheck_stats_t, %s)" % f for f, _ in S._fields_]
    # no existing struct grew
    names += ["sizeof(pf_assign_t)", "sizeof(pf_hapmeth_assign_t)", "sizeof(pf_hapmeth_assign_stats_t)", "sizeof(pf_hapmeth_opts_t)"]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    exp = [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_] + [C.sizeof(PfHapmethTagcheck), C.sizeof(S)]
    exp += [getattr(S, f).offset for f, _ in S._fields_]
    exp += [C.sizeof(PfAssign), C.sizeof(PfHapmethAssign), C.sizeof(PfHapmethAssignStats), C.sizeof(PfHapmethOpts)]
    assert got == exp
    assert got[-4:] == [56, 16, 40, 64]


def test_tag_check_needs_dmr(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import LoadConfig, PfHapmethOpts, PfHapmethTagcheck
    from pomfret_amd.pipeline import _bind, hapmeth_files
    out = str(tmp_path / "o")
    with pytest.raises(PomfretError):
        hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=None, tag_check=True)
    L = _bind()
    o = PfHapmethOpts(b"absent.bam", out.encode(), None, 0, 0, LoadConfig(min_len=0).to_c(), 1, 0, 0, 0)
    assert L.pf_hapmeth_run_tagcheck(C.byref(o), None, None, None, C.byref(PfHapmethTagcheck(0, 0)), None, None, None, None,
                                     None) == -1
    for suffix in SUFFIXES:
        assert not os.path.exists(out + suffix)


@pytest.mark.parametrize("args,word", [
    (["--tag-check"], "--tag-check needs --dmr"),
    (["--tag-check", "--assign-min-llr", "2"], "--tag-check needs --dmr"),
    (["--dmr", "--assign-min-llr", "2"], "need --assign"),          # alone it is still refused
    (["--dmr", "--assign-min-calls", "3"], "need --assign"),
    (["--dmr", "--tag-check", "--assign-min-llr", "0"], "--assign-min-llr"),
    (["--dmr", "--tag-check", "--assign-min-calls", "65536"], "--assign-min-calls")])
def test_cli_option_errors(tmp_path, args, word):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    for suffix in SUFFIXES:
        assert not os.path.exists(out + suffix)


def test_cli_help_and_valid_line(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1
    for word in ("--tag-check", "leave-one-out", ".hapmeth.tagcheck.tsv", ".hapmeth.tagcheck.regions.tsv", "ok / (ok + flip)"):
        assert word in r.stderr, word
    # the two thresholds are accepted with --tag-check alone: the line gets as far as the BAM and leaves no file
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--dmr", "--tag-check", "--assign-min-llr", "2", "--assign-min-calls", "1",
                        str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
    for suffix in SUFFIXES:
        assert not os.path.exists(out + suffix)


def _simulate(p1, p2, seed, regions=40, sites=30, depth=15):
    from tests.test_pileup_gpu import _calls_batch
    rng = np.random.default_rng(seed)
    wins = []
    for k in range(regions):
        pos = [1000 * k + 10 * i for i in range(sites)]
        reads = [(h, [(p, int(rng.random() >= (p1, p2)[h])) for p in pos]) for h in (0, 1) for _ in range(depth)]
        wins.append((1000 * k, 1000 * k + 10 * sites, reads))
    return _calls_batch(wins)


def test_why_leave_one_out():
    """Documentation of the definition, printed (pytest -s), no threshold on the figures: 40
    regions of 30 sites, 15 + 15 reads, 3 bits / 2 calls, min_cov 3.  With both
    haplotypes methylated at 0.5 there is nothing to tell them apart, yet
    scoring a read against the model it helped to build calls a large share
    "concordant"; leave-one-out does not.  At 0.9 / 0.1 the two agree."""
    out = {}
    for name, (p1, p2) in (("null 0.5/0.5", (0.5, 0.5)), ("alternative 0.9/0.1", (0.9, 0.1))):
        b = _simulate(p1, p2, 11)
        for how, naive in (("self-scoring", True), ("leave-one-out", False)):
            ref = tagcheck_ref_batch(b, 3, 2, 3 << 16, self_scoring=naive)
            v = ref["verdict"]
            out[(name, how)] = (int((v == 0).sum()), int((v == 1).sum()), int((v == 2).sum()))
            print("[tag-check simulation] %s, %s: concordant %d, discordant %d, undecided %d" % ((name, how) + out[(name, how)]))
    assert all(sum(x) == 40 * 30 for x in out.values())     # every read has usable entries under both scorings
