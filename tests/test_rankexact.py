"""The exact rank test without a device: the reference's two forms against
each other (tests/_rankexact_ref.py: brute is the definition, dp the counting
identity the kernel uses), known answers, scipy's exact Mann-Whitney p-values
on tie-free cases, pf_rank_exact_p, the writer's bytes (pf_write_rank_exact),
the new structs' layout and the entry points' argument checks."""
import ctypes as C
import os
import subprocess
from math import comb

import numpy as np
import pytest

from tests._rank_ref import rank_ref, rank_text
from tests._rankexact_ref import HEAD_EXTRA, brute, dp, rank_exact_text, rankexact_ref
from tests.test_ranktest import EXE, HEADER, KNOWN, ROOT, _recs


def _case(rng, n, top):
    """n counted reads with m, u below top (top 3: nearly everything ties), both haplotypes present."""
    m, u = rng.integers(0, top, n), rng.integers(0, top, n)
    m[(m + u) == 0] = 1
    tags = rng.integers(0, 2, n)
    tags[rng.integers(0, n)] = 0
    tags[(int(np.flatnonzero(tags == 0)[0]) + 1) % n] = 1
    return [(int(a), int(a + b)) for a, b in zip(m, u)], [int(t) for t in tags]


def test_dp_is_brute_force():
    """300 random windows of 2 .. 12 reads, m and u in 0 .. 2, 0 .. 4 or 0 .. 11:
    heavy ties, and equal fractions with different denominators (1/2 and 2/4)."""
    rng = np.random.default_rng(64)
    seen_equal_diff_den = 0
    for it in range(300):
        n = int(rng.integers(2, 13))
        f, tags = _case(rng, n, (3, 5, 12)[it % 3])
        b, d = brute(f, tags), dp(f, tags)
        assert b == d, (f, tags, b, d)
        u0, total, le, ge, two = d
        n1 = tags.count(0)
        assert total == comb(n, n1) and 1 <= two <= total and 1 <= le <= total and 1 <= ge <= total
        seen_equal_diff_den += any(a[1] != c[1] and a[0] * c[1] == c[0] * a[1] for a in f for c in f)
    assert seen_equal_diff_den > 100


def test_le_plus_ge_minus_equal_is_total():
    rng = np.random.default_rng(5)
    for it in range(60):
        f, tags = _case(rng, int(rng.integers(2, 11)), (3, 8)[it % 2])
        u0, total, le, ge, two = dp(f, tags)
        n1 = tags.count(0)
        # the subsets that hit u0 exactly, by the definition
        import itertools
        from tests._rankexact_ref import _u2
        eq = sum(_u2(f, [i in A for i in range(len(f))]) == u0 for A in itertools.combinations(range(len(f)), n1))
        assert le + ge - eq == total and eq >= 1


@pytest.mark.parametrize("k", [1, 5, 10, 32])
def test_separated_groups(k):
    """k + k reads, every read of haplotype 1 above every read of haplotype 2, no ties: only A0 and its complement reach the
    observed distance, so two == 2 and p = 2 / C(2k, k)."""
    f = [(k + 1 + i, 3 * k) for i in range(k)] + [(1 + i, 3 * k) for i in range(k)]
    for tags in ([0] * k + [1] * k, [1] * k + [0] * k):
        u0, total, le, ge, two = dp(f, tags)
        assert total == comb(2 * k, k) and two == 2 and u0 == (2 * k * k if tags[0] == 0 else 0)
        assert (le, ge) == ((total, 1) if tags[0] == 0 else (1, total))
    if k == 32:
        assert total == 1832624140942590534 < 2 ** 63


def test_all_tied_and_single_read():
    f = [(1 + i % 5, 2 * (1 + i % 5)) for i in range(64)]                # 64 reads at 1/2
    u0, total, le, ge, two = dp(f, [i % 2 for i in range(64)])
    assert u0 == 32 * 32 and le == ge == two == total == comb(64, 32)
    # n1 = 1: the read's rank among 9 distinct fractions decides everything
    f = [(i, 10) for i in range(1, 10)]
    for pos in range(9):
        tags = [1] * 9
        tags[pos] = 0
        u0, total, le, ge, two = dp(f, tags)
        d = abs(pos - 4)                                                # positions at least as far from the middle one
        assert (u0, total, le, ge) == (2 * pos, 9, pos + 1, 9 - pos) and two == (10 - 2 * d if d else 9)
    # n2 = 1 with ties: haplotype 2's read ties with two of haplotype 1's five
    f, tags = [(1, 2), (2, 4), (1, 3), (3, 4), (4, 5), (5, 10)], [0, 0, 0, 0, 0, 1]
    assert dp(f, tags) == brute(f, tags) and dp(f, tags)[1] == 6


def test_reference_window_rules():
    """status, the limit and what a status-2 window still carries."""
    for name, ((m, u, tags, mc), (nr, ns, cls, u2, ties, status)) in KNOWN.items():
        r = rankexact_ref(m, u, tags, mc)
        assert (r["n_reads"], r["n_short"], r["u2"], r["status"]) == (nr, ns, u2, status), name
        assert (r["total"] > 0) == (status == 0)
    m, u, tags = [1, 2, 3, 4, 5, 1], [5, 4, 3, 2, 1, 0], [0, 1, 0, 1, 0, 1]
    over = rankexact_ref(m, u, tags, 1, max_reads=5)
    assert over["status"] == 2 and (over["total"], over["le"], over["ge"], over["two"]) == (0, 0, 0, 0)
    assert over["u2"] == rank_ref(m, u, tags, 1)["u2"] > 0
    assert rankexact_ref(m, u, tags, 1, max_reads=6)["status"] == 0


def test_one_sided_against_scipy():
    """le / total and ge / total against scipy.stats.mannwhitneyu(method="exact")
    with alternative "less" / "greater" on tie-free windows of 2 .. 40 reads.
    scipy builds the distribution in doubles; the integers themselves are
    pinned by brute force above.  Largest relative deviation measured over
    these 120 windows (scipy 1.15.3): 3.98e-16, about two units in the last
    place; asserted at ten times that."""
    from scipy.stats import mannwhitneyu
    rng = np.random.default_rng(40)
    worst = 0.0
    for it in range(120):
        n1, n2 = int(rng.integers(1, 21)), int(rng.integers(1, 21))
        num = rng.permutation(997)[:n1 + n2] + 1                         # distinct numerators over one denominator
        f = [(int(a), 1000) for a in num]
        tags = [0] * n1 + [1] * n2
        u0, total, le, ge, two = dp(f, tags)
        x, y = [a / 1000 for a in num[:n1]], [a / 1000 for a in num[n1:]]
        for cnt, alt in ((le, "less"), (ge, "greater")):
            ref = mannwhitneyu(x, y, alternative=alt, method="exact")
            assert 2 * ref.statistic == u0
            worst = max(worst, abs(cnt / total - ref.pvalue) / ref.pvalue)
    print("largest relative deviation from scipy's exact p: %.3g" % worst)
    assert worst <= 3.98e-15


def test_rank_exact_p():
    from pomfret_amd import PomfretError, rank_exact_p
    assert rank_exact_p(2, 184756) == 2.0 / 184756.0 and rank_exact_p(0, 5) == 0.0 and rank_exact_p(7, 7) == 1.0
    big = comb(64, 32)
    assert rank_exact_p(2, big) == 2.0 / float(big) and rank_exact_p(big - 1, big) == float(big - 1) / float(big)
    assert rank_exact_p(2 ** 64 - 1, 2 ** 64 - 1) == 1.0
    for count, total in ((1, 0), (0, 0), (6, 5), (-1, 5), (1, 2 ** 64)):
        with pytest.raises(PomfretError):
            rank_exact_p(count, total)
    # the issue's table: k + k separated reads
    for k, p in ((8, 1.55e-4), (10, 1.08e-5), (12, 7.40e-7), (15, 1.29e-8), (20, 1.45e-11)):
        assert abs(rank_exact_p(2, comb(2 * k, k)) / p - 1) < 5e-3


def _xrecs():
    """test_ranktest's records, each with its window's exact test."""
    recs = _recs()
    for r, name in zip(recs, ["switch", "tied", "one-sided", "short", "shift"]):
        x = rankexact_ref(*KNOWN[name][0])
        assert x["u2"] == r["u2"]
        r.update(two=x["two"], total=x["total"], exact_status=x["status"])
    recs[5].update(two=0, total=0, exact_status=2)                        # 4,097 counted reads: neither test
    recs.append(dict(recs[0], start=900, end=990, two=0, total=0, exact_status=2))      # rank_p alone: best_p = rank_p
    return recs


def test_writer_bytes(tmp_path):
    from pomfret_amd.pipeline import write_rank, write_rank_exact
    p, q = str(tmp_path / "x.tsv"), str(tmp_path / "plain.tsv")
    recs = _xrecs()
    for bh in (False, True):
        assert write_rank_exact(p, recs, bh=bh) == (5, 4)
        got = open(p).read()
        assert got == rank_exact_text(recs, bh)
        assert write_rank(q, recs, bh=bh) == 5
        plain = open(q, "rb").read().split(b"\n")
        mine = open(p, "rb").read().split(b"\n")
        assert len(plain) == len(mine) and all(m.split(b"\t")[:17] == pl.split(b"\t") for m, pl in zip(mine[:-1], plain[:-1]))
        assert all(len(m.split(b"\t")) == 20 for m in mine[:-1])
    lines = open(p).read().splitlines()
    assert lines[0] == HEADER.rstrip("\n") + HEAD_EXTRA
    cols = [x.split("\t") for x in lines[1:]]
    # 3 v 3 apart: two of C(6, 3) = 20 subsets; every read tied: 6 of 6; one-sided and over the limit: nothing
    assert cols[0][17] == cols[0][18] == "0.1" and cols[1][17] == cols[1][18] == "1" and float(cols[0][15]) < 0.1
    assert cols[2][15:] == [".", ".", ".", ".", "."] and cols[5][15:] == [".", ".", ".", ".", "."]
    assert cols[6][17] == "." and cols[6][18] == cols[6][15] != "." and cols[6][19] != "."
    assert all(c[19] == "." for c in [x.split("\t") for x in rank_exact_text(recs, False).splitlines()[1:]])
    assert write_rank_exact(p, []) == (0, 0) and open(p).read() == HEADER.rstrip("\n") + HEAD_EXTRA + "\n"
    assert rank_text(recs, True).splitlines()[3] == "\t".join(cols[2][:17])


def test_writer_argument_errors(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import _bind, write_rank_exact
    from pomfret_amd.abi import PfRankRec
    p = str(tmp_path / "x.tsv")
    for two, total in ((21, 20), (1, 0)):
        bad = _xrecs()
        bad[0].update(two=two, total=total)
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            write_rank_exact(p, bad)
        assert not os.path.exists(p)
    with pytest.raises(PomfretError):
        write_rank_exact(str(tmp_path / "nodir" / "x.tsv"), _xrecs())
    assert _bind().pf_write_rank_exact(p.encode(), (PfRankRec * 1)(), None, 1, 0, None, None) == -1


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import PfHapmethRankExact, PfHapmethRankExactStats, PfRankExact, PfRankExactRec
    fields = {"pf_rank_exact_t": (PfRankExact, ["min_calls", "max_reads", "n_reads", "n_short", "status", "u2", "total", "le",
                                                "ge", "two", "ms_kernels"]),
              "pf_rank_exact_rec_t": (PfRankExactRec, ["two", "total", "status"]),
              "pf_hapmeth_rank_exact_t": (PfHapmethRankExact, ["max_reads"]),
              "pf_hapmeth_rank_exact_stats_t": (PfHapmethRankExactStats, ["n_exact", "n_over", "ms_kernels"])}
    names, exp = ["PF_RANK_EXACT_MAX_READS"], [64]
    for t, (cls, fs) in fields.items():
        names.append("sizeof(%s)" % t)
        exp.append(C.sizeof(cls))
        for f in fs:
            names.append("offsetof(%s, %s)" % (t, f))
            exp.append(getattr(cls, f).offset)
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == exp


def test_exact_needs_rank(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import DmrConfig, LoadConfig, PfHapmethDmr, PfHapmethOpts, PfHapmethRank, PfHapmethRankExact
    from pomfret_amd.pipeline import _bind, hapmeth_files
    out = str(tmp_path / "o")
    with pytest.raises(PomfretError):
        hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=DmrConfig(), rank_exact=True)
    for mx in (1, 65):
        with pytest.raises(PomfretError):
            hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=DmrConfig(), dmr_rank=True, rank_exact=True, rank_exact_max=mx)
    L = _bind()
    o = PfHapmethOpts(b"absent.bam", out.encode(), None, 0, 0, LoadConfig(min_len=0).to_c(), 1, 0, 0, 0)
    d = PfHapmethDmr(DmrConfig().to_c(), 1.0, None)

    def run(rank, mx):
        return L.pf_hapmeth_run_rank_exact(C.byref(o), C.byref(d), None, None, None, None, None,
                                           C.byref(PfHapmethRank(3)) if rank else None, C.byref(PfHapmethRankExact(mx)),
                                           None, None, None, None, None, None, None, None, None)
    assert run(False, 64) == -1 and run(True, 1) == -1 and run(True, 65) == -1
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.rank.tsv")


@pytest.mark.parametrize("args,word", [
    (["--dmr", "--dmr-rank-exact"], "--dmr-rank-exact needs --dmr-rank"),
    (["--dmr", "--dmr-rank", "--dmr-rank-exact-max", "8"], "--dmr-rank-exact-max needs --dmr-rank-exact"),
    (["--dmr", "--dmr-rank", "--dmr-rank-exact", "--dmr-rank-exact-max", "1"], "bad --dmr-rank-exact-max"),
    (["--dmr", "--dmr-rank", "--dmr-rank-exact", "--dmr-rank-exact-max", "65"], "bad --dmr-rank-exact-max"),
    (["--regions", "r.bed", "--dmr-rank", "--dmr-rank-exact", "--dmr-rank-exact-max", "8x"], "bad --dmr-rank-exact-max")])
def test_cli_option_errors(tmp_path, args, word):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    assert "absent.bam or its index" not in r.stderr and "no usable GPU" not in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.rank.tsv")


def test_cli_help_and_valid_line(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1 and "is not computed" not in r.stderr
    for word in ("--dmr-rank-exact", "--dmr-rank-exact-max", "exact_p", "best_p", "best_q", "2 .. 64", "[64]"):
        assert word in r.stderr, word
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--dmr", "--dmr-rank", "--dmr-rank-exact", "--dmr-rank-exact-max", "2",
                        str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
