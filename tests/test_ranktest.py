"""hapmeth --dmr-rank's host side: the reference's own known answers and its
agreement with scipy's Mann-Whitney U, pf_rank_p against scipy's asymptotic
p-value and its edge cases, pf_bh_adjust_p against a Python loop, the
writer's bytes (pf_write_rank), the new structs' layout, and the entry
point's and the CLI's option checks.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests._rank_ref import bh_ref, rank_p_ref, rank_ref, rank_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
HEADER = ("#chrom\tstart\tend\treads_h1\treads_h2\tshort_h1\tshort_h2\tallmeth_h1\tallunmeth_h1\tmixed_h1\tallmeth_h2"
          "\tallunmeth_h2\tmixed_h2\tauc\tz\trank_p\trank_q\n")

# (m, u, tags, min_calls) -> (n_reads, n_short, cls, u2, ties, status), worked by hand:
#   switch     fractions 1,1,1 | 0,0,0: G = 9; two tie groups of three, 2 * (27 - 3)
#   tied       1/2, 2/4, 3/6, 50/100 across both haplotypes: E = 4; one group of four, 64 - 4
#   one-sided  no read of haplotype 2: nothing to test
#   short      min_calls 3 leaves 3/3 against 2/4: G = 1; one short read each
#   shift      3/4, 1/4 | 2/4, 1/2: G = 2; the pair of 1/2 ties, 8 - 2
#   no-h1      min_calls takes haplotype 1's only read away
KNOWN = {
    "switch": (([5, 5, 5, 0, 0, 0], [0, 0, 0, 5, 5, 5], [0, 0, 0, 1, 1, 1], 1),
               ([3, 3], [0, 0], [[3, 0, 0], [0, 3, 0]], 18, 48, 0)),
    "tied": (([1, 2, 3, 50], [1, 2, 3, 50], [0, 1, 0, 1], 1), ([2, 2], [0, 0], [[0, 0, 2], [0, 0, 2]], 4, 60, 0)),
    "one-sided": (([3, 4], [1, 0], [0, 0], 1), ([2, 0], [0, 0], [[1, 0, 1], [0, 0, 0]], 0, 0, 1)),
    "short": (([3, 1, 0, 2], [0, 0, 1, 2], [0, 0, 1, 1], 3), ([1, 1], [1, 1], [[1, 0, 0], [0, 0, 1]], 2, 0, 0)),
    "shift": (([3, 1, 2, 1], [1, 3, 2, 1], [0, 0, 1, 1], 1), ([2, 2], [0, 0], [[0, 0, 2], [0, 0, 2]], 4, 6, 0)),
    "no-h1": (([1, 4, 0], [1, 0, 4], [0, 1, 1], 3), ([0, 2], [1, 0], [[0, 0, 0], [1, 1, 0]], 0, 0, 1)),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_reference_known_answers(name):
    (m, u, tags, mc), (nr, ns, cls, u2, ties, status) = KNOWN[name]
    r = rank_ref(m, u, tags, mc)
    assert (r["n_reads"], r["n_short"], r["cls"], r["u2"], r["ties"], r["status"]) == (nr, ns, cls, u2, ties, status)
    assert sum(r["sum"]) == sum(a + b for a, b in zip(m, u) if a + b >= mc)


def _sample(rng, n1, n2, top):
    m, u = rng.integers(0, top, n1 + n2), rng.integers(0, top, n1 + n2)
    m[(m + u) == 0] = 1
    return m.tolist(), u.tolist(), [0] * n1 + [1] * n2


def _scipy(m, u, tags):
    from scipy.stats import mannwhitneyu
    f = [a / (a + b) for a, b in zip(m, u)]
    x, y = [v for v, t in zip(f, tags) if t == 0], [v for v, t in zip(f, tags) if t == 1]
    return mannwhitneyu(x, y, alternative="two-sided", method="asymptotic", use_continuity=True)


def test_reference_is_scipys_u():
    """2 * statistic == u2, also through the numpy path past 300 reads."""
    rng = np.random.default_rng(11)
    for n1, n2, top in [(1, 1, 3), (5, 9, 4), (30, 30, 6), (64, 65, 40), (200, 150, 40)]:
        m, u, tags = _sample(rng, n1, n2, top)
        r = rank_ref(m, u, tags, 1)
        assert r["status"] == 0 and 2 * _scipy(m, u, tags).statistic == r["u2"], (n1, n2)
    # the two paths of the reference agree at a size both can run
    m, u, tags = _sample(rng, 160, 150, 5)
    small = rank_ref(m[:300], u[:300], tags[:300], 2)
    one = rank_ref(m[:300] + [0], u[:300] + [1], tags[:300] + [1], 2)         # 301 with a short read: 300 counted
    assert (one["u2"], one["ties"]) == (small["u2"], small["ties"])
    big = rank_ref(m, u, tags, 1)                                               # 310: the numpy path
    assert 2 * _scipy(m, u, tags).statistic == big["u2"]
    lit = sum((a * (c + d) > c * (a + b)) * 2 + (a * (c + d) == c * (a + b))
              for a, b, s in zip(m, u, tags) if s == 0 for c, d, t in zip(m, u, tags) if t == 1)
    assert lit == big["u2"]


def test_rank_p_against_scipy():
    """pf_rank_p against scipy's asymptotic two-sided p with tie and continuity
    correction, at rel 1e-6 / abs 1e-300 (the tolerance of tests/test_oracle.py),
    and bit for bit against the Python loop of the same steps up to erfc.
    Largest relative difference to scipy seen over these 400 samples: 8.5e-15
    in p (scipy 1.15.3)."""
    from pomfret_amd import rank_p
    rng = np.random.default_rng(2024)
    worst = 0.0
    for k in range(400):
        n1, n2 = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        m, u, tags = _sample(rng, n1, n2, int(rng.integers(2, 30)))
        if k % 5 == 0:                                        # a shifted haplotype: small p-values too
            m = [a + 20 if t == 0 else a for a, t in zip(m, tags)]
        r = rank_ref(m, u, tags, 1)
        auc, z, p = rank_p(r["u2"], n1, n2, r["ties"])
        ref = _scipy(m, u, tags)
        if math.isnan(ref.pvalue):                            # scipy divides by zero where every read ties
            assert r["ties"] == (n1 + n2) ** 3 - (n1 + n2) and (z, p) == (0.0, 1.0)
            continue
        assert p == pytest.approx(ref.pvalue, rel=1e-6, abs=1e-300), (k, p, ref.pvalue)
        assert auc == r["u2"] / (2.0 * n1 * n2)
        a2, z2, p2 = rank_p_ref(r["u2"], n1, n2, r["ties"])
        assert (auc, z) == (a2, z2) and p == pytest.approx(p2, rel=1e-15)
        if ref.pvalue > 0:
            worst = max(worst, abs(p - ref.pvalue) / ref.pvalue)
    print("largest relative difference to scipy: %.3g" % worst)
    assert worst < 1e-6


def test_rank_p_cases():
    from pomfret_amd import PomfretError, rank_p
    # every read tied: the variance is 0
    n = 7 + 5
    assert rank_p(7 * 5, 7, 5, n ** 3 - n) == (0.5, 0.0, 1.0)
    auc, z, p = rank_p(4, 2, 2, 60)                           # KNOWN["tied"]
    assert (auc, z, p) == (0.5, 0.0, 1.0)
    # u2 == n1 * n2 without ties: the continuity correction would go below 0
    assert rank_p(30 * 40, 30, 40, 0) == (0.5, 0.0, 1.0)
    assert rank_p(30 * 40 + 1, 30, 40, 0)[1:] == (0.0, 1.0)   # |u2 - a| / 2 = 0.5
    assert rank_p(30 * 40 + 2, 30, 40, 0)[2] < 1.0
    # complete separation of 2,000 against 2,000: p underflows, z does not
    auc, z, p = rank_p(2 * 2000 * 2000, 2000, 2000, 0)
    assert auc == 1.0 and p == 0.0 and 54.0 < z < 55.0 and math.isfinite(z)
    auc, z2, p = rank_p(0, 2000, 2000, 0)
    assert auc == 0.0 and p == 0.0 and z2 == z
    # the largest window: 4,096 counted reads
    assert rank_p(2 * 2048 * 2048, 2048, 2048, 2 * (2048 ** 3 - 2048))[0] == 1.0
    for bad in ((0, 0, 5, 0), (0, 5, 0, 0), (2 * 4 * 5 + 1, 4, 5, 0)):
        with pytest.raises(PomfretError, match=r"\(-1\)"):
            rank_p(*bad)


def test_bh_adjust_p():
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import bh_adjust_p
    # by hand: m = 4; 0.04*4/4 = 0.04, 0.03*4/3 = 0.04, 0.01*4/2 = 0.02, 0.005*4/1 = 0.02
    q = bh_adjust_p([0.01, 0.04, 0.03, 0.005], [1, 1, 1, 1])
    assert q.tolist() == pytest.approx([0.02, 0.04, 0.04, 0.02], rel=1e-15)
    # equal p-values share the last rank; untested entries are NaN and do not count in m
    q = bh_adjust_p([0.03, 0.5, 0.03, 0.001, 0.03, 0.9], [1, 0, 1, 1, 1, 1])
    assert math.isnan(q[1]) and q[0] == q[2] == q[4] == (0.03 * 5.0) / 4.0 and q[3] == (0.001 * 5.0) / 1.0 and q[5] == 0.9
    assert bh_adjust_p([0.6, 0.9], [1, 1]).tolist() == [0.9, 0.9] and bh_adjust_p([0.8], [1]).tolist() == [0.8]
    assert bh_adjust_p([], []).size == 0 and np.isnan(bh_adjust_p([0.1, 0.2], [0, 0])).all()
    assert bh_adjust_p([0.0, 0.0, 1.0], [1, 1, 1]).tolist() == [0.0, 0.0, 1.0]
    rng = np.random.default_rng(8)
    for n in (1, 2, 17, 400):
        p = rng.choice(np.concatenate([rng.random(n), [0.0, 1.0, 1e-300, 0.25, 0.25]]), n)
        p[rng.random(n) < 0.3] = 0.25                          # many exactly equal
        t = rng.random(n) < 0.8
        got, ref = bh_adjust_p(p, t), bh_ref(p.tolist(), t.tolist())
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isnan(got), ~t)
        assert got[t].tobytes() == np.asarray(ref, np.float64)[t].tobytes(), n
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        bh_adjust_p([0.1, float("nan")], [1, 1])
    assert math.isnan(bh_adjust_p([0.1, float("nan")], [1, 0])[1])
    with pytest.raises(PomfretError):
        bh_adjust_p([0.1], [1, 1])


def _recs():
    recs = []
    for k, name in enumerate(["switch", "tied", "one-sided", "short", "shift"]):
        r = rank_ref(*KNOWN[name][0])
        recs.append(dict(r, chrom="chr7" if k < 3 else "chrQ", start=100 * k, end=100 * k + 61))
    recs.append(dict(n_reads=[4000, 97], n_short=[1, 2], cls=[[1, 2, 3997], [90, 3, 4]], u2=0, ties=0, status=2, chrom="chrQ",
                     start=7, end=9))
    return recs


def test_writer_bytes(tmp_path):
    from pomfret_amd.pipeline import write_rank
    p = str(tmp_path / "o.rank.tsv")
    recs = _recs()
    assert write_rank(p, recs) == 4
    got = open(p).read()
    assert got == rank_text(recs, False)
    lines = got.splitlines(True)
    # by hand: 3 v 3 apart: var = 9/12 * (7 - 48/30) = 4.05, d = 9/2 - 0.5 = 4, z = 4 / sqrt(4.05)
    z = 4.0 / math.sqrt(4.05)
    assert lines[0] == HEADER
    assert lines[1] == "chr7\t0\t61\t3\t3\t0\t0\t3\t0\t0\t0\t3\t0\t1.0000\t%.3f\t%.6g\t.\n" % (z, math.erfc(z / math.sqrt(2.0)))
    assert lines[1].split("\t")[14] == "1.988"
    assert lines[2] == "chr7\t100\t161\t2\t2\t0\t0\t0\t0\t2\t0\t0\t2\t0.5000\t0.000\t1\t.\n"
    assert lines[3] == "chr7\t200\t261\t2\t0\t0\t0\t1\t0\t1\t0\t0\t0\t.\t.\t.\t.\n"
    assert lines[6] == "chrQ\t7\t9\t4000\t97\t1\t2\t1\t2\t3997\t90\t3\t4\t.\t.\t.\t.\n"
    # with q-values: Benjamini-Hochberg over the four tested records
    assert write_rank(p, recs, bh=True) == 4
    got = open(p).read()
    assert got == rank_text(recs, True)
    qs = [l.rstrip("\n").split("\t")[16] for l in got.splitlines()[1:]]
    assert qs[2] == qs[5] == "." and qs[1] == "1" and float(qs[0]) > float(lines[1].split("\t")[15])
    # no record: the header alone
    assert write_rank(p, []) == 0 and open(p).read() == HEADER
    assert write_rank(p, [], bh=True) == 0 and open(p).read() == HEADER


def test_writer_argument_errors(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import write_rank
    with pytest.raises(PomfretError):
        write_rank(str(tmp_path / "nodir" / "x.tsv"), _recs())
    bad = _recs()
    bad[0]["u2"] = 19                                          # above 2 * n1 * n2 with status 0
    p = str(tmp_path / "x.tsv")
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        write_rank(p, bad)
    assert not os.path.exists(p)


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import PfHapmethRank, PfHapmethRankStats, PfRank, PfRankRec
    fields = {"pf_rank_t": (PfRank, ["min_calls", "n_reads", "n_short", "cls", "sum", "u2", "ties", "status", "ms_kernels"]),
              "pf_rank_rec_t": (PfRankRec, ["start", "end", "reads", "n_short", "cls", "status", "u2", "ties"]),
              "pf_hapmeth_rank_t": (PfHapmethRank, ["min_calls"]),
              "pf_hapmeth_rank_stats_t": (PfHapmethRankStats, ["n_untested", "n_records", "ms_kernels"])}
    names, exp = ["PF_RANK_MAX_READS"], [4096]
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


def test_rank_needs_dmr(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import DmrConfig, LoadConfig, PfHapmethDmr, PfHapmethOpts, PfHapmethRank
    from pomfret_amd.pipeline import _bind, hapmeth_files
    out = str(tmp_path / "o")
    with pytest.raises(PomfretError):
        hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=None, dmr_rank=True)
    for mc in (0, 65536):
        with pytest.raises(PomfretError):
            hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=DmrConfig(), dmr_rank=True, dmr_rank_min_calls=mc)
    # the entry point itself, before the BAM is opened
    L = _bind()
    o = PfHapmethOpts(b"absent.bam", out.encode(), None, 0, 0, LoadConfig(min_len=0).to_c(), 1, 0, 0, 0)
    d = PfHapmethDmr(DmrConfig().to_c(), 1.0, None)

    def run(dm, mc):
        return L.pf_hapmeth_run_rank(C.byref(o), dm, None, None, None, None, None, C.byref(PfHapmethRank(mc)),
                                     None, None, None, None, None, None, None, None)
    assert run(None, 3) == -1 and run(C.byref(d), 0) == -1 and run(C.byref(d), 65536) == -1
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.rank.tsv")


@pytest.mark.parametrize("args,word", [
    (["--dmr-rank"], "--dmr-rank needs --dmr or --regions"),
    (["--dmr", "--dmr-rank-min-calls", "4"], "--dmr-rank-min-calls needs --dmr-rank"),
    (["--dmr-rank-min-calls", "4"], "--dmr-rank-min-calls needs --dmr-rank"),
    (["--dmr", "--dmr-rank", "--dmr-rank-min-calls", "0"], "bad --dmr-rank-min-calls"),
    (["--dmr", "--dmr-rank", "--dmr-rank-min-calls", "65536"], "bad --dmr-rank-min-calls"),
    (["--regions", "r.bed", "--dmr-rank", "--dmr-rank-min-calls", "3x"], "bad --dmr-rank-min-calls")])
def test_cli_option_errors(tmp_path, args, word):
    """Reported before any device is opened: the run gets no further than its options."""
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    assert "absent.bam or its index" not in r.stderr and "no usable GPU" not in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.rank.tsv")


def test_cli_help_and_valid_line(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1
    for word in ("--dmr-rank", "--dmr-rank-min-calls", "rank_p", "rank_q", "asymptotic", "eight reads", "z > 38",
                 "not a measured optimum"):
        assert word in r.stderr, word
    out = str(tmp_path / "o")
    for src in (["--dmr"], ["--regions", str(tmp_path / "r.bed")]):
        r = subprocess.run([EXE, "hapmeth", "-o", out] + src + ["--dmr-rank", "--dmr-rank-min-calls", "65535",
                            str(tmp_path / "absent.bam")], capture_output=True, text=True)
        assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
        assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.rank.tsv")
