"""The host side of `hapmeth --regions` (no GPU): the BED loader, the
Benjamini-Hochberg q-values against the literal formula, the writer's bytes,
the struct layouts, the additivity of the reference and the CLI option checks."""
import ctypes as C
import gzip
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from pomfret_amd.abi import DmrConfig

from tests._regions_ref import HEADER, PERM_COLUMNS, add, bh_ref, region_ref, regions_text, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
NAMES = ["chr1", "chr2", "chrM"]

BED = ("# a comment\n"
       "track name=icr description=\"known ICRs\"\n"
       "browser position chr1:1-100\n"
       "chr2\t500\t900\tH19\t0\t+\n"
       "\n"
       "chr1\t300\t400\n"
       "chr1 100 200 spaced extra columns\n"
       "chrUn\t1\t2\tunknown\n"
       "chr1\t100\t150\tfirst_tie\n"
       "chr1\t100\t200\tsecond\r\n"
       "chr1\t100\t150\tsecond_tie\n"
       "chr1\t7\t7\tempty\n"
       "chrUn2\t5\t9\n"
       "chr2\t0\t536870912\twhole")                        # 2^29, and no final newline


def _load(tmp_path, text, name="r.bed", names=NAMES):
    from pomfret_amd.pipeline import regions_load
    p = tmp_path / name
    if name.endswith(".gz"):
        with gzip.open(p, "wb") as f:
            f.write(text.encode())
    else:
        p.write_bytes(text.encode())
    return regions_load(str(p), names)


@pytest.mark.parametrize("name", ["r.bed", "r.bed.gz"])
def test_load_sorts_skips_and_reads_the_last_line(tmp_path, name):
    got = _load(tmp_path, BED, name)
    c1, c2, cm = got["contigs"]
    # stably sorted by (start, end): ties keep file order; the unsorted file's order is gone
    assert list(zip(c1["start"], c1["end"], c1["name"])) == [
        (7, 7, "empty"), (100, 150, "first_tie"), (100, 150, "second_tie"), (100, 200, "spaced"), (100, 200, "second"),
        (300, 400, ".")]
    # the last line has no newline and is read
    assert list(zip(c2["start"], c2["end"], c2["name"])) == [(0, 2 ** 29, "whole"), (500, 900, "H19")]
    assert cm == dict(start=[], end=[], name=[]) and got["n_unknown_contig"] == 2


def test_load_empty_and_absent(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import regions_load
    got = _load(tmp_path, "")
    assert all(c["start"] == [] for c in got["contigs"]) and got["n_unknown_contig"] == 0
    assert _load(tmp_path, "#only\n\n   \ntrack x\n")["contigs"][0]["start"] == []
    assert _load(tmp_path, "chr1\t1\t2\n", names=[])["n_unknown_contig"] == 1
    with pytest.raises(PomfretError):
        regions_load(str(tmp_path / "absent.bed"), NAMES)


@pytest.mark.parametrize("line,word,code", [
    ("chr1\t5", "fewer than three columns", "argument"), ("chr1\t5\tx9", "not a number", "argument"),
    ("chr1\t-1\t9", "not a number", "argument"), ("chr1\t10\t9", "start is above end", "argument"),
    ("chrUn\t10\t9", "start is above end", "argument"), ("chr1\t0\t536870913", "above 2^29", "limit")])
def test_load_errors_name_the_line(tmp_path, capfd, line, word, code):
    from pomfret_amd import PomfretError
    text = "#c\nchr1\t1\t2\n\ntrack t\n" + line + "\nchr1\t3\t4\n"
    for tail in ("", "cut"):                                   # also as the last line, without a newline
        capfd.readouterr()
        with pytest.raises(PomfretError, match=code):
            _load(tmp_path, text if not tail else text[:text.index(line) + len(line)])
        err = capfd.readouterr().err
        assert "line 5:" in err and word in err and "r.bed" in err


def _bh(hits, tested, n_perm):
    from pomfret_amd.pipeline import bh_adjust
    got = bh_adjust(hits, tested, n_perm).tolist()
    ref = bh_ref(list(hits), list(tested), n_perm)
    assert [struct.pack("<d", x) for x in got] == [struct.pack("<d", x) for x in ref]     # the bits, NaN included
    return got


def test_bh_hand_worked():
    # four tests, 99 permutations: p = 0.01, 0.02, 0.03, 0.5; p * 4 / rank = 0.04, 0.04, 0.04, 0.5
    q = _bh([0, 1, 2, 49], [1, 1, 1, 1], 99)
    assert q == pytest.approx([0.04, 0.04, 0.04, 0.5], rel=1e-12) and q[0] <= q[1] <= q[2]
    # the monotone step: a later, smaller value reaches back
    q = _bh([9, 10, 11], [1, 1, 1], 99)
    assert q[0] == q[1] == q[2] == pytest.approx(0.12, rel=1e-12)
    # ties share the largest rank, and their value
    q = _bh([4, 4, 4, 0], [1, 1, 1, 1], 9)
    assert q == [0.5] * 3 + [pytest.approx(0.4, rel=1e-12)]
    # untested entries are NaN and do not count in m
    q = _bh([0, 7, 1, 99], [1, 0, 1, 0], 99)
    assert math.isnan(q[1]) and math.isnan(q[3]) and q[0] == q[2] == pytest.approx(0.02, rel=1e-12)
    # never above 1: 0.99 * 2 / 1 is cut, and so is its successor's 1.0 * 2 / 2
    assert _bh([99, 99], [1, 1], 99) == [1.0, 1.0] and _bh([98, 99], [1, 1], 99) == [1.0, 1.0]


def test_bh_all_untested_m_one_and_empty():
    assert all(math.isnan(x) for x in _bh([3, 4], [0, 0], 99))
    assert _bh([3], [1], 99) == [0.04] and _bh([0, 5], [0, 1], 9)[1] == 0.6
    assert _bh([], [], 99) == []


def test_bh_random_against_the_formula():
    rng = np.random.default_rng(5)
    for n, n_perm in ((1, 1), (7, 9), (40, 99), (200, 999)):
        hits = rng.integers(0, n_perm + 1, n)
        hits[rng.random(n) < 0.3] = hits[0]                    # ties
        _bh(hits.tolist(), (rng.random(n) < 0.8).astype(int).tolist(), n_perm)


def _recs():
    F = 2 ** 31
    return [dict(chrom="chr7", start=100, end=161, name="A", n_cpg=9, n_sites=6, n_pos=5, n_neg=0, sum=[12, 0, 0, 11],
                 evidence=3 * 65536 + 32768, test=(14, 15, 0, 0)),
            dict(chrom="chr7", start=100, end=161, name=".", n_cpg=9, n_sites=6, n_pos=0, n_neg=4, sum=[0, 5, 5, 0],
                 evidence=-70000, test=(3, 2, 0, 2)),                                       # status 2: no p
            dict(chrom="chr7", start=5000, end=5000, name="empty", n_cpg=0, n_sites=0, n_pos=0, n_neg=0, sum=[0, 0, 0, 0],
                 evidence=0),
            dict(chrom="chr9", start=0, end=2 ** 29, name="whole", n_cpg=70000, n_sites=69000, n_pos=3, n_neg=2,
                 sum=[F, 7, F + 1, 9], evidence=2 ** 40),                                   # past INT32_MAX: no pooled_p
            dict(chrom="chr8", start=10, end=900, name="cut", n_cpg=5, n_sites=5, n_pos=0, n_neg=0, sum=[30, 2, 30, 2],
                 evidence=0, split=True),
            dict(chrom="chr8", start=10, end=400, name="t2", n_cpg=5, n_sites=5, n_pos=1, n_neg=1, sum=[30, 2, 3, 40],
                 evidence=12345, test=(8, 9, 4, 0))]


def test_writer_bytes(tmp_path):
    from pomfret_amd import fisher_exact
    from pomfret_amd.pipeline import write_regions
    p = str(tmp_path / "o.regions.bed")
    recs = _recs()
    assert write_regions(p, recs) == 0
    p3 = "%.6g" % fisher_exact(30, 2, 3, 40)[3]
    exp = [HEADER + "\n",
           "chr7\t100\t161\tA\t9\t6\t5\t0\th1>h2\t12\t0\t0\t11\t1.0000\t7.39602e-07\t3.500\tok\n",
           "chr7\t100\t161\t.\t9\t6\t0\t4\th1<h2\t0\t5\t5\t0\t-1.0000\t0.00793651\t-1.068\tok\n",
           "chr7\t5000\t5000\tempty\t0\t0\t0\t0\t.\t0\t0\t0\t0\t0.0000\t1\t0.000\tok\n",
           "chr9\t0\t536870912\twhole\t70000\t69000\t3\t2\th1>h2\t2147483648\t7\t2147483649\t9\t0.0000\t.\t16777216.000\tok\n",
           "chr8\t10\t900\tcut\t5\t5\t0\t0\t.\t30\t2\t30\t2\t0.0000\t1\t0.000\tsplit\n",
           f"chr8\t10\t400\tt2\t5\t5\t1\t1\th1>h2\t30\t2\t3\t40\t0.8677\t{p3}\t0.188\tok\n"]
    assert open(p).read() == "".join(exp)
    # the reference writes the same text; a break on a region's edge does not split it
    breaks = {"chr8": [10, 500], "chr7": [100, 161]}
    assert regions_text(recs, breaks=breaks) == "".join(exp)
    # with the permutation columns: two tests, 99 permutations; p = 0.01 and 0.05, q = min(0.02, 0.05) and 0.05
    assert write_regions(p, recs, perm=True, n_perm=99) == 2
    tail = ["\t14\t15\t0.01\t0.02", "\t3\t2\t.\t.", "\t.\t.\t.\t.", "\t.\t.\t.\t.", "\t.\t.\t.\t.", "\t8\t9\t0.05\t0.05"]
    assert open(p).read() == exp[0][:-1] + PERM_COLUMNS + "\n" + "".join(a[:-1] + b + "\n" for a, b in zip(exp[1:], tail))
    assert regions_text(recs, perm=[r.get("test") for r in recs], n_perm=99, breaks=breaks) == open(p).read()
    assert write_regions(p, []) == 0 and open(p).read() == HEADER + "\n"
    from pomfret_amd import PomfretError
    with pytest.raises(PomfretError):
        write_regions(str(tmp_path / "nodir" / "x.bed"), recs)


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import (REGION_SUM_DTYPE, PfHapmethRegions, PfHapmethRegionsStats, PfRegionRec, PfRegions,
                                 PfRegionSum)
    src = tmp_path / "l.c"
    names = ["sizeof(pf_region_sum_t)", "offsetof(pf_region_sum_t, n_neg)", "offsetof(pf_region_sum_t, sum)",
             "offsetof(pf_region_sum_t, evidence)", "sizeof(pf_regions_t)", "offsetof(pf_regions_t, r)",
             "offsetof(pf_regions_t, n_informative)", "offsetof(pf_regions_t, ms_kernels)",
             "offsetof(pf_regions_t, ms_upload)", "sizeof(pf_region_rec_t)", "offsetof(pf_region_rec_t, start)",
             "offsetof(pf_region_rec_t, s)", "offsetof(pf_region_rec_t, flags)", "offsetof(pf_region_rec_t, reads)",
             "offsetof(pf_region_rec_t, status)", "sizeof(pf_hapmeth_regions_t)", "sizeof(pf_hapmeth_regions_stats_t)",
             "offsetof(pf_hapmeth_regions_stats_t, n_untested)", "offsetof(pf_hapmeth_regions_stats_t, ms_kernels)",
             "(size_t)PF_REGION_TEST_MAX_SPAN", "(size_t)PF_REGION_SPLIT", "(size_t)PF_REGION_ELIGIBLE",
             "sizeof(pf_hapmeth_opts_t)", "sizeof(pf_hapmeth_dmr_t)", "sizeof(pf_dmr_cfg_t)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    from pomfret_amd.abi import REGION_ELIGIBLE, REGION_SPLIT, REGION_TEST_MAX_SPAN, PfDmrCfg, PfHapmethDmr, PfHapmethOpts
    exp = [C.sizeof(PfRegionSum), PfRegionSum.n_neg.offset, PfRegionSum.sum.offset, PfRegionSum.evidence.offset,
           C.sizeof(PfRegions), PfRegions.r.offset, PfRegions.n_informative.offset, PfRegions.ms_kernels.offset,
           PfRegions.ms_upload.offset, C.sizeof(PfRegionRec), PfRegionRec.start.offset, PfRegionRec.s.offset,
           PfRegionRec.flags.offset, PfRegionRec.reads.offset, PfRegionRec.status.offset, C.sizeof(PfHapmethRegions),
           C.sizeof(PfHapmethRegionsStats), PfHapmethRegionsStats.n_untested.offset, PfHapmethRegionsStats.ms_kernels.offset,
           REGION_TEST_MAX_SPAN, REGION_SPLIT, REGION_ELIGIBLE, C.sizeof(PfHapmethOpts), C.sizeof(PfHapmethDmr),
           C.sizeof(PfDmrCfg)]
    assert got == exp
    assert REGION_SUM_DTYPE.itemsize == C.sizeof(PfRegionSum) == 56
    assert [REGION_SUM_DTYPE.fields[k][1] for k in ("n_neg", "sum", "evidence")] == \
        [PfRegionSum.n_neg.offset, PfRegionSum.sum.offset, PfRegionSum.evidence.offset]
    assert C.sizeof(PfHapmethOpts) == 64 and C.sizeof(PfHapmethDmr) == 32 and C.sizeof(PfDmrCfg) == 16    # no struct grew


def test_reference_is_additive():
    """Two disjoint site ranges add field by field to the whole, for every region."""
    rng = np.random.default_rng(8)
    n = 300
    pos = 50 + np.cumsum(rng.integers(1, 20, n))
    cnt = np.zeros((n, 6), np.uint32)
    cnt[:, :4] = rng.integers(0, 30, (n, 4))
    cfg = DmrConfig()
    starts = rng.integers(0, int(pos[-1]), 60)
    ends = starts + rng.integers(0, 2000, 60)
    whole = region_ref(pos, cnt, cfg, starts, ends)
    assert whole["n_sites"].max() > 20 and (whole["n_cpg"] == 0).any()
    for j in (0, 1, 137, n - 1, n):
        same(add(region_ref(pos[:j], cnt[:j], cfg, starts, ends), region_ref(pos[j:], cnt[j:], cfg, starts, ends)), whole, j)


@pytest.mark.parametrize("args", [["--dmr"], ["--dmr-hmm"], ["--dmr", "--dmr-hmm"], ["--dmr-gap", "300"],
                                  ["--dmr-hmm-switch", "4"]])
def test_cli_regions_excludes_the_other_source(tmp_path, args):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--regions", str(tmp_path / "r.bed")] + args + [str(tmp_path / "absent.bam")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and "--regions" in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.regions.bed")


@pytest.mark.parametrize("args", [["--assign"], ["--tag-check"], ["--dmr-perm", "99", "--dmr-seed", "3"],
                                  ["--assign", "--assign-min-llr", "2", "--assign-min-calls", "3"],
                                  ["--dmr-min-cov", "4", "--dmr-delta", "30", "--dmr-min-sites", "3", "--dmr-max-p", "0.05",
                                   "--dmr-blocks", "b.gtf"]])
def test_cli_regions_stands_in_for_dmr(tmp_path, args):
    """The option check passes: the run gets as far as the BAM."""
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out, "--regions", str(tmp_path / "r.bed")] + args + [str(tmp_path / "absent.bam")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.regions.bed")
    # and without a source of regions the same options are refused as before
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and "need" in r.stderr


def test_cli_help_names_the_option():
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1 and "--regions FILE" in r.stderr and "perm_q" in r.stderr and "Benjamini-Hochberg" in r.stderr


def test_api_regions_excludes_dmr_hmm(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import HmmConfig
    from pomfret_amd.pipeline import hapmeth_files
    with pytest.raises(PomfretError, match="excludes"):
        hapmeth_files(str(tmp_path / "a.bam"), str(tmp_path / "o"), regions=str(tmp_path / "r.bed"), dmr_hmm=HmmConfig())
