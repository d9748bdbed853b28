"""The hidden Markov model of pf_dmr_hmm_regions on the CPU: the host's
evidence function against the literal reference (tests/_dmr_hmm_ref.py), the
case the model exists for, the bindings' struct layouts and the CLI's argument
errors.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from pomfret_amd.abi import DmrConfig, HmmConfig

from tests._assign_ref import ilog2_q16 as L
from tests._dmr_hmm_ref import CLAMP, evidence, hmm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
CFG = DmrConfig(min_cov=5, min_delta_pct=40, max_gap=500, min_sites=5)


def _lib_e(c):
    from pomfret_amd._lib import lib
    return int(lib().pf_dmr_hmm_evidence(*[int(x) for x in c]))


def _raw(m1, u1, m2, u2):
    """sep - pool before the clamp."""
    n1, n2 = m1 + u1, m2 + u2
    m, u, n = m1 + m2, u1 + u2, n1 + n2
    sep = (m1 * (L(m1 + 1) - L(n1 + 2)) + u1 * (L(u1 + 1) - L(n1 + 2)) +
           m2 * (L(m2 + 1) - L(n2 + 2)) + u2 * (L(u2 + 1) - L(n2 + 2)))
    return sep - (m * (L(m + 1) - L(n + 2)) + u * (L(u + 1) - L(n + 2)))


def test_evidence_small_counts():
    for c in itertools.product(range(9), repeat=4):
        assert _lib_e(c) == evidence(*c), c


def test_evidence_corners_and_random_counts():
    F = 65535
    cases = list(itertools.product((0, F), repeat=4)) + [(F, 0, 1, 0), (1, F, F, 1), (F - 1, F, F, F - 1)]
    rng = np.random.default_rng(5)
    cases += rng.integers(0, 65536, (300, 4)).tolist() + rng.integers(0, 60, (300, 4)).tolist()
    for c in cases:
        e = _lib_e(c)
        assert e == evidence(*c), c
        assert abs(e) <= CLAMP
    # the sign is the direction's: swapping the haplotypes negates it
    assert _lib_e((8, 2, 2, 8)) == -_lib_e((2, 8, 8, 2)) > 0


def test_evidence_special_cases():
    # no direction: equal levels, whatever the depth
    for c in ((5, 5, 5, 5), (3, 6, 10, 20), (0, 7, 0, 9), (0, 0, 0, 0)):
        assert c[0] * (c[2] + c[3]) == c[2] * (c[0] + c[1]) and _lib_e(c) == evidence(*c) == 0
    # the clamp binds: two full counters in opposite states are worth 2^33 bits raw
    assert _raw(65535, 0, 0, 65535) > CLAMP and _lib_e((65535, 0, 0, 65535)) == CLAMP
    assert _lib_e((0, 65535, 65535, 0)) == -CLAMP
    # the smoothing makes "two levels" the worse model: g is 0 although the levels differ
    c = (0, 3, 3, 12)
    assert _raw(*c) < 0 and c[0] * (c[2] + c[3]) != c[2] * (c[0] + c[1]) and _lib_e(c) == evidence(*c) == 0
    # a hand-checked site: 3 / 0 against 0 / 3 -- sep = 6 * (L(4) - L(5)), pool = 6 * (L(4) - L(8))
    assert _lib_e((3, 0, 0, 3)) == 6 * (L(8) - L(5)) == evidence(3, 0, 0, 3)


def planted_pile(seed, lens=(200, 40, 250, 40, 250, 12, 100)):
    """A contig of CpGs with about 10 calls per haplotype: flat stretches (both
    haplotypes at 50 %) alternate with planted regions at 85 % / 15 % (every
    second one the other way round).  Returns pos, cnt [n, 6] and the planted
    regions as (first site, one past the last site, sign)."""
    rng = np.random.default_rng(seed)
    planted, c4, i = [], [], 0
    for k, ln in enumerate(lens):
        sign = -1 if k % 4 == 3 else 1
        if k % 2:
            planted.append((i, i + ln, sign))
        for _ in range(ln):
            n1, n2 = rng.poisson(10, 2)
            f1, f2 = ((0.85, 0.15) if sign > 0 else (0.15, 0.85)) if k % 2 else (0.5, 0.5)
            m1, m2 = rng.binomial(n1, f1), rng.binomial(n2, f2)
            c4.append((m1, n1 - m1, m2, n2 - m2))
        i += ln
    pos = 1000 + np.cumsum(rng.integers(20, 120, i))
    cnt = np.zeros((i, 6), np.uint32)
    cnt[:, :4] = c4
    return pos.astype(np.uint32), cnt, planted


def test_noisy_regions_stay_whole():
    """What the model is for.  Planted regions of 40, 40 and 12 CpGs among 800
    flat ones: at the defaults the model returns one kept region per planted
    one, its edges at most one CpG off, and nothing else; the threshold rule
    cuts each 40-CpG region into several kept runs."""
    from tests.test_dmr_gpu import _dmr_ref
    pos, cnt, planted = planted_pile(4)
    h = hmm_ref(pos, cnt, CFG, HmmConfig())
    assert len(h["kept"]) == len(planted) == 3
    for r, (a, b, sign) in zip(h["kept"], planted):
        ia, ib = int(np.searchsorted(pos, r["start"])), int(np.searchsorted(pos, r["end"] - 1))
        assert abs(ia - a) <= 1 and abs(ib - (b - 1)) <= 1 and r["sign"] == sign
    t = [r for r in _dmr_ref(pos, cnt, CFG)["all"] if r["n_sites"] >= CFG.min_sites]
    for a, b, sign in planted[:2]:
        inside = [r for r in t if r["start"] >= pos[a] and r["end"] <= pos[b - 1] + 1]
        assert len(inside) > 1 and all(r["sign"] == sign for r in inside)
        assert sum(r["n_sites"] for r in inside) < b - a


def test_struct_layouts_match_header(tmp_path):
    from pomfret_amd.abi import PfDmr, PfDmrCfg, PfDmrHmm, PfDmrHmmCfg, PfDmrRun, PfHapmethHmm, PfHapmethHmmStats
    T, S = PfDmrHmm, PfHapmethHmmStats
    names = ["sizeof(pf_dmr_hmm_t)"] + ["offsetof(pf_dmr_hmm_t, %s)" % f for f, _ in T._fields_]
    names += ["sizeof(pf_dmr_hmm_cfg_t)", "sizeof(pf_hapmeth_hmm_t)", "sizeof(pf_hapmeth_hmm_stats_t)"]
    names += ["offsetof(pf_hapmeth_hmm_stats_t, %s)" % f for f, _ in S._fields_]
    names += ["sizeof(pf_dmr_t)", "sizeof(pf_dmr_cfg_t)", "sizeof(pf_dmr_run_t)", "PF_DMR_HMM_SITES", "PF_ABI_VERSION"]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\nint main(void){'
                   + "".join('printf("%%zu ", (size_t)%s);' % n for n in names) + 'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    from pomfret_amd.abi import DMR_HMM_SITES
    exp = [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    exp += [C.sizeof(PfDmrHmmCfg), C.sizeof(PfHapmethHmm), C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    exp += [C.sizeof(PfDmr), C.sizeof(PfDmrCfg), C.sizeof(PfDmrRun), DMR_HMM_SITES, 1]
    assert got == exp
    assert HmmConfig().to_c().site_cost_q16 == 131072 and HmmConfig().to_c().switch_q16 == 524288


def test_dmr_hmm_needs_dmr(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.abi import LoadConfig, PfDmrCfg, PfDmrHmmCfg, PfHapmethDmr, PfHapmethHmm, PfHapmethOpts
    from pomfret_amd.pipeline import _bind, hapmeth_files
    out = str(tmp_path / "o")
    with pytest.raises(PomfretError):
        hapmeth_files(str(tmp_path / "absent.bam"), out, dmr=None, dmr_hmm=HmmConfig())
    o = PfHapmethOpts(str(tmp_path / "absent.bam").encode(), out.encode(), None, 100000, 0, LoadConfig(min_len=0).to_c(), 1, 0, 0, 0)
    hm = PfHapmethHmm(HmmConfig().to_c())
    none = [None] * 6
    assert _bind().pf_hapmeth_run_hmm(C.byref(o), None, C.byref(hm), None, None, None, *none) == -1
    # a cost outside [0, 64] bits is an argument error before anything is opened
    d = PfHapmethDmr(PfDmrCfg(5, 40, 500, 5), 1.0, None)
    for bad in (PfDmrHmmCfg(-1, 0), PfDmrHmmCfg(0, 64 * 65536 + 1)):
        assert _bind().pf_hapmeth_run_hmm(C.byref(o), C.byref(d), C.byref(PfHapmethHmm(bad)), None, None, None, *none) == -1
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")


@pytest.mark.parametrize("args,word", [
    (["--dmr-hmm"], "--dmr-hmm needs --dmr"),
    (["--dmr", "--dmr-hmm-switch", "8"], "need --dmr-hmm"),
    (["--dmr", "--dmr-hmm-site-cost", "2"], "need --dmr-hmm"),
    (["--dmr-hmm-switch", "8"], "need --dmr-hmm"),
    (["--dmr", "--dmr-hmm", "--dmr-hmm-switch", "65"], "--dmr-hmm-switch"),
    (["--dmr", "--dmr-hmm", "--dmr-hmm-switch", "x"], "--dmr-hmm-switch"),
    (["--dmr", "--dmr-hmm", "--dmr-hmm-site-cost", "65"], "--dmr-hmm-site-cost"),
    (["--dmr", "--dmr-hmm", "--dmr-hmm-site-cost", "x"], "--dmr-hmm-site-cost"),
    (["--dmr", "--dmr-hmm", "--dmr-hmm-site-cost", "-0.5"], "--dmr-hmm-site-cost")])
def test_cli_option_errors(tmp_path, args, word):
    out = str(tmp_path / "o")
    r = subprocess.run([EXE, "hapmeth", "-o", out] + args + [str(tmp_path / "absent.bam")], capture_output=True, text=True)
    assert r.returncode == 1 and "[E::sancheck_cliopt_hapmeth]" in r.stderr and word in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed") and not os.path.exists(out + ".hapmeth.dmr.bed")


def test_cli_help_and_valid_line(tmp_path):
    r = subprocess.run([EXE, "hapmeth", "-h"], capture_output=True, text=True)
    assert r.returncode == 1
    for word in ("--dmr-hmm", "--dmr-hmm-site-cost", "--dmr-hmm-switch", "pooled difference", "not measured on real samples"):
        assert word in r.stderr, word
    # decimals and the two ends of the range are accepted: the line gets as far as the BAM and leaves no file
    out = str(tmp_path / "o")
    for cost, sw in (("1.5", "64"), ("0", "0")):
        r = subprocess.run([EXE, "hapmeth", "-o", out, "--dmr", "--dmr-hmm", "--dmr-hmm-site-cost", cost, "--dmr-hmm-switch", sw,
                            str(tmp_path / "absent.bam")], capture_output=True, text=True)
        assert r.returncode == 1 and "absent.bam" in r.stderr and "sancheck" not in r.stderr
    assert not os.path.exists(out + ".hapmeth.bed")
