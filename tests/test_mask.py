"""CPU tests of the site mask's host side: pf_mask_load (BED intervals and the
phased variants' [pos, pos+len), the masked_poss sets of main_methreport,
blockjoin.c:5006-5029), the two new pf_methphase_opts_t fields and the CLI's
--mask-bed / --mask-variants checks.  No GPU."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_VCF = os.path.join(ROOT, "tests", "golden", "example", "variants.vcf.gz")

BED = ("# a comment line\n"
       "chrA\t100\t110\n"
       "chrB\t5\t8\n"
       "chrA\t105\t120\n"          # overlaps the first
       "chrA\t50\t52\n"            # unsorted
       "chrA\t50\t52\n"            # duplicate
       "chrZ\t1\t1000\n"           # a contig the run does not have
       "chrA\t70\t70\n"            # empty
       "chrA\t90\t80\n"            # end < start: empty
       "\n"
       "chrB\t7\t9\n"
       "chrA\t120\t121\n")         # adjacent to a merged interval
EXPECT = {"chrA": [50, 51] + list(range(100, 121)), "chrB": [5, 6, 7, 8], "chrC": []}


def _expect(names):
    return [np.array(EXPECT[n], np.uint32) for n in names]


def test_bed_mask_sorted_unique_per_contig(tmp_path):
    from pomfret_amd.pipeline import load_mask
    names = ["chrB", "chrA", "chrC"]
    plain = tmp_path / "m.bed"
    plain.write_text(BED)
    gz = tmp_path / "m.bed.gz"
    with gzip.open(gz, "wt") as f:
        f.write(BED)
    for path in (plain, gz):
        got = load_mask(names, bed_path=str(path))
        assert len(got) == 3
        for g, e in zip(got, _expect(names)):
            assert g.dtype == np.uint32 and np.array_equal(g, e)
    # no file at all: empty masks
    assert all(g.size == 0 for g in load_mask(names))


def test_bed_mask_errors(tmp_path):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import _bind, load_mask
    L = _bind()
    names = ["chrA"]

    def rc_of(text):
        p = tmp_path / "e.bed"
        p.write_text(text)
        arr = (C.c_char_p * 1)(b"chrA")
        h = C.c_void_p()
        rc = L.pf_mask_load(str(p).encode(), None, 1, arr, C.byref(h))
        if rc == 0:
            L.pf_mask_free(h)
        return rc

    PF_ERR_ARG, PF_ERR_LIMIT = -1, -5
    lim = 1 << 29
    assert rc_of(f"chrA\t{lim - 1}\t{lim}\n") == 0                 # the last allowed position
    assert rc_of(f"chrA\t{lim - 1}\t{lim + 1}\n") == PF_ERR_LIMIT   # position 2^29
    assert rc_of(f"chrA\t{lim}\t{lim + 5}\n") == PF_ERR_LIMIT
    assert rc_of(f"chrQ\t{lim}\t{lim + 5}\n") == 0                  # ignored with its contig
    assert rc_of("chrA\t10\n") == PF_ERR_ARG
    assert rc_of("chrA\tten\t20\n") == PF_ERR_ARG
    with pytest.raises(PomfretError):
        load_mask(names, bed_path=str(tmp_path / "missing.bed"))


def _py_variant_union(vcf, names):
    """[pos, pos+len) of every entry of the known tables the package exposes."""
    from pomfret_amd.bam import vcf_known_vars_multi
    out = []
    for kv in vcf_known_vars_multi(vcf, names):
        s = set()
        for p, ln in zip(np.asarray(kv.pos).tolist(), np.asarray(kv.len).tolist()):
            s.update(range(p, p + ln))
        out.append(s)
    return out


def test_vcf_mask_is_the_known_tables_union(tmp_path):
    import oracle
    from pomfret_amd.pipeline import load_mask
    names = [c["name"] for c in oracle.vcf_gaps(GOLD_VCF)]
    assert names
    want = _py_variant_union(GOLD_VCF, names)
    assert sum(len(s) for s in want) > 0
    got = load_mask(names, vcf_path=GOLD_VCF)
    for g, s in zip(got, want):
        assert np.array_equal(g, np.array(sorted(s), np.uint32))
    # indels (len > 1) on a hand-written VCF, worked by hand from the table's
    # rules: SNP -> POS-1; deletion -> POS, len ref-alt; insertion -> POS-1,
    # len alt-ref; an unphased line gives nothing
    hv = tmp_path / "h.vcf"
    row = "{c}\t{p}\t.\t{r}\t{a}\t50\tPASS\t.\tGT:PS\t{g}:1\n"
    hv.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
                  + row.format(c="c1", p=5, r="A", a="C", g="0|1")
                  + row.format(c="c1", p=10, r="ACGT", a="A", g="1|0")
                  + row.format(c="c1", p=12, r="G", a="T", g="0|1")          # inside the deletion
                  + row.format(c="c1", p=20, r="A", a="ACC", g="0|1")
                  + row.format(c="c1", p=30, r="A", a="C", g="0/1")
                  + row.format(c="c2", p=7, r="T", a="G", g="1|0"))
    hm = load_mask(["c2", "c1"], vcf_path=str(hv))
    assert hm[0].tolist() == [6] and hm[1].tolist() == [4, 10, 11, 12, 19, 20]
    assert [sorted(s) for s in _py_variant_union(str(hv), ["c2", "c1"])] == [[6], [4, 10, 11, 12, 19, 20]]
    # with a BED added: the union of both; an unknown contig in `names` stays empty
    first = sorted(want[0])
    bed = tmp_path / "v.bed"
    bed.write_text(f"{names[0]}\t{first[0]}\t{first[0] + 3}\n{names[0]}\t7\t9\nother\t1\t5\n")
    got2 = load_mask(names + ["nope"], bed_path=str(bed), vcf_path=GOLD_VCF)
    u = set(want[0]) | set(range(first[0], first[0] + 3)) | {7, 8}
    assert np.array_equal(got2[0], np.array(sorted(u), np.uint32))
    for g, s in zip(got2[1:len(names)], want[1:]):
        assert np.array_equal(g, np.array(sorted(s), np.uint32))
    assert got2[-1].size == 0


def test_opts_layout_matches_header(tmp_path):
    """ctypes PfMethphaseOpts against the C compiler's sizeof / offsetof of
    the fields appended after bam_threads."""
    from pomfret_amd.pipeline import PfMethphaseOpts
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(pf_methphase_opts_t),'
                   'offsetof(pf_methphase_opts_t, bam_threads), offsetof(pf_methphase_opts_t, mask_path),'
                   'offsetof(pf_methphase_opts_t, mask_variants));return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    exp = [C.sizeof(PfMethphaseOpts), PfMethphaseOpts.bam_threads.offset, PfMethphaseOpts.mask_path.offset,
           PfMethphaseOpts.mask_variants.offset]
    assert got == exp
    assert PfMethphaseOpts.mask_path.offset > PfMethphaseOpts.bam_threads.offset


def test_make_opts_carries_the_mask(tmp_path):
    from pomfret_amd.pipeline import make_opts
    o = make_opts("a.bam", "a.vcf", None, None)
    assert o.mask_path is None and o.mask_variants == 0
    o = make_opts("a.bam", "a.vcf", None, None, mask_bed="m.bed", mask_variants=True)
    assert o.mask_path == b"m.bed" and o.mask_variants == 1


def _cli(*args):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("sub", ["methphase", "report"])
def test_cli_mask_option_checks(tmp_path, sub):
    """Both are refused by the option check, before the BAM is opened or a
    device is asked for (the BAM named here does not exist)."""
    bam = str(tmp_path / "absent.bam")
    tsv = tmp_path / "blocks.tsv"
    tsv.write_text("chrA\t100\t200\n")
    if sub == "methphase":
        r = _cli(sub, "-o", str(tmp_path / "o"), "--tsv", str(tsv), "--mask-variants", bam)
    else:
        r = _cli(sub, "-o", str(tmp_path / "o"), "--mask-variants", bam)
    assert r.returncode != 0
    assert "--mask-variants" in r.stderr or "vcf" in r.stderr
    r = _cli(sub, "-o", str(tmp_path / "o"), "--vcf", GOLD_VCF, "--mask-bed", str(tmp_path / "absent.bed"), bam)
    assert r.returncode != 0
    assert "--mask-bed" in r.stderr
    assert "HIP" not in r.stderr
    r = _cli(sub, "--help")
    assert "--mask-bed" in r.stderr and "--mask-variants" in r.stderr


def test_plan_refuses_a_bad_mask_before_the_bam(tmp_path):
    """pf_mp_plan: mask_variants without a VCF is an argument error; an
    unreadable BED fails the plan (the BAM here is a real file the plan would
    otherwise open)."""
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import INTERVALS_TSV, Plan, make_opts
    tsv = tmp_path / "blocks.tsv"
    tsv.write_text("chrA\t100\t200\nchrA\t300000\t400000\n")
    with pytest.raises(PomfretError):
        Plan(make_opts(str(tmp_path / "x.bam"), None, None, None, intervals=(str(tsv), INTERVALS_TSV),
                       mask_variants=True))
    with pytest.raises(PomfretError):
        Plan(make_opts(str(tmp_path / "x.bam"), None, None, None, intervals=(str(tsv), INTERVALS_TSV),
                       mask_bed=str(tmp_path / "absent.bed")))
