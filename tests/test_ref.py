"""MD synthesis from a reference FASTA, host side (no GPU): pf_ref_open, the MD
rule (pf_md_synth_host) against the generators' own MD strings and a Python
transcription of the rule, pf_bam_set_ref, the rescue on a BAM without MD
tags, and the --ref plumbing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _bamio import Rec, aux_i, aux_Z, write_bam
from _mdcases import (HAND_REF_LEN, batch_of, build_read, hand_expected, hand_made, nib_of_text, pack_nib, past_end,
                      py_md, stripped, u_batch, write_fasta)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- pf_ref_open
def _contigs():
    rng = np.random.default_rng(5)
    a = bytes(rng.choice(np.frombuffer(b"ACGTacgtNRn-Uu", np.uint8), 1_003))
    b = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 61))
    return [("c1 a description, with\ttabs", a), ("empty", b""), ("c3", b), ("odd|name.2 x", b"ACGTN")]


@pytest.mark.parametrize("width,eol,gz,last_nl", [(60, "\n", False, True), (7, "\n", False, True),
                                                  (0, "\n", False, True), (60, "\r\n", False, True),
                                                  (60, "\n", True, True), (7, "\r\n", True, False),
                                                  (0, "\n", False, False)])
def test_ref_open_reads_the_fasta(tmp_path, width, eol, gz, last_nl):
    from pomfret_amd.bam import Reference
    ctg = _contigs()
    p = str(tmp_path / ("r.fa.gz" if gz else "r.fa"))
    write_fasta(p, ctg, width=width, eol=eol, gz=gz, last_newline=last_nl)
    with Reference.open(p) as r:
        assert r.names == [h.split()[0] for h, _ in ctg]
        for h, s in ctg:
            nib, n = r.contig(h.split()[0])
            assert n == len(s)
            assert np.array_equal(nib, pack_nib(nib_of_text(s)))
        with pytest.raises(Exception):
            r.contig("absent")


def test_ref_open_header_as_last_line(tmp_path):
    from pomfret_amd.bam import Reference
    p = str(tmp_path / "r.fa")
    with open(p, "wb") as f:
        f.write(b">a\nAC\n>tail and words")
    with Reference(p) as r:
        assert r.names == ["a", "tail"]
        assert r.contig("tail")[1] == 0


def test_ref_open_errors(tmp_path):
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import Reference
    p = str(tmp_path / "dup.fa")
    write_fasta(p, [("a x", b"ACGT"), ("b", b"AC"), ("a y", b"GG")])
    with pytest.raises(PomfretError):
        Reference(p)
    p = str(tmp_path / "early.fa")
    with open(p, "wb") as f:
        f.write(b"ACGT\n>a\nAC\n")
    with pytest.raises(PomfretError):
        Reference(p)
    with pytest.raises(FileNotFoundError):
        Reference(str(tmp_path / "absent.fa"))


# ------------------------------------------------------------ pf_md_synth_host
@pytest.mark.parametrize("hac", [False, True])
def test_md_synth_host_equals_the_generators_md(hac):
    from pomfret_amd.bam import md_synth_host
    _, reads, nib = u_batch(hac)
    off, md = md_synth_host(reads, pack_nib(nib), len(nib))
    assert np.array_equal(off, reads.md_off.astype(np.uint64))
    assert np.array_equal(md, reads.md)


def test_py_rule_equals_the_generators_md():
    """The Python transcription the hand-made set is checked against states
    the same rule as the generator's MD strings."""
    _, reads, nib = u_batch(True)
    for r in range(0, reads.n_reads, 7):
        cg = reads.cigar[int(reads.cigar_off[r]):int(reads.cigar_off[r + 1])]
        pk = reads.seq[int(reads.seq_off[r]):int(reads.seq_off[r + 1])]
        sq = np.stack([pk >> 4, pk & 15], 1).ravel()[:int(reads.seq_len[r])]
        exp = bytes(reads.md[int(reads.md_off[r]):int(reads.md_off[r + 1])])
        assert py_md(reads.start[r], cg, sq, nib) == exp


def test_md_synth_host_hand_made_set():
    from pomfret_amd.bam import md_synth_host
    ref, reads, exp_off, exp_md, mds = hand_expected()
    assert len(ref) == HAND_REF_LEN
    # the cases are what they claim to be
    import re
    assert [int(x) for x in re.findall(rb"\d+", mds[12])] == [99, 100, 9_999, 10_000, 5]
    assert [int(x) for x in re.findall(rb"\d+", mds[13])] == [0, 100_000, 0]
    assert sum(m.count(b"^") for m in mds) >= 10 and max(len(m) for m in mds) > 300
    assert b"N" in mds[11] and mds[17] == b"0"
    off, md = md_synth_host(reads, pack_nib(ref), len(ref))
    assert np.array_equal(off, exp_off)
    for i, m in enumerate(mds):
        assert bytes(md[int(off[i]):int(off[i + 1])]) == m, i
    assert np.array_equal(md, exp_md)


def test_md_synth_host_past_the_contig_end():
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import md_synth_host
    ref, _ = hand_made()
    with pytest.raises(PomfretError):
        md_synth_host(batch_of(past_end(ref)), pack_nib(ref), len(ref))
    # a deletion past the end as well
    rng = np.random.default_rng(1)
    with pytest.raises(PomfretError):
        md_synth_host(batch_of([build_read(rng, ref, len(ref) - 20, [(0, 10), (2, 11)])]), pack_nib(ref), len(ref))


# ------------------------------------------------------------- pf_bam_set_ref
def _tiny_bam(tmp_path, refs):
    p = str(tmp_path / "t.bam")
    write_bam(p, refs, [Rec(0, 10, "q", cigar=[4 << 4], seq=bytes([0x11, 0x11]), l_seq=4)])
    return p


def test_set_ref_checks_lengths(tmp_path):
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import Bam, Reference
    bam = _tiny_bam(tmp_path, [("c", 100), ("d", 50)])
    good, short, other = (str(tmp_path / n) for n in ("good.fa", "short.fa", "other.fa"))
    write_fasta(good, [("c", b"A" * 100), ("d", b"C" * 50)])
    write_fasta(short, [("c", b"A" * 99)])
    write_fasta(other, [("zzz", b"ACGT")])
    with Bam(bam) as b:
        with Reference(short) as r, pytest.raises(PomfretError):
            b.set_ref(r)
        with Reference(other) as r:
            b.set_ref(r)                       # an absent contig is accepted
            b.set_ref(None)
        with Reference(good) as r:
            b.set_ref(r)
            b.set_ref(None)


# --------------------------------------------------------------------- rescue
def _rescue_input(tmp_path):
    """A BAM with MD over a random reference, the same records without MD, the
    FASTA, and rescue arguments whose map is not trivial."""
    from pomfret_amd.abi import KnownVars
    rng = np.random.default_rng(8)
    L = 30_000
    ref = rng.choice(np.array([1, 2, 4, 8], np.uint8), L)
    kpos = sorted(set(int(x) for x in rng.integers(1_000, 20_000, 80)))
    recs, meth = [], {}
    for i in range(160):
        k = kpos[int(rng.integers(0, len(kpos)))]
        off = int(rng.integers(10, 550))                 # the read's variant sits on a known position,
        p = k - off
        if rng.random() < 0.25:                          # or near one
            off = int(rng.integers(10, 500))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            pos, cg, sq = build_read(rng, ref, p, [(0, 600)], mism=[off])
        elif kind == 1:
            pos, cg, sq = build_read(rng, ref, p, [(0, off), (2, 2), (0, 600 - off)])
        else:
            pos, cg, sq = build_read(rng, ref, p, [(4, 5), (0, off), (1, 3), (0, 597 - off)], mism=[off + 7])
        hp_tag = int(rng.integers(0, 3))
        aux = (aux_i("HP", hp_tag) if hp_tag else b"") + aux_Z("MD", py_md(pos, cg, sq, ref).decode()) + aux_i("NM", 1)
        recs.append(Rec(0, pos, f"q{i}", cigar=cg, seq=pack_nib(sq).tobytes(), l_seq=len(sq), aux=aux))
        if rng.random() < 0.8:
            meth[f"q{i}"] = int(rng.integers(0, 3))
    # records the rescue never selects: unmapped, and one without CIGAR
    recs.append(Rec(0, 3_000, "un", flag=4, seq=bytes([0x12]), l_seq=2, aux=aux_i("NM", 0)))
    recs.sort(key=lambda r: r.pos)
    tagged, bare, fa = (str(tmp_path / n) for n in ("tagged.bam", "bare.bam", "ref.fa"))
    write_bam(tagged, [("c", L)], recs)
    write_bam(bare, [("c", L)], stripped(recs))
    write_fasta(fa, [("c", bytes(b"=ACMGRSVTWYHKDBN"[int(v)] for v in ref))])
    kn = KnownVars(pos=np.array(kpos), len=np.ones(len(kpos)), op=np.ones(len(kpos)),
                   haptag=np.zeros(len(kpos)), char_off=np.arange(len(kpos) + 1), chars=np.zeros(len(kpos)))
    dropped = [(1_200, 4_000), (6_000, 9_000), (12_000, 18_000)]
    return tagged, bare, fa, kn, dropped, meth


def test_rescue_on_a_bam_without_md(tmp_path):
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import BamFile, Reference, rescue_dropped
    tagged, bare, fa, kn, dropped, meth = _rescue_input(tmp_path)
    with BamFile(tagged) as b:
        exp = rescue_dropped(b, "c", dropped, kn, meth)
    assert len(exp) > 5 and any(v != 254 for v in exp.values())
    with BamFile(bare) as b:
        with pytest.raises(PomfretError):
            rescue_dropped(b, "c", dropped, kn, meth)
        with Reference(fa) as r:
            b.set_ref(r)
            assert rescue_dropped(b, "c", dropped, kn, meth) == exp
            assert rescue_dropped(b, "c", dropped, kn, meth, threads=3) == exp
            b.set_ref(None)
        with pytest.raises(PomfretError):
            rescue_dropped(b, "c", dropped, kn, meth)
    # the tagged BAM with the reference: the synthesised MD replaces an agreeing tag
    with BamFile(tagged) as b, Reference(fa) as r:
        b.set_ref(r)
        assert rescue_dropped(b, "c", dropped, kn, meth) == exp


def test_fetch_contig_reads_synthesises_md(tmp_path):
    """The --host-fetch pre-pass's reads (push_read): the stripped BAM with the
    reference gives the tagged BAM's batch, MD included; without it PF_ERR_ARG."""
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import BamFile, Reference
    tagged, bare, fa, *_ = _rescue_input(tmp_path)
    with BamFile(tagged) as b:
        exp, exp_q, _ = b.fetch_contig_reads("c")
    with BamFile(bare) as b:
        with pytest.raises(PomfretError):
            b.fetch_contig_reads("c")
        with Reference(fa) as r:
            b.set_ref(r)
            got, got_q, _ = b.fetch_contig_reads("c")
    assert got_q == exp_q and got.n_reads == exp.n_reads > 100
    for f in ("start", "end", "cigar_off", "cigar", "seq_off", "seq_len", "seq", "md_off", "md"):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), f


# ------------------------------------------------------------------- plumbing
def test_make_opts_carries_the_reference():
    from pomfret_amd.pipeline import make_opts
    assert make_opts("a.bam", "a.vcf", None, None).ref_path is None
    assert make_opts("a.bam", "a.vcf", None, None, ref="r.fa").ref_path == b"r.fa"


def test_opts_ref_field_matches_header(tmp_path):
    from pomfret_amd.pipeline import PfMethphaseOpts
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pomfret_amd.h"\n'
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(pf_methphase_opts_t),'
                   'offsetof(pf_methphase_opts_t, mask_variants), offsetof(pf_methphase_opts_t, ref_path));'
                   'return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(PfMethphaseOpts), PfMethphaseOpts.mask_variants.offset, PfMethphaseOpts.ref_path.offset]
    assert PfMethphaseOpts.ref_path.offset > PfMethphaseOpts.mask_variants.offset


@pytest.mark.parametrize("sub", ["methphase", "report", "varhaptag"])
def test_cli_refuses_an_unreadable_ref(tmp_path, sub):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    vcf, bam = str(tmp_path / "a.vcf"), str(tmp_path / "absent.bam")
    open(vcf, "w").write("##fileformat=VCFv4.2\n")
    ref = str(tmp_path / "absent.fa")
    if sub == "varhaptag":
        args = [sub, "-o", str(tmp_path / "o.bam"), "--ref", ref, vcf, bam]
    else:
        args = [sub, "-o", str(tmp_path / "o"), "--vcf", vcf, "--ref", ref, bam]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--ref" in r.stderr and "absent.fa" in r.stderr
