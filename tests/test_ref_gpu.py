"""MD synthesis on the device (pf_k4_mdlen / pf_k4_mdfill): the kernels against
the host rule and the generators' MD, K4 on the synthesised MD, the -u
pre-pass of a BAM without MD tags through the device fetch, and whole runs
with --ref against the runs on the tagged BAM.  Every comparison is
byte-exact."""
import os
import subprocess

import numpy as np
import pytest

from _bamio import write_bam
from _mdcases import batch_of, hand_expected, hand_made, pack_nib, past_end, stripped, u_batch, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def u_batches():
    return {hac: u_batch(hac) for hac in (False, True)}


@pytest.mark.parametrize("hac", [False, True], ids=["sup", "hac"])
def test_md_synth_equals_host_and_generator(gpu_ctx, u_batches, hac):
    from pomfret_amd.bam import md_synth, md_synth_host
    _, reads, nib = u_batches[hac]
    pk = pack_nib(nib)
    off, md = md_synth(gpu_ctx, reads, pk, len(nib))
    h_off, h_md = md_synth_host(reads, pk, len(nib))
    assert np.array_equal(off, h_off) and np.array_equal(md, h_md)
    assert np.array_equal(off, reads.md_off.astype(np.uint64)) and np.array_equal(md, reads.md)


def test_md_synth_hand_made_set(gpu_ctx):
    from pomfret_amd.bam import md_stats, md_synth, md_synth_host
    ref, reads, exp_off, exp_md, mds = hand_expected()
    pk = pack_nib(ref)
    before = md_stats(gpu_ctx)
    off, md = md_synth(gpu_ctx, reads, pk, len(ref))
    assert np.array_equal(off, exp_off)
    for i, m in enumerate(mds):
        assert bytes(md[int(off[i]):int(off[i + 1])]) == m, i
    assert np.array_equal(md, exp_md)
    h_off, h_md = md_synth_host(reads, pk, len(ref))
    assert np.array_equal(off, h_off) and np.array_equal(md, h_md)
    after = md_stats(gpu_ctx)
    assert after["n_reads"] - before["n_reads"] == reads.n_reads
    assert after["md_bytes"] - before["md_bytes"] == len(exp_md)


def test_md_synth_past_the_contig_end(gpu_ctx):
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import md_synth
    ref, R = hand_made()
    with pytest.raises(PomfretError):
        md_synth(gpu_ctx, batch_of(R[:3] + past_end(ref) + R[3:5]), pack_nib(ref), len(ref))


@pytest.mark.parametrize("hac", [False, True], ids=["sup", "hac"])
def test_haptag_reads_ref(oracle_lib, gpu_ctx, u_batches, hac):
    from pomfret_amd.abi import ReadAlnBatch
    from pomfret_amd.bam import haptag_reads_ref
    known, reads, nib = u_batches[hac]
    exp = gpu_ctx.haptag_reads(known, reads)
    # the reads without their MD: the synthesised one is all K4 sees
    bare = ReadAlnBatch(start=reads.start, end=reads.end, cigar_off=reads.cigar_off, cigar=reads.cigar,
                        seq_off=reads.seq_off, seq_len=reads.seq_len, seq=reads.seq,
                        md_off=np.zeros(reads.n_reads + 1), md=np.zeros(0, np.uint8))
    got = haptag_reads_ref(gpu_ctx, known, bare, pack_nib(nib), len(nib))
    assert np.array_equal(got, exp)
    assert np.array_equal(got, oracle_lib.haptag_reads(known, reads))
    assert (got < 2).mean() > 0.5


# ---------------------------------------------------------------- a stripped BAM
def ref_spec():
    from _genome import GenomeSpec
    from pomfret_amd.synth_aln import AlnSpec
    return GenomeSpec(contigs=(("chrR", 300_000),), coverage=20, block_min=52_000, block_max=64_000,
                      short_block_frac=0.25, gap_min=5_000, gap_max=15_000, lead=15_000, seed=43, qual=False, level=1,
                      chunk_reads=200,
                      aln=AlnSpec(het_snv_rate=0.001, untag_frac=0.0, mean_len=15_000, sd_len=7_500,
                                  min_len=7_500, max_len=60_000))


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """The tagged BAM + VCF, the same records without MD, and the FASTA."""
    from _genome import contig_layout, write_genome
    d = tmp_path_factory.mktemp("refg")
    spec = ref_spec()
    g = write_genome(str(d / "g"), spec, workers=4, keep_recs=True)
    recs = g["recs_by_contig"]["chrR"]
    assert all(b"MDZ" in r.aux for r in recs)
    bare = str(d / "bare.bam")
    write_bam(bare, g["refs"], stripped(recs), level=1)
    fa = str(d / "ref.fa")
    write_fasta(fa, [("chrR test genome", bytes(b"ACGT"[int(c)] for c in contig_layout(spec, 0)["ref"]))])
    return dict(bam=g["bam"], vcf=g["vcf"], bare=bare, fa=fa, n=len(recs))


def test_haptag_bam_on_a_stripped_bam(gpu_ctx, genome):
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.bam import BamFile, Reference, md_stats, vcf_known_vars
    known = vcf_known_vars(genome["vcf"], "chrR")
    with BamFile(genome["bam"]) as b:
        exp_hp, exp_q, _ = b.haptag_device(gpu_ctx, "chrR", known)
    assert len(exp_q) > 300 and (exp_hp < 2).sum() > 100
    with BamFile(genome["bare"]) as b:
        with pytest.raises(PomfretError):
            b.haptag_device(gpu_ctx, "chrR", known)
        with Reference(genome["fa"]) as r:
            b.set_ref(r)
            up0 = md_stats(gpu_ctx)["ref_upload_bytes"]
            for bounds in (None, [100_000, 200_000]):
                hp, q, _ = b.haptag_device(gpu_ctx, "chrR", known, bounds=bounds)
                assert q == exp_q and np.array_equal(hp, exp_hp), bounds
            # one upload of the contig's nibbles for the three pieces and both calls
            assert md_stats(gpu_ctx)["ref_upload_bytes"] - up0 == 150_000
            b.set_ref(None)
        with pytest.raises(PomfretError):
            b.haptag_device(gpu_ctx, "chrR", known)


def _outputs(prefix):
    return (open(prefix + ".mp.gtf").read(), open(prefix + ".mp.tsv").read(), open(prefix + ".mp.vcf", "rb").read())


@pytest.fixture(scope="module")
def tagged_run(gpu_ctx, genome, tmp_path_factory):
    from pomfret_amd import Config
    from pomfret_amd.pipeline import methphase_files
    out = str(tmp_path_factory.mktemp("refrun") / "t")
    res = methphase_files(genome["bam"], genome["vcf"], out, Config.from_coverage(20, given=True), ctx=gpu_ctx,
                          untagged=True, tsv=True)
    assert len(res["decision"]) >= 2 and len(res["raw_hp"]) > 300      # windows to decide, reads tagged by K4
    return res, _outputs(out)


@pytest.mark.parametrize("host_fetch", [False, True], ids=["device", "host_fetch"])
def test_methphase_with_ref_on_a_stripped_bam(gpu_ctx, genome, tagged_run, tmp_path, host_fetch):
    from pomfret_amd import Config
    from pomfret_amd._lib import PomfretError
    from pomfret_amd.pipeline import methphase_files
    exp, exp_files = tagged_run
    cfg = Config.from_coverage(20, given=True)
    out = str(tmp_path / "s")
    res = methphase_files(genome["bare"], genome["vcf"], out, cfg, ctx=gpu_ctx, untagged=True, tsv=True,
                          host_fetch=host_fetch, ref=genome["fa"])
    assert np.array_equal(res["decision"], exp["decision"])
    assert res["qname_hp"] == exp["qname_hp"] and list(res["qname_hp"]) == list(exp["qname_hp"])
    assert res["raw_hp"] == exp["raw_hp"]
    assert _outputs(out) == exp_files
    with pytest.raises(PomfretError):
        methphase_files(genome["bare"], genome["vcf"], str(tmp_path / "n"), cfg, ctx=gpu_ctx, untagged=True,
                        tsv=True, host_fetch=host_fetch)


def test_methphase_with_ref_on_the_tagged_bam(gpu_ctx, genome, tagged_run, tmp_path):
    """The synthesised MD replaces an agreeing tag without effect."""
    from pomfret_amd import Config
    from pomfret_amd.pipeline import methphase_files
    exp, exp_files = tagged_run
    out = str(tmp_path / "tr")
    res = methphase_files(genome["bam"], genome["vcf"], out, Config.from_coverage(20, given=True), ctx=gpu_ctx,
                          untagged=True, tsv=True, ref=genome["fa"])
    assert np.array_equal(res["decision"], exp["decision"])
    assert res["qname_hp"] == exp["qname_hp"] and res["raw_hp"] == exp["raw_hp"]
    assert _outputs(out) == exp_files


def test_cli_methphase_with_ref(genome, tagged_run, tmp_path):
    _, exp_files = tagged_run
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(tmp_path / "c")
    r = subprocess.run([exe, "methphase", "-u", "--ref", genome["fa"], "-c", "20", "-o", out, "--vcf", genome["vcf"],
                        "--output-tsv", genome["bare"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert _outputs(out) == exp_files
