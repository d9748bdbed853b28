"""`hapmeth --tile` end to end on the device: pf_hapmeth_run_tiles
(hapmeth_files, the CLI) over a haplotagged fixture BAM, against text built on
the CPU: the host fetch with the tiles as the windows, the oracle's loader, the
literal rank reference (tests/_rank_ref.py), pomfret_amd.rank_p and the Python
Benjamini-Hochberg loop (tests/test_ranktiles.tiles_text).  Every comparison is
on bytes.

The fixture is test_hapmeth_rank_gpu.py's BAM (coverage 12, two windows 600 kb
apart, so there are tiles without a read and fetch windows without a chunk);
the span is 826,921 bases.  The reference gives, and the fixture asserts:

       T  min_calls  tiles  with a participating read  tested  status 1  distinct rank_p
    1000          1    827                        315     263        52              230
    1000          3    827                        315     261        54              228
    5000          1    166                         66      57         9               55
    5000          3    166                         66      56        10               54

with at most 22 counted reads in a tile at T = 1000 and 30 at T = 5000 (min_calls 1).
"""
import os
import subprocess

import pytest

from pomfret_amd.abi import DmrConfig

from tests import _fixtures as fx
from tests._rank_ref import bh_ref, rank_ref_batch
from tests.test_hapmeth_dmr_gpu import LCFG
from tests.test_ranktiles import THEAD, tiles_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = 826_921
# (T, min_calls) -> tiles, with a participating read, tested, status 1, distinct rank_p
TABLE = {(1000, 1): (827, 315, 263, 52, 230), (1000, 3): (827, 315, 261, 54, 228),
         (5000, 1): (166, 66, 57, 9, 55), (5000, 3): (166, 66, 56, 10, 54)}
MOST = {1000: 22, 5000: 30}                      # the most counted reads in a tile, min_calls 1


def _tiles(lo, hi, T):
    return [(s, min(s + T, hi)) for s in range(lo, hi, T)]


def _records(ref, tiles, breaks=()):
    """The records of the tile file: the tiles with a participating read, split by a break strictly inside."""
    out = []
    for w, (s, e) in enumerate(tiles):
        if not (ref["n_reads"][w] + ref["n_short"][w]).any():
            continue
        out.append(dict({k: ref[k][w].tolist() for k in ("n_reads", "n_short", "cls", "sum")}, u2=int(ref["u2"][w]),
                        ties=int(ref["ties"][w]), status=int(ref["status"][w]), chrom="chrS", start=s, end=e,
                        split=any(s < x < e for x in breaks)))
    return out


def _figures(n_tiles, recs):
    from pomfret_amd import rank_p
    tested = [r for r in recs if r["status"] == 0]
    ps = {"%.6g" % rank_p(r["u2"], r["n_reads"][0], r["n_reads"][1], r["ties"])[2] for r in tested}
    return n_tiles, len(recs), len(tested), len([r for r in recs if r["status"] == 1]), len(ps)


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle_lib):
    from pomfret_amd.bam import BamFile
    tmp = tmp_path_factory.mktemp("hapmeth_tiles")
    aln, recs, bam, vcf = fx.tagged(tmp, n_windows=2, coverage=12, len_scale=0.3)
    lo = int(aln.pos.min())
    hi = int(aln.pos.max()) + 60_000             # past every read's end (reads <= 150 kb * 0.3)
    assert hi - lo == SPAN
    refs, tiles = {}, {}
    with BamFile(bam) as bf:
        for T in (1000, 5000):
            tiles[T] = _tiles(lo, hi, T)
            per, _, _ = bf.fetch_windows("chrS", [s for s, _ in tiles[T]], [e for _, e in tiles[T]], readback=0)
            pb, _ = oracle_lib.load_reads(LCFG, per)
            for mc in (1, 3):
                refs[(T, mc)] = rank_ref_batch(pb, mc)
    rec = {key: _records(refs[key], tiles[key[0]]) for key in TABLE}
    for key, exp in TABLE.items():
        assert _figures(len(tiles[key[0]]), rec[key]) == exp, (key, _figures(len(tiles[key[0]]), rec[key]))
    for T, most in MOST.items():
        assert max(sum(r["n_reads"]) for r in rec[(T, 1)]) == most
    return dict(tmp=tmp, bam=bam, region=f"chrS:{lo + 1}-{hi}", lo=lo, hi=hi, refs=refs, tiles=tiles, rec=rec,
                text={key: tiles_text(rec[key]) for key in TABLE})


def _run(case, name, T=1000, min_calls=3, **kw):
    from pomfret_amd.pipeline import hapmeth_files
    res = hapmeth_files(case["bam"], str(case["tmp"] / name), region=case["region"], tile=T, tile_min_calls=min_calls, **kw)
    assert res["tiles_path"] == str(case["tmp"] / name) + ".hapmeth.tiles.tsv"
    return res, open(res["tiles_path"]).read()


@pytest.mark.parametrize("T,min_calls", sorted(TABLE))
def test_file_equals_cpu_text(case, T, min_calls):
    res, text = _run(case, f"a{T}_{min_calls}", T, min_calls)
    assert text == case["text"][(T, min_calls)] and text.startswith(THEAD)
    n, written, tested = TABLE[(T, min_calls)][:3]
    assert (res["n_tiles"], res["tiles_written"], res["tiles_tested"], res["tiles_split"]) == (n, written, tested, 0)
    assert res["tiles_ms_kernels"] > 0
    assert "dmr_path" not in res and not os.path.exists(str(case["tmp"] / f"a{T}_{min_calls}") + ".hapmeth.dmr.bed")


@pytest.mark.parametrize("T,chunk", [(1000, 1000), (1000, 5000), (5000, 5000), (5000, 25_000)])
def test_chunk_size_same_bytes(case, T, chunk):
    """A tile lies in one fetch window whatever the chunk size (the default, 100,000, is the run above)."""
    _, text = _run(case, f"c{T}_{chunk}", T, 3, chunk_size=chunk)
    assert text == case["text"][(T, 3)]


@pytest.mark.parametrize("jw", [1, 3])
def test_job_size_same_bytes(case, jw):
    _, text = _run(case, f"j{jw}", 1000, 1, job_windows=jw)
    assert text == case["text"][(1000, 1)]


def test_host_fetch_same_bytes(case):
    _, text = _run(case, "h", 1000, 3, host_fetch=True, threads=2)
    assert text == case["text"][(1000, 3)]


def test_cli_same_bytes(case):
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "cli")
    r = subprocess.run([exe, "hapmeth", "-v", "-o", out, "-r", case["region"], "--tile", "5000", "--tile-min-calls", "1",
                        case["bam"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.tiles.tsv").read() == case["text"][(5000, 1)]
    assert "tiles of 5000 bases: 166 planned, 66 with a read written, 57 tested (at least 1 calls a read), 0 split" in r.stderr
    assert "66 tiles written to %s.hapmeth.tiles.tsv, 57 of them with a rank-sum p-value" % out in r.stderr
    # the default of --tile-min-calls is 3
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--tile", "5000", case["bam"]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.tiles.tsv").read() == case["text"][(5000, 3)]


def test_bad_tile_and_chunk_sizes(case):
    from pomfret_amd import PomfretError
    from pomfret_amd.pipeline import hapmeth_files
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "bad")
    with pytest.raises(PomfretError, match="multiple"):
        hapmeth_files(case["bam"], out, region=case["region"], tile=1000, chunk_size=1500)
    for bad in (dict(tile=50), dict(tile=99), dict(tile=200_000), dict(tile=1000, tile_min_calls=0),
                dict(tile=1000, tile_min_calls=65536)):
        with pytest.raises(PomfretError):
            hapmeth_files(case["bam"], out, region=case["region"], **bad)
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--tile", "1000", "--chunk-size", "1500", case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "multiple" in r.stderr
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--tile", "50", case["bam"]], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--tile" in r.stderr
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--tile-min-calls", "2", case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "needs --tile" in r.stderr
    for ext in ("bed", "tiles.tsv"):
        assert not os.path.exists(out + ".hapmeth." + ext)


def test_phase_blocks(case):
    """A block boundary strictly inside one tested tile (split: counted, '.'
    in the four test columns, left out of rank_q) and exactly on the edge of
    another (ok)."""
    from pomfret_amd import rank_p
    recs = case["rec"][(1000, 3)]
    tested = [r for r in recs if r["status"] == 0]
    a, b = tested[3], tested[40]
    assert a["end"] < b["start"]
    gap = (a["start"] + 400, b["start"] + 1)     # the blocks (.., s] and [e, ..] 1-based: breaks at s and e - 1
    gtf, _ = fx.blocks_files(case["tmp"], {"chrS": [gap]})
    breaks = sorted({max(1, gap[0] - 100_000) - 1, gap[0], gap[1] - 1, gap[1] + 100_000})
    assert a["start"] < breaks[1] < a["end"] and breaks[2] == b["start"]
    exp_recs = _records(case["refs"][(1000, 3)], case["tiles"][1000], breaks)
    exp = tiles_text(exp_recs)
    res, text = _run(case, "blocks", 1000, 3, dmr_blocks=gtf)
    assert text == exp and text != case["text"][(1000, 3)]
    rows = {(int(x[1]), int(x[2])): x for x in (ln.split("\t") for ln in text.splitlines()[1:])}
    ra, rb = rows[(a["start"], a["end"])], rows[(b["start"], b["end"])]
    assert ra[22] == "split" and ra[13:17] == ["."] * 4 and [int(v) for v in ra[3:5]] == a["n_reads"]
    assert rb[22] == "ok" and rb[15] != "."
    n_split = sum(r["split"] for r in exp_recs)
    assert res["tiles_split"] == n_split >= 1 and res["tiles_tested"] == sum(r["status"] == 0 and not r["split"] for r in exp_recs)
    # rank_q over the rest
    keep = [r["status"] == 0 and not r["split"] for r in exp_recs]
    p = [rank_p(r["u2"], r["n_reads"][0], r["n_reads"][1], r["ties"])[2] if t else 1.0 for r, t in zip(exp_recs, keep)]
    col = [ln.split("\t")[16] for ln in text.splitlines()[1:]]
    assert col == ["%.6g" % v if t else "." for v, t in zip(bh_ref(p, keep), keep)]
    # the same blocks through the CLI, --dmr-blocks with --tile alone
    exe = os.path.join(ROOT, "pomfret_amd", "pomfret-amd")
    out = str(case["tmp"] / "blocks_cli")
    r = subprocess.run([exe, "hapmeth", "-o", out, "-r", case["region"], "--tile", "1000", "--dmr-blocks", gtf, case["bam"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out + ".hapmeth.tiles.tsv").read() == exp


def test_other_files_keep_their_bytes(case):
    from pomfret_amd.pipeline import hapmeth_files
    cfg = DmrConfig(min_cov=3, min_delta_pct=30, max_gap=1000, min_sites=2)
    plain = hapmeth_files(case["bam"], str(case["tmp"] / "plain"), region=case["region"])
    assert "tiles_path" not in plain and not os.path.exists(str(case["tmp"] / "plain") + ".hapmeth.tiles.tsv")
    res, text = _run(case, "with", 1000, 3)
    assert open(plain["path"], "rb").read() == open(res["path"], "rb").read()
    both = hapmeth_files(case["bam"], str(case["tmp"] / "both"), region=case["region"], dmr=cfg, dmr_rank=True)
    res3, text3 = _run(case, "all", 1000, 3, dmr=cfg, dmr_rank=True)
    assert text3 == text == case["text"][(1000, 3)]
    for k in ("path", "dmr_path", "rank_path"):
        assert open(both[k], "rb").read() == open(res3[k], "rb").read(), k
    assert res3["n_regions"] == both["n_regions"] > 0 and res3["rank_tested"] == both["rank_tested"]


def test_against_the_given_regions_pass(case):
    """The written tiles as a --regions BED through the second pass and
    pf_batch_ranktest: every line of that rank file has the tile file's
    reads_h1 .. rank_p; rank_q differs, the sets differ."""
    from pomfret_amd.pipeline import hapmeth_files
    _, text = _run(case, "x", 5000, 3)
    rows = [ln.split("\t") for ln in text.splitlines()[1:]]
    bed = str(case["tmp"] / "tiles.bed")
    with open(bed, "w") as f:
        f.write("".join("%s\t%s\t%s\n" % (x[0], x[1], x[2]) for x in rows))
    res = hapmeth_files(case["bam"], str(case["tmp"] / "xr"), region=case["region"], regions=bed, dmr_rank=True,
                        dmr_rank_min_calls=3, dmr_max_p=1.0, dmr=DmrConfig(min_sites=1))
    by = {(x[0], x[1], x[2]): x for x in rows}
    got = [ln.split("\t") for ln in open(res["rank_path"]).read().splitlines()[1:]]
    assert len(got) > 20
    for x in got:
        assert by[(x[0], x[1], x[2])][3:16] == x[3:16], x[:3]
