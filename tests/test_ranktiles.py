"""The tile file of `hapmeth --tile` on the host (pf_write_rank_tiles): the 17
columns of the rank file from tests/_rank_ref.rank_text's pieces, then the
counted reads' calls, delta and block, all against text built here; rank_q
against the Python Benjamini-Hochberg loop over the records that are tested and
not split.  No GPU."""
import os

import numpy as np
import pytest

from tests._rank_ref import HEAD, bh_ref, rank_ref

THEAD = HEAD[:-1] + "\th1_meth\th1_unmeth\th2_meth\th2_unmeth\tdelta\tblock\n"


def tiles_text(recs):
    """{prefix}.hapmeth.tiles.tsv from records (chrom, start, end, rank_ref's
    dict with its sum, and split): the p-values by pomfret_amd.rank_p, the
    q-values by bh_ref over the status-0 records that are not split."""
    from pomfret_amd import rank_p
    tested = [int(r["status"]) == 0 and not r.get("split", False) for r in recs]
    st = [rank_p(int(r["u2"]), int(r["n_reads"][0]), int(r["n_reads"][1]), int(r["ties"])) if t else None
          for r, t in zip(recs, tested)]
    q = bh_ref([s[2] if s else 1.0 for s in st], tested)
    lines = []
    for r, s, qq in zip(recs, st, q):
        ints = [int(r["start"]), int(r["end"]), *np.asarray(r["n_reads"]).ravel().tolist(),
                *np.asarray(r["n_short"]).ravel().tolist(), *np.asarray(r["cls"]).ravel().tolist()]
        mid = "\t.\t.\t.\t." if s is None else "\t%.4f\t%.3f\t%.6g\t%.6g" % (s[0], s[1], s[2], qq)
        m1, u1, m2, u2 = (int(x) for x in r["sum"])
        delta = "%.4f" % (m1 / (m1 + u1) - m2 / (m2 + u2)) if m1 + u1 and m2 + u2 else "."
        lines.append(r["chrom"] + "".join("\t%d" % x for x in ints) + mid + "\t%d\t%d\t%d\t%d\t%s\t%s\n"
                     % (m1, u1, m2, u2, delta, "split" if r.get("split", False) else "ok"))
    return THEAD + "".join(lines)


def _recs(seed=3, n=40):
    """n tiles of random reads: some with one haplotype only (status 1), some split."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        nr = int(rng.integers(1, 25))
        m, u = rng.integers(0, 9, nr), rng.integers(0, 9, nr)
        m[(m + u) == 0] = 1
        tags = rng.integers(0, 2, nr)
        if k % 7 == 3:
            tags[:] = k % 2                                  # status 1
        r = rank_ref(m.tolist(), u.tolist(), tags.tolist(), 3)
        out.append(dict(r, chrom="chrT" if k < n // 2 else "chrU", start=1000 * k, end=1000 * k + 1000, split=k % 5 == 4))
    return out


def test_text_and_rank_q(tmp_path):
    from pomfret_amd import write_rank_tiles
    recs = _recs()
    exp = tiles_text(recs)
    path = str(tmp_path / "t.tiles.tsv")
    n = write_rank_tiles(path, recs)
    assert open(path).read() == exp
    body = [x.split("\t") for x in exp.splitlines()[1:]]
    assert len(body[0]) == 23 and len(THEAD.rstrip("\n").split("\t")) == 23
    tested = [r["status"] == 0 and not r["split"] for r in recs]
    assert n == sum(tested) and 5 < n < len(recs)
    # split and status-1 records are left out of m: the q-values are bh_ref's over the rest
    st1 = [r for r in recs if r["status"] == 1]
    sp = [r for r in recs if r["split"] and r["status"] == 0]
    assert st1 and sp
    from pomfret_amd import rank_p
    p = [rank_p(r["u2"], r["n_reads"][0], r["n_reads"][1], r["ties"])[2] if t else 1.0 for r, t in zip(recs, tested)]
    assert [x[16] for x in body] == ["%.6g" % v if t else "." for v, t in zip(bh_ref(p, tested), tested)]
    with_all = bh_ref(p, [r["status"] == 0 for r in recs])           # a larger m gives other q-values
    assert ["%.6g" % v for v, t in zip(with_all, tested) if t] != [x[16] for x, t in zip(body, tested) if t]
    for x, r in zip(body, recs):
        assert x[22] == ("split" if r["split"] else "ok")
        if r["split"]:
            assert x[13:17] == ["."] * 4 and [int(v) for v in x[17:21]] == r["sum"]   # counted, not tested


def test_delta_dot_without_a_counted_call(tmp_path):
    from pomfret_amd import write_rank_tiles
    one = dict(rank_ref([2, 5], [1, 0], [0, 0], 3), chrom="c", start=0, end=100)        # haplotype 2 has no read
    short = dict(rank_ref([2, 1], [2, 0], [0, 1], 3), chrom="c", start=100, end=200)    # its one read is short
    both = dict(rank_ref([3, 0], [1, 4], [0, 1], 3), chrom="c", start=200, end=300)
    path = str(tmp_path / "d.tsv")
    assert write_rank_tiles(path, [one, short, both]) == 1
    text = open(path).read()
    assert text == tiles_text([one, short, both])
    rows = [x.split("\t") for x in text.splitlines()[1:]]
    assert [x[21] for x in rows] == [".", ".", "0.7500"] and rows[1][17:21] == ["2", "2", "0", "0"]
    assert rows[0][15] == "." and rows[2][15] != "."


def test_header_alone(tmp_path):
    from pomfret_amd import write_rank_tiles
    path = str(tmp_path / "e.tsv")
    assert write_rank_tiles(path, []) == 0
    assert open(path).read() == THEAD


def test_unwritable_path(tmp_path):
    from pomfret_amd import PomfretError, write_rank_tiles
    path = str(tmp_path / "no_such_dir" / "t.tsv")
    with pytest.raises(PomfretError, match=r"\(-1\)"):
        write_rank_tiles(path, _recs(n=3))
    assert not os.path.exists(path) and not os.path.exists(os.path.dirname(path))
