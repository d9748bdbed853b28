"""The crafted DEFLATE corpus (tests/_deflate.py, tests/_deflate_cases.py)
against zlib, on the CPU: every valid block inflates to exactly the bytes its
token stream implies, every malformed block is refused by zlib or by the
footer check, and the corpus as a whole reaches the corners of RFC 1951 it
was built for.  The device tests (test_inflate_streams_gpu.py) rest on this."""
import zlib

import numpy as np
import pytest

from tests import _deflate_cases as cases
from tests._deflate import (DIST_EXTRA, LEN_EXTRA, Lit, Match, Stream, canonical, cl_encode, kraft,
                            random_complete_lengths)


def all_valid():
    out = list(cases.valid_cases())
    for seed in cases.FUZZ_SEEDS:
        out += cases.fuzz_corpus(seed)
    return out


def refused(f, *args):
    """"zlib" / "footer" when f(*args) refuses its input, None when it accepts it."""
    try:
        f(*args)
    except zlib.error:
        return "zlib"
    except ValueError:
        return "footer"
    return None


def test_encoder_primitives():
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    codes = canonical([3, 3, 3, 3, 3, 2, 4, 4])
    want = ["010", "011", "100", "101", "110", "00", "1110", "1111"]
    assert [format(c, "0%db" % n)[::-1] for c, n in codes] == want
    rng = np.random.default_rng(0)
    for n, depth in ((2, 1), (2, 15), (16, 15), (30, 9), (286, 9), (286, 15), (19, 7), (100, 7)):
        d = random_complete_lengths(n, depth, rng)
        assert len(d) == n and kraft(d) == 32768 and max(d) <= depth
        assert max(d) == depth or n < depth + 1
    seq = [3, 3, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 5, 5, 5, 5]
    for style in ("none", "greedy", "split", "random"):
        got = []
        for s, k in cl_encode(seq, 8, style, rng):
            got += [s] if s < 16 else [0 if s > 16 else got[-1]] * k
        assert got == seq, style
    # a stored block after any bit position
    s = Stream().fixed([Lit(1)]).stored(b"").stored(b"xy").fixed([Lit(2), Match(3, 1)], final=True)
    assert zlib.decompress(s.payload(), -15) == bytes(s.out) == b"\x01xy\x02\x02\x02\x02"


def test_valid_roundtrip():
    n = 0
    for c in all_valid():
        assert zlib.decompress(c.block[18:-8], -15) == c.data, c.name
        assert cases.host_inflate(c.block) == c.data, c.name
        n += len(c.data)
    fuzz = [c for seed in cases.FUZZ_SEEDS for c in cases.fuzz_corpus(seed)]
    assert len(fuzz) == 3 * 64 and max(len(c.data) for c in fuzz) <= 20480 and min(len(c.data) for c in fuzz) == 0
    assert {r.btype for c in fuzz for r in c.records} == {0, 1, 2}
    assert n < 8 << 20


def test_malformed_refused():
    names = set()
    for e in cases.error_cases():
        assert refused(cases.host_inflate, e.block), e.name
        assert e.name not in names
        names.add(e.name)
        if e.name.startswith(("E1", "E2", "E3", "E4", "E5", "E6")):     # the stream itself is invalid
            assert refused(zlib.decompress, e.block[18:-8], -15) == "zlib", e.name
    # E9: the cut stream is incomplete for zlib; with the footer's first byte it would end cleanly
    e9 = cases.e9_case()
    with pytest.raises(zlib.error, match="incomplete"):
        zlib.decompress(e9.block[18:-8], -15)
    d = zlib.decompressobj(-15)
    d.decompress(e9.block[18:-7])
    assert d.eof and e9.block[-8] & 0x7F == 0
    assert {n[:2] for n in names} == {"E%d" % k for k in range(1, 10)}


def test_corpus_coverage():
    recs = [r for c in all_valid() for r in c.records]
    len_x, dist_x = {}, {}
    for r in recs:
        for tab, src in ((len_x, r.len_extra), (dist_x, r.dist_extra)):
            for k, (lo, hi) in src.items():
                e = tab.setdefault(k, [lo, hi])
                e[0], e[1] = min(e[0], lo), max(e[1], hi)
    assert sorted(len_x) == list(range(257, 286))
    assert sorted(dist_x) == list(range(30))
    for k, (lo, hi) in len_x.items():
        assert lo == 0 and hi == (1 << LEN_EXTRA[k - 257]) - 1, k
    for k, (lo, hi) in dist_x.items():
        assert lo == 0 and hi == (1 << DIST_EXTRA[k]) - 1, k
    dyn = [r for r in recs if r.btype == 2]
    assert set().union(*(r.ll_lens for r in dyn)) == set(range(1, 16))
    assert set().union(*(r.d_lens for r in dyn)) == set(range(1, 16))
    assert max(r.eob_len for r in dyn) == 15 and sum(r.eob_len > 10 for r in dyn) >= 2
    assert any(r.max_dist == 32768 for r in recs)
    assert any(r.d1_l258 for r in recs)
    assert any(r.starts_on_edge for r in recs) and any(r.ends_on_edge for r in recs)
    assert any(r.crosses_chunk for r in recs) and any(r.overlap for r in recs)
    # every block type starts at every bit phase
    for t in (0, 1, 2):
        assert {r.bit_start % 8 for r in recs if r.btype == t} == set(range(8)), t
    # both encodings of length 258
    assert any(r.len_extra.get(284, [0, 0])[1] == 31 for r in recs) and any(285 in r.len_extra for r in recs)


def test_directed_geometry():
    """The listed order puts every V7 / V8 case on a chunk edge of the output
    and the small blocks at the planned offsets."""
    off = 0
    small = {}
    for c in cases.valid_cases():
        if c.name.startswith(("V7.", "V8.")) and "geo_" not in c.name:
            assert off % 256 == 0, c.name
        if "geo_isize" in c.name:
            small.setdefault(len(c.data), set()).add(off % 256)
        off += len(c.data)
    assert sorted(small) == cases.GEO_ISIZES
    for n, offs in small.items():                  # every small ISIZE at 32 or more output phases
        assert len(offs) >= 32 and {0, 255} <= offs, n
    full = [c for c in cases.valid_cases() if c.name.startswith("V7.d1_full")]
    assert len(full) == 2 and all(len(c.data) == cases.MAX_ISIZE for c in full)
    assert min(len(c.block) for c in full) < 128


def test_sandwich_geometry():
    """Every malformed block starts on a chunk edge of the output, so the wrong
    CRCs of E8 are met with 1, 255 and 256 bytes in the last chunk."""
    bad = cases.error_cases()
    comp, slots = cases.sandwiches(bad)
    assert all(sl.out_off % 256 == 0 and 1 <= len(sl.pad.data) <= 256 for sl in slots)
    ends = sorted((sl.out_off + sl.isize) & 255 for b, sl in zip(bad, slots) if b.name.startswith("E8"))
    assert ends == [0, 1, 1, 255]
    o = 0
    for k in range(4 * len(bad)):                  # the blocks lie where the slots say
        if k % 4 == 1:
            assert comp[o:o + len(bad[k // 4].block)] == bad[k // 4].block and slots[k // 4].index == k
        o += int.from_bytes(comp[o + 16:o + 18], "little") + 1
    assert o == len(comp)


def test_mutants_classified():
    m = cases.mutants()
    assert sum(".flip" in x.name for x in m) == 256 and sum(".cut" in x.name for x in m) == 64
    assert len({x.base.name for x in m}) == 16
    assert any(x.good for x in m) and not all(x.good for x in m)
    for x in m:
        if ".cut" in x.name:
            assert len(x.block) < len(x.base.block)
