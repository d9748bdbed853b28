"""The crafted DEFLATE corpus (test infrastructure): directed valid BGZF
blocks, directed malformed ones, seeded structured fuzz and single-fault
mutants, all written by tests/_deflate.py.  tests/test_deflate_streams.py
checks every one of them against zlib on the CPU; tests/
test_inflate_streams_gpu.py feeds them to the device decoder.

Three limits of RFC 1951 and BGZF shape the cases at the edges:
 * HCLEN = 4 names only the code-length symbols 16, 17, 18 and 0, so every
   code length is 0 and the end-of-block code is missing: the smallest valid
   HCLEN is 5 (V5.hclen5); HCLEN = 4 is a malformed case (E4.hclen4);
 * a zero run that crosses from the literal/length lengths into the distance
   lengths starts after symbol 256, so it is at most 29 + 29 long: symbol 18
   crosses the boundary with repeat 58 (V5.rep18_cross) and reaches 138
   inside the literal/length lengths (V5.rep18_138);
 * one literal, 254 matches of length 258 at distance 1 and one of length 3
   fill the largest ISIZE, 65536 (V7.d1_full)."""
import functools
import struct
import zlib
from collections import namedtuple

import numpy as np

from tests._deflate import (CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, Lit, Match,
                            RawBits, Stream, bgzf_wrap, canonical, cl_encode, random_complete_lengths,
                            spread_lengths)

Case = namedtuple("Case", "name block data records")
BadCase = namedtuple("BadCase", "name block status")      # status: the device's code, None = any non-zero

MAX_ISIZE = 65536                                          # pf_bgzf_scan refuses a larger footer ISIZE


def host_inflate(block):
    """What a BGZF reader makes of one block: zlib's raw inflate of the payload
    (all of it consumed up to the final block), then the footer's ISIZE and
    CRC32.  Raises ValueError / zlib.error for a block it must fail."""
    bsize = struct.unpack_from("<H", block, 16)[0] + 1
    assert bsize == len(block)
    d = zlib.decompressobj(-15)
    out = d.decompress(block[18:-8])
    if not d.eof:
        raise ValueError("incomplete stream")
    crc, isize = struct.unpack_from("<II", block, len(block) - 8)
    if len(out) != isize:
        raise ValueError("ISIZE")
    if zlib.crc32(out) & 0xFFFFFFFF != crc:
        raise ValueError("CRC")
    return out


def _case(name, s):
    blk = bgzf_wrap(s.payload(), bytes(s.out))
    assert blk is not None and len(s.out) <= MAX_ISIZE, name
    return Case(name, blk, bytes(s.out), s.records)


def _lits(data):
    return [Lit(b) for b in data]


def _rand(rng, n, k=256):
    return rng.integers(0, k, n, dtype=np.uint8).tobytes()


def _spine(n):
    """Lengths 1, 2, ..., n-1, n-1: a complete set with one code of every length."""
    return list(range(1, n)) + [n - 1]


# ---------------------------------------------------------------------------
# directed valid cases

def _v1(rng):
    """Every (length symbol, extra) x (distance symbol, extra) pair at the
    minimum and maximum extra values, after 32768 stored bytes; the first match
    of the first block is D = 32768 onto the block's first byte."""
    lens = []
    for i in range(29):
        for x in sorted({0, (1 << LEN_EXTRA[i]) - 1}):
            lens.append(Match(LEN_BASE[i] + x, 0, 257 + i))
    dists = []
    for i in range(29, -1, -1):
        for x in sorted({0, (1 << DIST_EXTRA[i]) - 1}, reverse=True):
            dists.append(DIST_BASE[i] + x)
    assert dists[0] == 32768 and 24577 in dists
    pairs = [(m, d) for d in dists for m in lens]
    out, k, n = [], 0, 0
    while k < len(pairs):
        s = Stream().stored(_rand(rng, 32768))
        toks = []
        room = MAX_ISIZE - 32768
        while k < len(pairs) and pairs[k][0].L <= room:
            m, d = pairs[k]
            toks.append(Match(m.L, d, m.sym))
            room -= m.L
            k += 1
        s.fixed(toks, final=True)
        out.append(_case("V1.pairs%d" % n, s))
        n += 1
    return out


def _v2(rng):
    s = Stream().fixed([Lit(7), Match(258, 1), Match(258, 1, 284), Lit(9), Match(258, 2, 284)], final=True)
    ll = spread_lengths([7, 9, 256, 284, 285], [2, 2, 2, 3, 3], 286)
    t = Stream().dynamic([Lit(7), Match(258, 1, 284), Match(258, 1), Lit(9), Match(258, 259, 284)], ll, [1, 0, 0, 0,
                         0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], final=True)
    return [_case("V2.fixed", s), _case("V2.dynamic", t)]


def _all_symbol_tokens(rng, lits, hist):
    """Every literal of lits once, then every length symbol and every distance
    symbol twice (random extra values), with `hist` bytes already written."""
    toks = _lits(lits)
    for j in range(60):
        li, di = j % 29, j % 30
        L = LEN_BASE[li] + int(rng.integers(1 << LEN_EXTRA[li]))
        D = DIST_BASE[di] + int(rng.integers(1 << DIST_EXTRA[di]))
        assert D <= hist
        toks.append(Match(L, D, 257 + li))
    return toks


def _v3(rng):
    out = []
    for llmax, dmax in ((11, 9), (12, 10), (13, 11), (14, 12), (15, 13), (15, 14), (15, 15), (11, 15)):
        lits = rng.permutation(256)[:48].tolist()
        used = lits + list(range(256, 286))
        ll = spread_lengths(used, random_complete_lengths(len(used), llmax, rng), 286, rng)
        d = spread_lengths(range(30), random_complete_lengths(30, dmax, rng), 30, rng)
        assert max(ll) == llmax and max(d) == dmax
        s = Stream().stored(_rand(rng, 32768))
        s.dynamic(_all_symbol_tokens(rng, lits, 32768), ll, d, final=True)
        out.append(_case("V3.max%d_%d" % (llmax, dmax), s))
    # one code of every length 1..15 in both sets; the end-of-block code is 15 bits
    lits = list(range(65, 72))
    used = lits + [257, 258, 260, 265, 270, 275, 280, 285, 256]
    ll = spread_lengths(used, _spine(16), 286)
    dsy = [0, 1, 2, 3, 4, 5, 8, 11, 14, 17, 20, 23, 26, 28, 29, 16]
    d = spread_lengths(dsy, _spine(16), 30)
    assert ll[256] == 15 and sorted(set(ll) - {0}) == list(range(1, 16))
    toks = _lits(lits)
    for li, di in zip([0, 1, 3, 8, 13, 18, 23, 28] * 2, dsy):
        toks.append(Match(LEN_BASE[li], DIST_BASE[di], 257 + li))
    s = Stream().stored(_rand(rng, 32768)).dynamic(toks, ll, d, final=True)
    out.append(_case("V3.spine_eob15", s))
    # every literal on an 11-bit code: no speculative literal run
    ll = [11] * 256 + [2, 1, 3]
    data = _rand(rng, 700)
    toks = _lits(data[:300]) + [Match(3, 5), Match(4, 300)] + _lits(data[300:]) + [Match(3, 1)]
    out.append(_case("V3.long_literals", Stream().dynamic(toks, ll, spread_lengths([0, 4, 16], [1, 2, 2], 30), final=True)))
    # literals on 1- and 2-bit codes: 64 literals in one speculative step
    ll = spread_lengths([65, 66, 256, 257], [1, 2, 3, 3], 286)
    data = bytes(65 if x else 66 for x in rng.integers(0, 8, 900))
    toks = _lits(bytes([65]) * 200 + data[:400]) + [Match(3, 7)] + _lits(data[400:] + bytes([65]) * 130)
    out.append(_case("V3.short_literals", Stream().dynamic(toks, ll, [0] * 5 + [1], final=True)))
    return out


def _v4(rng):
    out = []
    ll = spread_lengths([97, 98, 99, 256], [2, 2, 2, 2], 286)
    out.append(_case("V4.no_dist", Stream().dynamic(_lits(b"abcabcaab" * 9), ll, [0], hdist=1, final=True)))
    ll = spread_lengths([97, 98, 256, 257, 260, 285], [2, 2, 3, 3, 3, 3], 286)
    toks = _lits(b"abba") + [Match(3, 1), Lit(98), Match(6, 1), Match(258, 1), Lit(97), Match(3, 1)]
    out.append(_case("V4.one_dist_d1", Stream().dynamic(toks, ll, [1], final=True)))
    toks = _lits(b"abbabaab") + [Match(3, 7), Lit(98), Match(6, 8), Match(258, 7), Lit(97), Match(3, 8)]
    out.append(_case("V4.one_dist_d7", Stream().dynamic(toks, ll, [0, 0, 0, 0, 0, 1], final=True)))
    out.append(_case("V4.only_eob", Stream().dynamic([], spread_lengths([256], [1], 257), [0], final=True)))
    ll = spread_lengths([0, 255, 256], [1, 2, 2], 257)
    out.append(_case("V4.hlit257_hdist1", Stream().dynamic(_lits(bytes([0, 255, 0, 0, 255])), ll, [0], hlit=257,
                                                             hdist=1, final=True)))
    ll = spread_lengths([0, 255, 256, 257], [1, 2, 3, 3], 286)
    toks = _lits(bytes([0, 255, 0, 0, 255])) + [Match(3, 2), Match(3, 1)]
    out.append(_case("V4.hlit286_hdist30", Stream().dynamic(toks, ll, [1, 1], hlit=286, hdist=30, final=True)))
    return out


def straddles(cl_seq, nlit):
    """Symbols of the repeat items of cl_seq that cover both sides of position nlit."""
    i, out = 0, set()
    for s, k in cl_seq:
        k = k if s >= 16 else 1
        if i < nlit < i + k:
            out.add(s)
        i += k
    return out


def _v5(rng):
    out = []
    # HCLEN 5 (symbols 16, 17, 18, 0, 8): every code is 8 bits
    ll = [8] * 255 + [0, 8]
    out.append(_case("V5.hclen5", Stream().dynamic(_lits(_rand(rng, 300, 255)), ll, [0], hclen=5, final=True)))
    s = Stream().dynamic(_lits(b"hello, hello"), spread_lengths([104, 101, 108, 111, 44, 32, 256],
                                                                 [2, 3, 3, 3, 3, 3, 3], 286), [0], hclen=19, final=True)
    out.append(_case("V5.hclen19", s))
    # symbol 16 across the boundary: ... 3 3 3 3 | 3 3 3 3 1
    ll = spread_lengths([97, 98, 253, 254, 255, 256], [2, 2, 3, 3, 3, 3], 257)
    d = [3, 3, 3, 3, 1]
    seq = cl_encode(ll + d, 257, "greedy")
    assert straddles(seq, 257) == {16}
    toks = _lits(b"abba" + bytes([253, 254, 255]))
    out.append(_case("V5.rep16_cross", Stream().dynamic(toks, ll, d, cl_seq=seq, final=True)))
    # symbol 18 across the boundary: lengths 257..285 and distance lengths 0..28 are one run of 58 zeros
    ll = spread_lengths([97, 98, 256], [1, 2, 2], 286)
    d = [0] * 29 + [1]
    seq = cl_encode(ll + d, 286, "greedy")
    assert (18, 58) in seq and straddles(seq, 286) == {18}
    out.append(_case("V5.rep18_cross", Stream().dynamic(_lits(b"abaab"), ll, d, hlit=286, cl_seq=seq, final=True)))
    ll = spread_lengths([250, 251, 256], [1, 2, 2], 257)
    seq = cl_encode(ll + [0], 257, "split")
    assert (18, 138) in seq
    out.append(_case("V5.rep18_138", Stream().dynamic(_lits(bytes([250, 251, 250])), ll, [0], cl_seq=seq, final=True)))
    # symbol 16 after 17 and after 18 repeats zeros
    ll = spread_lengths([8, 120, 256], [1, 2, 2], 257)
    seq = [(17, 5), (16, 3), (1, 1), (18, 108), (16, 3), (2, 1), (18, 132), (16, 3), (2, 1), (0, 1)]
    assert sum(k if s >= 16 else 1 for s, k in seq) == 258
    out.append(_case("V5.rep16_after_zero_run", Stream().dynamic(_lits(bytes([8, 120, 8])), ll, [0], cl_seq=seq,
                                                                   final=True)))
    ll = spread_lengths([97, 98, 99, 256, 257], [2, 2, 2, 3, 3], 286)
    out.append(_case("V5.no_repeats", Stream().dynamic(_lits(b"abcab") + [Match(3, 2)], ll, [1, 1], style="none",
                                                         final=True)))
    # code-length codes up to 7 bits: lengths 0..7 all in use, no repeats
    used = [65, 66, 67, 68, 69, 70, 256, 257]
    ll = spread_lengths(used, [1, 2, 3, 4, 5, 6, 7, 7], 286)
    cl = spread_lengths([0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 7], 19)
    toks = _lits(b"ABCDEFAB") + [Match(3, 1)]
    out.append(_case("V5.cl_7bit", Stream().dynamic(toks, ll, [1], style="none", cl_lens=cl, final=True)))
    return out


PAD_LL = spread_lengths([120, 256], [1, 1], 257)


def _pad_to_phase(s, phase):
    """A dynamic block of 1-bit literals after which the stream is at bit phase `phase`."""
    probe = Stream()
    probe.dynamic([], PAD_LL, [0])
    hdr = probe.w.bitpos                           # header + end-of-block, no literals
    k = (phase - (s.w.bitpos + hdr)) % 8
    s.dynamic([Lit(120)] * k, PAD_LL, [0])
    assert s.w.bitpos % 8 == phase


def _v6(rng):
    out = []
    ll = spread_lengths([97, 98, 99, 256, 257], [2, 2, 2, 3, 3], 286)
    for phase in range(8):
        s = Stream()
        _pad_to_phase(s, phase)
        s.stored(b"")
        _pad_to_phase(s, phase)
        s.fixed(_lits(b"fixed") + [Match(4, 2)])
        _pad_to_phase(s, phase)
        s.dynamic(_lits(b"abcab") + [Match(3, 2)], ll, [1, 1])
        _pad_to_phase(s, phase)
        s.stored(_rand(rng, 37), final=True)
        out.append(_case("V6.phase%d" % phase, s))
    out.append(_case("V6.empty_fixed_first", Stream().fixed([]).fixed(_lits(b"after"), final=True)))
    s = Stream()
    for j in range(40):
        s.dynamic(_lits(b"ab"[:1 + j % 2]) + ([Match(3, 1)] if j % 3 == 0 else []), ll, [1, 1], final=j == 39)
    out.append(_case("V6.tiny_x40", s))
    return out


def _pad_lits(toks, rng, pos, mod):
    """Literals up to the next output position congruent to mod (256)."""
    n = (mod - pos) % 256
    toks += _lits(_rand(rng, n))
    return pos + n


def _v7(rng):
    out = []
    for D in (1, 2, 3, 4, 5, 255, 256, 257, 258):
        toks = _lits(_rand(rng, 600))
        pos = 600
        for start, L in ((251, 10), (255, 258), (0, 20), (226, 30), (100, 50), (250, 258), (3, 253), (254, 3)):
            pos = _pad_lits(toks, rng, pos, start)
            toks.append(Match(L, D))
            pos += L
        toks += _lits(_rand(rng, 70))
        out.append(_case("V7.span_d%d" % D, Stream().fixed(toks, final=True)))
    # sources that are themselves pending matches of the same chunk, six deep
    toks = _lits(_rand(rng, 256)) + _lits(b"wxyz")
    toks += [Match(4, 4), Match(8, 8), Match(16, 16), Match(32, 32), Match(64, 64), Match(100, 3), Match(20, 101)]
    toks += _lits(_rand(rng, 300)) + [Match(5, 2), Match(7, 3), Match(9, 4), Match(11, 6), Match(13, 9), Match(90, 1)]
    out.append(_case("V7.chain", Stream().fixed(toks, final=True)))
    # the largest ISIZE from the smallest input
    toks = [Lit(0)] + [Match(258, 1)] * 254 + [Match(3, 1)]
    out.append(_case("V7.d1_full_fixed", Stream().fixed(toks, final=True)))
    ll = spread_lengths([0, 256, 257, 285], [3, 3, 2, 1], 286)
    out.append(_case("V7.d1_full", Stream().dynamic(toks, ll, [1], final=True)))
    assert len(out[-1].data) == MAX_ISIZE
    return out


# out_off & 255 of the small blocks below: every ISIZE at each of these 32 values
GEO_OFFSETS = [0, 255, 1, 254, 2, 253, 3, 252, 63, 64, 65, 127, 128, 129, 191, 192, 193, 4, 5, 7, 8, 9, 15, 16, 17,
               31, 32, 33, 250, 251, 100, 200]
GEO_ISIZES = [0, 1, 63, 64, 65, 255, 256, 257]


def _small_block(rng, n, dynamic):
    data = _rand(rng, n, 4)
    toks = _lits(data[:n - 5]) + [Match(5, min(3, n - 5))] if n >= 6 else _lits(data)
    if not dynamic:
        return Stream().fixed(toks, final=True)
    ll = spread_lengths([0, 1, 2, 3, 256, 259], [2, 2, 3, 3, 3, 3], 286)
    return Stream().dynamic(toks, ll, [1, 2, 2], final=True)


def _v8(rng):
    out = []
    out.append(_case("V8.literals", Stream().fixed(_lits(_rand(rng, 200)), final=True)))
    toks = _lits(_rand(rng, 120, 4))
    n = 120
    while n < 200:
        L = min(int(rng.integers(3, 11)), 203 - n)
        toks.append(Match(L, int(rng.integers(1, 40))))
        n += L
    out.append(_case("V8.short_matches", Stream().fixed(toks, final=True)))
    out.append(_case("V8.match_to_isize", Stream().fixed(_lits(_rand(rng, 150)) + [Match(3, 9)], final=True)))
    out.append(_case("V8.long_match_to_isize", Stream().fixed(_lits(_rand(rng, 150)) + [Match(258, 100)], final=True)))
    out.append(_case("V8.short_block_match", Stream().fixed(_lits(b"abc") + [Match(40, 3)], final=True)))
    out.append(_case("V8.literal_then_64", Stream().fixed(_lits(_rand(rng, 66, 3)) + [Match(62, 5), Lit(1), Lit(2)],
                                                          final=True)))
    return out


def _filler(name, rng, n):
    return _case(name, Stream().stored(_rand(rng, n), final=True))


@functools.lru_cache(maxsize=None)
def valid_cases():
    """The directed valid cases in listed order.  The geometry cases (V7, V8)
    follow stored filler blocks that bring the running output size to a
    multiple of 256, so block-relative chunk edges are the decoder's own
    (its chunks are aligned to the output arena) when the blocks are
    inflated in this order from offset 0."""
    rng = np.random.default_rng(1951)
    cases = _v1(rng) + _v2(rng) + _v3(rng) + _v4(rng) + _v5(rng) + _v6(rng)
    total = sum(len(c.data) for c in cases)
    for c in _v7(rng) + _v8(rng):
        if total % 256:
            cases.append(_filler("align.%s" % c.name, rng, 256 - total % 256))
            total += len(cases[-1].data)
        cases.append(c)
        total += len(c.data)
    for j, (n, off) in enumerate((n, off) for n in GEO_ISIZES for off in GEO_OFFSETS):
        pre = (off - total) % 256 or 256
        cases.append(_filler("V7.geo_pre%d" % j, rng, pre))
        cases.append(_case("V7.geo_isize%d_at%d" % (n, off), _small_block(rng, n, j % 3 == 0)))
        total += pre + n
    return tuple(cases)


# ---------------------------------------------------------------------------
# directed malformed cases

def _bad(name, s, status, crc=None, isize=None):
    blk = bgzf_wrap(s.payload(), bytes(s.out), crc, isize)
    assert blk is not None
    return BadCase(name, blk, status)


@functools.lru_cache(maxsize=None)
def error_cases():
    rng = np.random.default_rng(1952)
    out = []
    fll, fd = canonical(FIXED_LL), canonical(FIXED_D)
    ok_ll = spread_lengths([97, 98, 256, 257], [2, 2, 2, 2], 286)
    tail = [Lit(97), Lit(98)]
    out.append(_bad("E1.btype3", Stream().fixed(_lits(b"ab")).raw_header(True, 3).fixed(_lits(b"cd"), final=True), 1))
    out.append(_bad("E1.btype3_first", Stream().raw_header(True, 3).fixed(_lits(b"cd"), final=True), 1))
    out.append(_bad("E2.nlen", Stream().stored(b"stored", final=True, nlen=0xFFF8), 2))
    out.append(_bad("E2.nlen_equal", Stream().fixed(_lits(b"x")).stored(b"stored", final=True, nlen=6), 2))
    # E3: code sets zlib's inflate_table refuses
    out.append(_bad("E3.ll_over", Stream().dynamic([], spread_lengths([0, 1, 256], [1, 1, 1], 257), [0], final=True), 3))
    out.append(_bad("E3.ll_over_deep", Stream().dynamic([], spread_lengths([0, 1, 2, 256], [1, 2, 15, 2], 257), [0],
                                                         final=True), 3))
    out.append(_bad("E3.dist_over", Stream().dynamic(tail, ok_ll, [1, 1, 1], final=True), 3))
    out.append(_bad("E3.dist_over_deep", Stream().dynamic(tail, ok_ll, [1, 2, 3, 3, 9], final=True), 3))
    cl = spread_lengths([0, 1, 2], [1, 1, 1], 19)
    out.append(_bad("E3.cl_over", Stream().dynamic([], spread_lengths([0, 256], [1, 1], 257), [0], style="none",
                                                    cl_lens=cl, final=True), 3))
    out.append(_bad("E3.ll_incomplete", Stream().dynamic([Lit(0)], spread_lengths([0, 256], [2, 2], 257), [0],
                                                          final=True), 3))
    out.append(_bad("E3.ll_incomplete_deep", Stream().dynamic([Lit(0)], spread_lengths([0, 1, 256], [1, 2, 15], 257),
                                                               [0], final=True), 3))
    out.append(_bad("E3.dist_incomplete", Stream().dynamic(tail, ok_ll, [2, 2, 2], final=True), 3))
    cl = spread_lengths([0, 1], [2, 2], 19)
    out.append(_bad("E3.cl_incomplete", Stream().dynamic([], spread_lengths([0, 256], [1, 1], 257), [0], style="none",
                                                          cl_lens=cl, final=True), 3))
    cl = spread_lengths([1], [1], 19)
    out.append(_bad("E3.cl_one_code", Stream().dynamic([], [1] * 257, [1], style="none", cl_lens=cl, final=True), 3))
    # E4: code-length sequences
    ll = spread_lengths([0, 1, 2, 3, 256], [3, 3, 3, 3, 1], 257)
    seq = [(16, 3)] + cl_encode((ll + [0])[3:], 254, "split")
    out.append(_bad("E4.rep16_first", Stream().dynamic([], ll, [0], cl_seq=seq, final=True), 3))
    seq = cl_encode(ll + [0], 257, "split")[:-1] + [(17, 3)]
    out.append(_bad("E4.rep17_past_end", Stream().dynamic([], ll, [0], cl_seq=seq, final=True), 3))
    seq = cl_encode(ll + [0], 257, "split")[:-2] + [(16, 6)]
    out.append(_bad("E4.rep16_past_end", Stream().dynamic([], ll, [0], cl_seq=seq, final=True), 3))
    seq = cl_encode(ll + [0], 257, "split")[:-1] + [(18, 138)]
    out.append(_bad("E4.rep18_past_end", Stream().dynamic([], ll, [0], cl_seq=seq, final=True), 3))
    out.append(_bad("E4.no_eob", Stream().dynamic([Lit(0)], spread_lengths([0, 1], [1, 1], 257), [0], eob=False,
                                                   final=True), 3))
    for hlit in (287, 288):
        out.append(_bad("E4.hlit%d" % hlit, Stream().dynamic(tail, ok_ll, [1, 1], hlit=hlit, final=True), 3))
    for hdist in (31, 32):
        out.append(_bad("E4.hdist%d" % hdist, Stream().dynamic(tail, ok_ll, [1, 1], hdist=hdist, final=True), 3))
    cl = spread_lengths([0, 18], [1, 1], 19)
    seq = [(18, 138), (18, 120)]
    out.append(_bad("E4.hclen4", Stream().dynamic([], [0] * 257, [0], cl_seq=seq, cl_lens=cl, hclen=4, eob=False,
                                                   final=True), 3))
    # E5: codes that name nothing
    for sym in (286, 287):
        out.append(_bad("E5.fixed_ll%d" % sym, Stream().fixed(_lits(b"ab") + [RawBits(*fll[sym]), RawBits(0, 5)],
                                                              final=True), 3))
    for sym in (30, 31):
        out.append(_bad("E5.fixed_dist%d" % sym, Stream().fixed(_lits(b"ab") + [RawBits(*fll[257]),
                                                                RawBits(*fd[sym])], final=True), 3))
    llc = canonical(ok_ll)
    out.append(_bad("E5.match_no_dist", Stream().dynamic(tail + [RawBits(*llc[257]), RawBits(0, 6)], ok_ll, [0],
                                                          final=True), 3))
    out.append(_bad("E5.one_dist_unused", Stream().dynamic(tail + [RawBits(*llc[257]), RawBits(1, 1)], ok_ll, [1],
                                                            final=True), 3))
    out.append(_bad("E5.one_dist_unused_first", Stream().dynamic([RawBits(*llc[257]), RawBits(1, 1)], ok_ll, [1],
                                                                  final=True), 3))
    # E6: one byte before the block's first
    out.append(_bad("E6.first_symbol", Stream().fixed([Match(3, 1)], final=True), 4))
    out.append(_bad("E6.second_symbol", Stream().fixed([Lit(5), Match(3, 2)], final=True), 4))
    out.append(_bad("E6.after_32767", Stream().stored(_rand(rng, 32767)).fixed([Match(3, 32768)], final=True), 4))
    ll = spread_lengths([0, 256, 257], [1, 2, 2], 286)
    d = spread_lengths([29, 0], [1, 1], 30)
    out.append(_bad("E6.after_32767_dynamic", Stream().stored(_rand(rng, 32767)).dynamic([Match(3, 32768)], ll, d,
                                                                                          final=True), 4))
    # E7: output against ISIZE
    for n in (1, 70, 300):
        data = _rand(rng, n, 5)
        s = Stream().fixed(_lits(data), final=True)
        out.append(_bad("E7.short_%d" % n, s, 5, isize=n + 1))
        out.append(_bad("E7.over_literal_%d" % n, s, 5, isize=n - 1))
        s = Stream().fixed(_lits(data) + [Match(3, 1)], final=True)
        out.append(_bad("E7.over_match_%d" % n, s, 5, isize=n + 2))
        s = Stream().fixed(_lits(data)).stored(b"xyz", final=True)
        out.append(_bad("E7.over_stored_%d" % n, s, 5, isize=n + 2))
    s = Stream().fixed(_lits(_rand(rng, 100, 5)) + [Match(258, 3)], final=True)
    out.append(_bad("E7.over_long_match", s, 5, isize=357))
    # E8: a wrong CRC; a bad block starts on a chunk edge (sandwiches), so the last chunk holds 1, 255, 256, 1 bytes
    for n, bit in ((257, 0), (511, 31), (512, 13), (1, 7)):
        data = _rand(rng, n, 7)
        s = Stream().fixed(_lits(data), final=True)
        out.append(_bad("E8.crc_%d" % n, s, 7, crc=(zlib.crc32(data) & 0xFFFFFFFF) ^ (1 << bit)))
    out.append(e9_case())
    return tuple(out)


def e9_case():
    """A fixed block whose 7-bit end-of-block code is the payload's last byte,
    alone; the byte is cut off and BSIZE shortened, the footer kept, and the
    data chosen so the footer's first byte reads as the missing code."""
    for a in range(144):
        for b in range(144):
            data = bytes([200, 201, 202, 203, 204, 65, 66, a, b])       # five 9-bit literals: 3 + 45 + 32 = 80 bits
            if zlib.crc32(data) & 0x7F == 0:
                s = Stream().fixed(_lits(data), final=True)
                p = s.payload()
                assert len(p) == 11 and p[-1] == 0 and s.w.bitpos == 87
                return BadCase("E9.cut_eob", bgzf_wrap(p[:-1], data), 6)
    raise AssertionError("no data with crc32 & 0x7f == 0")


def bad_layout(case):
    """(input bytes, index of the bad block, neighbours) of one malformed
    block between two valid ones; the left one's output is 256 bytes."""
    left, right = _neighbours()
    return left.block + case.block + right.block, 1, (left, right)


@functools.lru_cache(maxsize=None)
def _pad_block(n):
    return _case("pad%d" % n, Stream().stored(bytes((7 * i + n) & 255 for i in range(n)), final=True))


Slot = namedtuple("Slot", "index out_off isize pad")       # of one bad block in sandwiches()


def sandwiches(bad):
    """(input bytes, one Slot per bad block) of left, bad, right, pad for every
    bad block in turn: the stored pad block (1 to 256 bytes) brings the output
    to a multiple of 256 and left's output is 256 bytes, so every bad block
    starts on a chunk edge of the output however long the blocks before it are."""
    left, right = _neighbours()
    comp, slots, off = [], [], 0
    for i, b in enumerate(bad):
        isize = struct.unpack_from("<I", b.block, len(b.block) - 4)[0]
        pad = _pad_block(256 - (isize + len(right.data)) % 256)
        comp += [left.block, b.block, right.block, pad.block]
        slots.append(Slot(4 * i + 1, off + 256, isize, pad))
        off += 256 + isize + len(right.data) + len(pad.data)
        assert off % 256 == 0
    return b"".join(comp), slots


@functools.lru_cache(maxsize=None)
def _neighbours():
    rng = np.random.default_rng(7)
    toks = _lits(_rand(rng, 100, 6)) + [Match(56, 17)] + _lits(_rand(rng, 100))
    left = _case("left256", Stream().fixed(toks, final=True))
    ll = spread_lengths([1, 2, 3, 256, 258], [2, 2, 2, 3, 3], 286)
    toks = [Lit(1 + int(x)) for x in rng.integers(0, 3, 90)]
    right = _case("right", Stream().dynamic(toks + [Match(4, 33)], ll, spread_lengths([9, 10], [1, 1], 30), final=True))
    return left, right


# ---------------------------------------------------------------------------
# seeded structured fuzz

FUZZ_SEEDS = (11, 12, 13)
FUZZ_BLOCKS = 64
_XL = [3, 10, 11, 258]
_XD = [1, 4, 5, 256, 257, 32768]


def _log_uniform(rng, lo, hi):
    return int(min(hi, max(lo, round(float(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))) - 0.5)))))


def _random_tokens(rng, hist, n):
    """Tokens for n output bytes with hist bytes of history."""
    k = _log_uniform(rng, 2, 256)
    alpha = rng.permutation(256)[:k]
    p_match = rng.uniform(0.02, 0.6)
    toks = []
    left = n
    lits = alpha[rng.integers(0, k, n + 1)].tolist()
    coin = rng.random(n + 1).tolist()
    while left > 0:
        if hist and left >= 3 and coin[left] < p_match:
            L = _XL[int(rng.integers(4))] if rng.random() < 0.3 else _log_uniform(rng, 3, 258)
            D = _XD[int(rng.integers(6))] if rng.random() < 0.3 else _log_uniform(rng, 1, 32768)
            L = min(L, left)
            if D > hist:
                D = int(rng.integers(1, hist + 1))
            alt = L == 258 and rng.random() < 0.5
            toks.append(Match(L, D, 284 if alt else None))
            hist += L
            left -= L
        else:
            toks.append(Lit(lits[left]))
            hist += 1
            left -= 1
    return toks


def _random_sets(rng, toks):
    """Random complete literal/length and distance length sets for toks."""
    from tests._deflate import _DSYM, _LSYM
    lu, du = {256}, set()
    for t in toks:
        if type(t) is Lit:
            lu.add(t.b)
        else:
            lu.add(t.sym or _LSYM[t.L][0])
            du.add(_DSYM[t.D][0])
    for extra, pool, n in ((lu, 286, int(rng.integers(0, 4))), (du, 30, int(rng.integers(0, 3)))):
        for s in rng.integers(0, pool, n).tolist():      # coded but never emitted
            extra.add(s)
    lu, du = sorted(lu), sorted(du)
    if len(lu) == 1:
        lu.append(int(rng.integers(0, 256)))
    depth = int(rng.integers(7, 16))
    ll = spread_lengths(lu, random_complete_lengths(len(lu), max(depth, (len(lu) - 1).bit_length()), rng), 286, rng)
    depth = int(rng.integers(7, 16))
    d = spread_lengths(du, random_complete_lengths(len(du), depth, rng), 30, rng) if du else [0]
    return ll, d


def random_block(rng):
    """One BGZF block of 1 to 6 DEFLATE blocks of random type."""
    nb = int(rng.integers(1, 7))
    total = 0 if rng.random() < 0.05 else _log_uniform(rng, 1, 20480)
    cuts = sorted(rng.integers(0, total + 1, nb - 1).tolist()) + [total]
    s = Stream()
    at = 0
    for j, c in enumerate(cuts):
        n, final = c - at, j == nb - 1
        at = c
        btype = int(rng.integers(0, 3))
        if btype == 0:
            s.stored(_rand(rng, n, _log_uniform(rng, 2, 256)), final=final)
            continue
        toks = _random_tokens(rng, len(s.out), n)
        if btype == 1:
            s.fixed(toks, final=final)
            continue
        ll, d = _random_sets(rng, toks)
        style = ("none", "greedy", "split", "random")[int(rng.integers(4))]
        hlit = int(rng.integers(max(257, max(i for i, l in enumerate(ll) if l) + 1), 287))
        hdist = int(rng.integers(max(1, max([0] + [i + 1 for i, l in enumerate(d) if l])), 31))
        seq = cl_encode((ll + [0] * 30)[:hlit] + (d + [0] * 30)[:hdist], hlit, style, rng)
        used = sorted({x for x, _ in seq})
        if len(used) == 1:
            used.append(0 if used[0] else 1)
        cl = spread_lengths(used, random_complete_lengths(len(used), int(rng.integers(5, 8)), rng, False), 19, rng)
        hclen = int(rng.integers(max(4, max(i + 1 for i, x in enumerate(CL_ORDER) if cl[x])), 20))
        s.dynamic(toks, ll, d, final=final, hlit=hlit, hdist=hdist, hclen=hclen, cl_seq=seq, cl_lens=cl)
    return s


@functools.lru_cache(maxsize=None)
def fuzz_corpus(seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < FUZZ_BLOCKS:
        s = random_block(rng)
        if bgzf_wrap(s.payload(), bytes(s.out)) is None:      # (a stored-heavy block over 64 KiB: drawn again)
            continue
        out.append(_case("fuzz%d.%d" % (seed, len(out)), s))
    return tuple(out)


# ---------------------------------------------------------------------------
# single-fault mutants of fuzz blocks

Mutant = namedtuple("Mutant", "name block good base")      # good: zlib + footer accept it as the base block's bytes


def _classify(block, data):
    try:
        return host_inflate(block) == data
    except (zlib.error, ValueError):
        return False


@functools.lru_cache(maxsize=None)
def mutants():
    """256 single-bit flips and 64 truncations (1 to 12 payload bytes, BSIZE
    adjusted, footer kept) of 16 fuzz blocks, none excluded; each is
    classified by zlib and the footer."""
    rng = np.random.default_rng(1953)
    base = [c for c in fuzz_corpus(FUZZ_SEEDS[0]) if len(c.block) - 26 >= 16][:16]
    assert len(base) == 16
    out = []
    for c in base:
        npay = len(c.block) - 26
        for j in range(16):
            bit = int(rng.integers(0, 8 * npay))
            b = bytearray(c.block)
            b[18 + bit // 8] ^= 1 << (bit % 8)
            out.append(Mutant("%s.flip%d" % (c.name, bit), bytes(b), _classify(bytes(b), c.data), c))
        for j in range(4):
            cut = int(rng.integers(1, 13))
            b = bytearray(c.block[:-8 - cut] + c.block[-8:])
            struct.pack_into("<H", b, 16, len(b) - 1)
            out.append(Mutant("%s.cut%d" % (c.name, cut), bytes(b), _classify(bytes(b), c.data), c))
    return tuple(out)
