"""A small DEFLATE (RFC 1951) encoder for the tests (test infrastructure, pure
Python): the caller chooses every degree of freedom an encoder has -- block
types and their order, code lengths, the encoding of the code-length sequence,
the length symbol of a match -- so the device decoder (pf_inflate.hip) sees
valid streams no zlib ever emits, and malformed ones.  tests/
test_deflate_streams.py proves what this writes against zlib's decoder.

Every emitter fills a BlockRecord with what the emitted symbols actually
used; the corpus coverage assertions read those records."""
import struct
import zlib
from collections import namedtuple
from dataclasses import dataclass, field

Lit = namedtuple("Lit", "b")
Match = namedtuple("Match", "L D sym", defaults=(None,))   # sym: the length symbol, when two encode L
RawBits = namedtuple("RawBits", "v n")                     # n bits of v, LSB first (malformed streams)

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(L, alt=False):
    """(symbol, extra value) of match length L; alt: 258 as symbol 284 + 31."""
    if L == 258:
        return (284, 31) if alt else (285, 0)
    s = max(i for i in range(28) if LEN_BASE[i] <= L)
    return 257 + s, L - LEN_BASE[s]


def dist_symbol(D):
    s = max(i for i in range(30) if DIST_BASE[i] <= D)
    return s, D - DIST_BASE[s]


_LSYM = [None] * 259
for _L in range(3, 259):
    _LSYM[_L] = length_symbol(_L)
_DSYM = [None] * 32769
for _s in range(30):
    for _x in range(1 << DIST_EXTRA[_s]):
        _DSYM[DIST_BASE[_s] + _x] = (_s, _x)


def canonical(lengths):
    """Canonical Huffman codes of a list of code lengths: per symbol (code bits
    reversed for an LSB-first writer, length), None for length 0."""
    cnt = [0] * 16
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    nxt = [0] * 17
    code = 0
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if not l:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)               # (an over-subscribed set wraps; no decoder gets that far)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lengths):
    """Sum of 2^-l in units of 2^-15: 32768 for a complete set."""
    return sum(1 << (15 - l) for l in lengths if l)


def balanced_lengths(n):
    """A complete set of n >= 2 lengths, as flat as possible."""
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def random_complete_lengths(n, maxdepth, rng, force_max=True):
    """Depths of the n leaves of a random full binary tree no deeper than
    maxdepth: from one leaf, a random leaf shallower than the maximum is split
    until there are n (first along one spine down to maxdepth, when force_max
    and n allows, so the longest length is reached).  n == 1 gives [1]."""
    if n == 1:
        return [1]
    assert 2 <= n <= (1 << maxdepth)
    d = [0]
    if force_max and n >= maxdepth + 1:
        d = list(range(1, maxdepth + 1)) + [maxdepth]
    while len(d) < n:
        i = int(rng.integers(len(d)))
        if d[i] >= maxdepth:
            continue
        d[i] += 1
        d.append(d[i])
    return d


def spread_lengths(used, depths, n, rng=None):
    """Length list of n symbols: the depths (shuffled when rng) on `used`, 0 elsewhere."""
    depths = list(depths)
    if rng is not None:
        rng.shuffle(depths)
    out = [0] * n
    for s, l in zip(used, depths):
        out[s] = l
    return out


class BitWriter:
    """LSB-first bit stream; Huffman codes go in already reversed (canonical())."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 32:
            self.buf += (self.acc & 0xFFFFFFFF).to_bytes(4, "little")
            self.acc >>= 32
            self.n -= 32

    def align(self):
        self.n = (self.n + 7) & ~7

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def getvalue(self):
        nb = (self.n + 7) // 8
        return bytes(self.buf) + self.acc.to_bytes(nb, "little")


@dataclass
class BlockRecord:
    btype: int
    bit_start: int = 0                             # bit position of the block header in the stream
    ll_lens: set = field(default_factory=set)      # literal/length code lengths of emitted symbols
    d_lens: set = field(default_factory=set)
    len_extra: dict = field(default_factory=dict)  # length symbol -> [min, max] extra value emitted
    dist_extra: dict = field(default_factory=dict)
    eob_len: int = 0
    crosses_chunk: bool = False                    # a match spans a multiple of 256 (block-relative output)
    starts_on_edge: bool = False
    ends_on_edge: bool = False
    overlap: bool = False                          # a match with D < L
    max_dist: int = 0
    d1_l258: bool = False


def cl_encode(seq, nlit, style="greedy", rng=None):
    """The code-length sequence of seq (HLIT lengths then HDIST lengths) as
    (symbol, repeat) items.  none: literal lengths only; greedy: longest
    repeats, which may straddle the literal/length-to-distance boundary;
    split: repeats never straddle it; random: a random mix (rng)."""
    out = []
    i, n = 0, len(seq)
    while i < n:
        v = seq[i]
        end = n if style in ("greedy", "random") or i >= nlit else nlit
        r = 1
        while i + r < end and seq[i + r] == v:
            r += 1
        rep = style != "none" and (style != "random" or rng.random() < 0.7)
        if rep and v == 0 and r >= 3:
            k = min(r, 138)
            if style == "random":
                k = int(rng.integers(3, k + 1))
            out.append((18, k) if k >= 11 else (17, k))
            i += k
            continue
        prev_ok = i > 0 and seq[i - 1] == v and (style != "split" or i != nlit)
        if rep and v != 0 and prev_ok and r >= 3:
            k = min(r, 6)
            if style == "random":
                k = int(rng.integers(3, k + 1))
            out.append((16, k))
            i += k
            continue
        out.append((v, 1))
        i += 1
    return out


class Stream:
    """One raw DEFLATE stream under construction: .payload() is the stream,
    .out the bytes it implies, .records one BlockRecord per block."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.records = []

    def payload(self):
        return self.w.getvalue()

    def _rec(self, btype):
        r = BlockRecord(btype, self.w.bitpos)
        self.records.append(r)
        return r

    def stored(self, data, final=False, nlen=None):
        self._rec(0)
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        assert self.w.n % 8 == 0
        for b in data:
            self.w.bits(b, 8)
        self.out += data
        return self

    def raw_header(self, final, btype):
        self.w.bits(int(final), 1)
        self.w.bits(btype, 2)
        return self

    def fixed(self, tokens, final=False, eob=True):
        rec = self._rec(1)
        self.raw_header(final, 1)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), rec, eob)
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, hlit=None, hdist=None, hclen=None, cl_seq=None,
                cl_lens=None, style="greedy", rng=None, eob=True):
        """ll_lens / d_lens: code lengths by symbol (shorter lists are padded
        with 0 up to HLIT / HDIST).  cl_seq: explicit (symbol, repeat) items;
        cl_lens: the 19 code-length code lengths; both derived when None."""
        rec = self._rec(2)
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        if hlit is None:
            hlit = max([257] + [i + 1 for i, l in enumerate(ll_lens) if l])
        if hdist is None:
            hdist = max([1] + [i + 1 for i, l in enumerate(d_lens) if l])
        ll = (ll_lens + [0] * 320)[:hlit]
        d = (d_lens + [0] * 32)[:hdist]
        if cl_seq is None:
            cl_seq = cl_encode(ll + d, hlit, style, rng)
        if cl_lens is None:
            used = sorted({s for s, _ in cl_seq})
            if len(used) == 1:                       # a one-code set is incomplete: give it a sibling
                used.append(0 if used[0] else 1)
            cl_lens = spread_lengths(used, balanced_lengths(len(used)), 19)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        self.raw_header(final, 2)
        self.w.bits(hlit - 257, 5)
        self.w.bits(hdist - 1, 5)
        self.w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.w.bits(cl_lens[s], 3)
        clc = canonical(cl_lens)
        for s, k in cl_seq:
            self.w.bits(*clc[s])
            if s == 16:
                self.w.bits(k - 3, 2)
            elif s == 17:
                self.w.bits(k - 3, 3)
            elif s == 18:
                self.w.bits(k - 11, 7)
        self._tokens(tokens, canonical(ll), canonical(d), rec, eob)
        return self

    def _tokens(self, tokens, llc, dc, rec, eob):
        w, out = self.w, self.out
        for t in tokens:
            if type(t) is Lit:
                c = llc[t.b]
                w.bits(c[0], c[1])
                rec.ll_lens.add(c[1])
                out.append(t.b)
            elif type(t) is Match:
                L, D = t.L, t.D
                if t.sym is None:
                    ls, lx = _LSYM[L]
                else:
                    ls, lx = t.sym, L - LEN_BASE[t.sym - 257]
                    assert 0 <= lx < (1 << LEN_EXTRA[ls - 257])
                ds, dx = _DSYM[D]
                c = llc[ls]
                w.bits(c[0], c[1])
                rec.ll_lens.add(c[1])
                w.bits(lx, LEN_EXTRA[ls - 257])
                c = dc[ds]
                w.bits(c[0], c[1])
                rec.d_lens.add(c[1])
                w.bits(dx, DIST_EXTRA[ds])
                for tab, k, x in ((rec.len_extra, ls, lx), (rec.dist_extra, ds, dx)):
                    e = tab.setdefault(k, [x, x])
                    e[0] = min(e[0], x)
                    e[1] = max(e[1], x)
                a = len(out)
                rec.crosses_chunk |= (a >> 8) != ((a + L - 1) >> 8)
                rec.starts_on_edge |= a % 256 == 0
                rec.ends_on_edge |= (a + L) % 256 == 0
                rec.overlap |= D < L
                rec.max_dist = max(rec.max_dist, D)
                rec.d1_l258 |= D == 1 and L == 258
                if D > a:                          # malformed: the implied bytes are undefined
                    out += bytes(L)
                elif D >= L:
                    out += out[a - D:a - D + L]
                else:
                    out += (bytes(out[a - D:]) * (L // D + 1))[:L]
            else:
                w.bits(t.v, t.n)
        if eob:
            c = llc[256]
            w.bits(c[0], c[1])
            rec.ll_lens.add(c[1])
            rec.eob_len = c[1]


def bgzf_wrap(payload, data, crc=None, isize=None):
    """The BGZF block of a raw DEFLATE payload whose output is data (layout as
    tests/_bgzf.py); None when BSIZE would exceed 65536."""
    bsize = 18 + len(payload) + 8
    if bsize > 65536:
        return None
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize - 1)
    return hdr + bytes(payload) + struct.pack("<II", (zlib.crc32(data) & 0xFFFFFFFF) if crc is None else crc,
                                              len(data) if isize is None else isize)
