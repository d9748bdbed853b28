"""Device BGZF inflate (pf_inflate.hip) on hand-built DEFLATE streams that
zlib's encoder never emits (tests/_deflate.py, tests/_deflate_cases.py; all of
them proven against zlib's decoder in test_deflate_streams.py): every length
and distance symbol at both ends of its extra bits, distance 32768, codes of
11 to 15 bits (the lane-parallel canonical fallback), degenerate code sets,
every code-length encoding, block sequences at every bit phase, matches
across chunk edges and chains of pending matches, and the malformed streams
behind every status code of pf_ingest.h.

Why malformed input is safe to run (read from inflate_blocks, pf_inflate.hip):

Input.  Every global load of compressed bytes is bits_issue's, which clamps
its dword index to lim - 1, and lim is the payload's dwords plus 2: at most 11
bytes past the payload, inside the 8 footer bytes and the next block or the
512 bytes pf_bgzf_inflate pads the input with.  bits_fill reads the LDS ring at
rd & 127.  Once rd passes lim, `over` is set and stale ring words are decoded.
After the final block the bits consumed are compared with the payload's size
exactly, so a stream that ends in the footer or the slack is refused (E9).

Termination.  Every DEFLATE block consumes at least 3 header bits and the
block loop ends on err or BFINAL.  `over` is checked after every code-length
item, after every match, after a stored block and at every end of block, so
after the input is exhausted at most one block's literals follow, and those
are bounded as below.  The code-length loop advances i by rep >= 1 up to
total <= 316.  A stored copy runs len <= 65535 steps, and only when
a + len <= hi.  In the symbol loop every pass either emits a symbol or ends:
the general step takes a literal only while a < hi, a match only when
a + L <= hi; the speculative run takes at most 64 symbols per pass and is
entered with hi - a >= 64 or checks a < hi per literal.  (A run of 1-bit
literals after an in-run match can carry `a` past hi by under 64 bytes.  Then
hi - a wraps, so the unchecked branch of the run is taken again in every
later pass and block: the overshoot is bounded by the input's size, not by 64
bytes.  From then on every match and every general-step literal is refused,
so each further pass must end its block, and the block loop ends with the
input; no byte at or past hi is stored, see Output.  Such a stream ends with
a != hi: status 5 or 6.)  out_flush's resolve loop settles at least the
earliest pending byte per round, since a source always precedes its byte and
never lies before lo (D <= a - lo is checked before every match, in the run
and in the general step).

Tables.  HLIT <= 286 and HDIST <= 30 are checked before any length is
stored, so lens[] indices stay below 288 + 30; a repeat is refused when
i + rep > total; build_table refuses an over-subscribed set before it fills
a root table, and root fills and sorted-symbol stores are indexed by ranks
below the symbol count.  slow_decode reads sym[off + code - fst] only for
code - fst < cnt.

Output.  out_lit and out_match only write registers.  out_flush is the only
global store and stores byte q only for lo <= q < hi and q < a; its only
global loads are of match sources, lo <= s < cb, bytes it has already
stored.  The CRC fold touches registers and LDS.

So for every class below (bad block types, stored lengths, code sets,
code-length sequences, invalid codes, far distances, size overruns, wrong
CRCs, cut payloads, single-bit flips and truncations) the decode ends and no
access leaves the block's input window plus slack or its [lo, hi) output."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import _deflate_cases as cases

pytestmark = pytest.mark.gpu


def inflate_raw(ctx, comp):
    """pf_bgzf_inflate without the wrapper's raise: (output bytes, per-block
    status, return code), so a failed call's neighbours can be compared."""
    from pomfret_amd._lib import lib
    comp = np.frombuffer(bytes(comp), np.uint8)
    cap = 65536 * (comp.size // 28 + 1)
    out = np.zeros(cap, np.uint8)
    n = C.c_uint64()
    st = np.zeros(comp.size // 26 + 1, np.uint32)
    ms = C.c_float()
    rc = lib().pf_bgzf_inflate(ctx.handle, comp.ctypes.data, comp.size, out.ctypes.data, cap, C.byref(n),
                               st.ctypes.data, st.size, C.byref(ms))
    return out[:n.value].tobytes(), st, rc


def check_valid(ctx, blocks):
    comp = b"".join(c.block for c in blocks)
    got, st, rc = inflate_raw(ctx, comp)
    off = 0
    for i, c in enumerate(blocks):                 # the first differing block, by case name
        assert st[i] == 0, "%s: status %d (block %d)" % (c.name, st[i], i)
        assert got[off:off + len(c.data)] == c.data, "%s: bytes differ (block %d, output offset %d)" % (c.name, i, off)
        off += len(c.data)
    assert off == len(got) and not st.any() and rc == 0


def layout(blocks):
    """(in_off & 3, out_off & 255) of every block of a concatenation."""
    i = o = 0
    out = []
    for c in blocks:
        out.append(((i + 18) & 3, o & 255))
        i += len(c.block)
        o += len(c.data)
    return out


def test_crafted_valid(gpu_ctx):
    listed = list(cases.valid_cases())
    lay = layout(listed)
    assert {a for a, _ in lay} == {0, 1, 2, 3}
    for n in cases.GEO_ISIZES:                     # every small ISIZE at 32 or more output phases
        geo = {o for (_, o), c in zip(lay, listed) if "geo_isize" in c.name and len(c.data) == n}
        assert len(geo) >= 32 and {0, 255} <= geo, n
    check_valid(gpu_ctx, listed)
    rng = np.random.default_rng(5)
    shuffled = [listed[i] for i in rng.permutation(len(listed))]
    assert {a for a, _ in layout(shuffled)} == {0, 1, 2, 3}
    check_valid(gpu_ctx, shuffled)
    # and through the wrapper, as the callers reach it
    got, st, ms = gpu_ctx.bgzf_inflate(b"".join(c.block for c in listed))
    assert not st.any() and got == b"".join(c.data for c in listed)


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_crafted_fuzz(gpu_ctx, seed):
    blocks = list(cases.fuzz_corpus(seed))
    check_valid(gpu_ctx, blocks)
    rng = np.random.default_rng(seed)
    check_valid(gpu_ctx, [blocks[i] for i in rng.permutation(len(blocks))])


def check_sandwiches(ctx, bad, want):
    """One call: left, bad[0], right, pad, left, bad[1], right, pad, ...
    (cases.sandwiches: every bad block starts on a chunk edge of the output);
    want(i, status) judges bad block i; every neighbour must be intact."""
    left, right = cases.bad_layout(bad[0])[2]
    comp, slots = cases.sandwiches(bad)
    got, st, rc = inflate_raw(ctx, comp)
    assert len(st) >= 4 * len(bad)
    problems = []
    for i, (b, sl) in enumerate(zip(bad, slots)):
        assert sl.out_off % 256 == 0
        k, off = sl.index, sl.out_off
        if st[k - 1] != 0 or st[k + 1] != 0 or st[k + 2] != 0:
            problems.append("%s: neighbour status %d / %d / %d" % (b.name, st[k - 1], st[k + 1], st[k + 2]))
        if got[off - 256:off] != left.data:
            problems.append("%s: left neighbour's bytes" % b.name)
        off += sl.isize
        if got[off:off + len(right.data)] != right.data:
            problems.append("%s: right neighbour's bytes" % b.name)
        off += len(right.data)
        if got[off:off + len(sl.pad.data)] != sl.pad.data:
            problems.append("%s: pad block's bytes" % b.name)
        msg = want(i, int(st[k]))
        if msg:
            problems.append("%s: %s" % (b.name, msg))
    assert slots[-1].out_off + slots[-1].isize + len(right.data) + len(slots[-1].pad.data) == len(got)
    assert not problems, "\n".join(problems)
    return rc


def test_crafted_errors(gpu_ctx):
    from pomfret_amd._lib import PomfretError
    bad = list(cases.error_cases())

    def want(i, status):
        if status == 0:
            return "accepted (status 0), want %s" % bad[i].status
        if bad[i].status is not None and status != bad[i].status:
            return "status %d, want %d" % (status, bad[i].status)

    # E8's geometry, from the layout that runs: the wrong CRC is met with 1, 255 and 256 bytes in the last chunk
    ends = {b.name: (sl.out_off + sl.isize) & 255 for b, sl in zip(bad, cases.sandwiches(bad)[1]) if b.name[:2] == "E8"}
    assert ends == {"E8.crc_257": 1, "E8.crc_511": 255, "E8.crc_512": 0, "E8.crc_1": 1}
    assert check_sandwiches(gpu_ctx, bad, want) != 0
    # and through the wrapper: the call fails, the status words stay readable
    comp, at, _ = cases.bad_layout(bad[0])
    with pytest.raises(PomfretError):
        gpu_ctx.bgzf_inflate(comp)
    assert list(gpu_ctx.last_inflate_status[:3]) == [0, bad[0].status, 0]


def test_crafted_mutants(gpu_ctx):
    m = list(cases.mutants())

    def want(i, status):
        if m[i].good and status != 0:
            return "zlib and the footer accept it, device status %d" % status
        if not m[i].good and status == 0:
            return "zlib or the footer refuse it, device status 0"

    check_sandwiches(gpu_ctx, m, want)
