"""K0's MM pass and its late scalar fields against the oracle loader, on
hand-built records at the smallest shapes where the parse can go wrong.

K0 reads the MM text as aligned 4-byte words, 64 words (a 256-byte row) per
step, and the texts of a batch are concatenated, so a text starts at any of
the four byte offsets of a word (its misalignment, set by the lengths of the
texts before it).  The cases put the C m entry's header and its ';' on every
byte of a word and on the first and last lane of a row, vary the text length
around one, two and four rows, the entry's place in the tag, and the list
length around the wave's rank batch (64) and its LDS list (640, past which the
record's HBM slice is used), forward and reverse.  Malformed texts must be
dropped for the same records as the oracle drops, and counted.

Every batch is compared record by record with oracle.load_reads: kept
records, call offsets, positions, categories, first and last call; the
loader's counters are compared with what the records were built to be (the
oracle keeps no counters).
"""
import numpy as np
import pytest

from tests._aln_cases import LOAD_CFG_SMALL, records_batch

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


# --------------------------------------------------------------------------
# record builders.  Every read is "CG" repeated: each C (forward) and each
# stored G (reverse: the original read's C's, counted from the end) is in CpG
# context, so every call of a well-formed tag is kept.
def skips_for(nd, seed):
    """nd skip counts 0..2 (1-digit) with a few 2- and 3-digit ones; the
    first at least 1, so that every count gives a call."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 3, nd)
    big = rng.random(nd) < 0.05
    s[big] = rng.integers(10, 130, int(big.sum()))
    s[0] = max(s[0], 1)                      # the read's first C is never a call (no base before / after it)
    return s.tolist()


def entry(hdr, skips, end=";"):
    return hdr + "".join("," + str(x) for x in skips) + end


def entry_of_len(hdr, total, seed=0):
    """A whole entry (header, counts, ';') of exactly `total` bytes and the
    number of counts in it: 1-digit counts, the last one padded with leading
    zeros to reach the length."""
    body = total - len(hdr) - 1
    assert body >= 2, total
    k = body // 2
    sk = [str(x) for x in np.random.default_rng(seed).integers(0, 3, k)]
    sk[-1] = "0" * (body - 2 * k) + sk[-1]
    txt = hdr + "".join("," + x for x in sk) + ";"
    assert len(txt) == total
    return txt, [int(x) for x in sk]


def n_pairs(*skip_lists):
    """CG pairs a read needs for the longest of the skip lists, and a few more."""
    return max(sum(s) + len(s) for s in skip_lists) + 3


class Batch:
    """Records of one window list, with the byte offset of every MM text in the
    batch's concatenated MM array (which sets the text's misalignment)."""

    def __init__(self):
        self.wins = [[]]
        self.tot = 0
        self.bad = 0                         # records built with an undecodable MM/ML
        self.multi = 0                       # records built with several C m entries
        self.where = []                      # (misalignment, text) of the records under test

    def filler(self, mis):
        """A plain kept record whose text length moves the next text to `mis`."""
        z = (mis - self.tot - 7) % 4
        self.add("C+m?," + "0" * z + "1;", [200], 4, note=False)
        assert self.tot % 4 == mis

    def add(self, mm, ml, pairs, rev=False, bad=False, multi=False, note=True, cigar=None, seq=None, win=0):
        seq = seq if seq is not None else "CG" * max(pairs, 4)
        rec = dict(seq=seq, cigar=f"{len(seq)}M" if cigar is None else cigar, mm=mm, ml=ml,
                   pos=1000 + 4000 * sum(len(w) for w in self.wins), flag=16 if rev else 0)
        while len(self.wins) <= win:
            self.wins.append([])
        self.wins[win].append(rec)
        if note:
            self.where.append((self.tot % 4, mm))
        self.tot += len(mm)
        self.bad += bad
        self.multi += multi

    def at(self, mis, *a, **kw):
        self.filler(mis)
        self.add(*a, **kw)

    def aln(self):
        return records_batch([(10_000_000 * i, 10_000_000 * (i + 1), w) for i, w in enumerate(self.wins)])


def check(oracle_lib, gpu_ctx, B, tag, lcfg=LOAD_CFG_SMALL, **want):
    """The batch through K0 against the oracle; `want` holds counter values."""
    from pomfret_amd import Config
    aln = B.aln()
    b, rec_read = oracle_lib.load_reads(lcfg, aln)
    co = b.read_call_off.astype(np.int64)
    pos, cat = b.call_pos.copy(), b.call_cat.copy()
    first = np.zeros(b.n_reads, np.uint32)
    last = np.zeros(b.n_reads, np.uint32)
    for r in range(b.n_reads):
        s = slice(co[r], co[r + 1])
        if co[r + 1] > co[r]:
            first[r], last[r] = b.call_pos[co[r]], b.call_pos[co[r + 1] - 1]
        o = np.lexsort((cat[s], pos[s]))
        pos[s], cat[s] = pos[s][o], cat[s][o]
    db = gpu_ctx.upload_aln(Config(), aln, lcfg)
    try:
        off, gpos, gcat, gfirst, glast = db.debug_calls()
        assert np.array_equal(db.read_recs(), np.flatnonzero(rec_read != NONE)), f"{tag}: kept records"
        assert np.array_equal(off, b.read_call_off), f"{tag}: call offsets"
        assert np.array_equal(gpos, pos), f"{tag}: positions differ at {np.flatnonzero(gpos != pos)[:5].tolist()}"
        assert np.array_equal(gcat, cat), f"{tag}: categories"
        assert np.array_equal(gfirst, first) and np.array_equal(glast, last), f"{tag}: first / last call"
        assert np.array_equal(np.diff(b.win_read_off.astype(np.int64)),
                              np.bincount(np.searchsorted(aln.win_rec_off[1:], db.read_recs(), side="right"),
                                          minlength=aln.n_windows)), f"{tag}: window read counts"
        # the counters add up over the loader's runs: one more run's increase
        c0 = db.load_counters()
        db.debug_calls()
        c = {k: v - c0[k] for k, v in db.load_counters().items()}
        assert c["bad_mm"] == B.bad, f"{tag}: bad_mm {c['bad_mm']} != {B.bad}"
        assert c["multi_cm"] == B.multi, f"{tag}: multi_cm {c['multi_cm']} != {B.multi}"
        for k, v in want.items():
            assert c[k] == v, f"{tag}: {k} {c[k]} != {v}"
        return b, rec_read
    finally:
        db.free()


# --------------------------------------------------------------------------
# 1. row and word geometry
def cm_tag(pre_len, cm_end, seed, hdr="C+m?", end=";"):
    """A `C+h?` entry of pre_len bytes (none when 0), then the C m entry with
    its ';' at text offset cm_end (or, without one, its last byte there)."""
    pre, psk = entry_of_len("C+h?", pre_len, seed) if pre_len else ("", [])
    cm, csk = entry_of_len(hdr, cm_end + 1 - pre_len, seed + 1)
    if not end:
        cm = cm[:-1]
    rng = np.random.default_rng(seed + 2)
    ml = rng.integers(0, 256, len(psk) + len(csk)).tolist()
    return pre + cm, ml, n_pairs(psk, csk)


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_header_and_semicolon_on_every_byte_and_row_edge(oracle_lib, gpu_ctx, mis):
    """The C m entry's header at the four byte offsets of a word and in the
    last and the first lane of a row (row offsets 252-259); its ';' likewise
    (251-260 and 507-516), for a text that starts at byte `mis` of a word."""
    B = Batch()
    seed = 100 * mis
    for hoff in [7, 8, 9, 10] + [o - mis for o in range(252, 260)]:
        for tail in range(4):                                   # the ';' on each byte of a word
            mm, ml, np_ = cm_tag(hoff, hoff + 12 + tail, seed := seed + 3)
            B.at(mis, mm, ml, np_, rev=bool(tail & 1))
    for e in [o - mis for o in list(range(251, 261)) + list(range(507, 517))]:
        for hoff in (0, 9):                                     # first entry, and after C+h?
            mm, ml, np_ = cm_tag(hoff, e, seed := seed + 3)
            B.at(mis, mm, ml, np_, rev=bool(e & 1))
    assert {m for m, _ in B.where} == {mis}
    heads = {(m + t.index("C+m")) & 3 for m, t in B.where} | {(m + t.rindex(";")) & 3 for m, t in B.where}
    lanes = {((m + t.index("C+m")) >> 2) & 63 for m, t in B.where} | {((m + t.rindex(";")) >> 2) & 63 for m, t in B.where}
    assert heads == {0, 1, 2, 3} and {0, 63} <= lanes
    _, rec_read = check(oracle_lib, gpu_ctx, B, f"geometry mis {mis}")
    assert (rec_read != NONE).all()


LENGTHS = [255, 256, 257, 511, 512, 513, 1023, 1024, 1025]


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_text_lengths_and_entry_order(oracle_lib, gpu_ctx, mis):
    """Texts of 255-1025 bytes (one, two and four rows, and a byte either
    side) with the C m entry first, second (after C+h?), third (after a ChEBI
    entry and C+h?), followed by a non-C entry, and without its final ';'."""
    B = Batch()
    seed = 1000 + 100 * mis
    rng = np.random.default_rng(seed)
    for N in LENGTHS:
        for lay in ("first", "second", "third", "then_other", "no_semicolon"):
            seed += 5
            parts = []                                           # (text, counts) in tag order
            if lay == "third":
                parts.append(entry_of_len("C+76792?", 40, seed))
            if lay in ("second", "third"):
                parts.append(entry_of_len("C+h?", N // 3, seed + 1))
            post = ("A+a?,1,2;", [1, 2]) if lay == "then_other" else None
            used = sum(len(t) for t, _ in parts) + (len(post[0]) if post else 0)
            cm, csk = entry_of_len("C+m?", N - used + (1 if lay == "no_semicolon" else 0), seed + 2)
            parts.append((cm[:-1], csk) if lay == "no_semicolon" else (cm, csk))
            if post:
                parts.append(post)
            mm = "".join(t for t, _ in parts)
            assert len(mm) == N
            ml = rng.integers(0, 256, sum(len(s) for _, s in parts)).tolist()
            B.at(mis, mm, ml, n_pairs(*[s for t, s in parts if t[0] == "C"]), rev=bool(seed & 1))
    _, rec_read = check(oracle_lib, gpu_ctx, B, f"lengths mis {mis}")
    assert (rec_read != NONE).all()


# --------------------------------------------------------------------------
# 2. list sizes: the rank batch (64), the reversal pivot (odd / even), the
# LDS list and the HBM slice
@pytest.mark.parametrize("rev", [False, True], ids=["fwd", "rev"])
def test_list_sizes(oracle_lib, gpu_ctx, rev):
    """nd of 1, 2, 63, 64, 65, 639, 640, 641 under C+h?;C+m? tags, whose ML
    length (2 nd) puts the upload's bound past 640 where nd is not: 639 and
    640 stay in the LDS list, 641 takes the record's HBM slice."""
    B = Batch()
    for k, nd in enumerate([1, 2, 63, 64, 65, 639, 640, 641]):
        hs, ms = skips_for(nd, 10 + k), skips_for(nd, 50 + k)
        ml = np.random.default_rng(90 + k).integers(0, 256, 2 * nd).tolist()
        B.at(k % 4, entry("C+h?", hs) + entry("C+m?", ms), ml, n_pairs(hs, ms), rev=rev)
    b, rec_read = check(oracle_lib, gpu_ctx, B, f"list sizes rev={rev}")
    kept = np.flatnonzero(rec_read != NONE)
    assert kept.size == 16                                       # the fillers and every record under test
    assert sorted(np.diff(b.read_call_off.astype(np.int64))[1::2].tolist()) == [1, 2, 63, 64, 65, 639, 640, 641]


# --------------------------------------------------------------------------
# 3. malformed text inside the C m entry
def long_cm(nd, seed):
    sk = skips_for(nd, seed)
    return "C+m?" + "".join("," + str(x) for x in sk) + ";", sk


@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_malformed_inside_the_cm_entry(oracle_lib, gpu_ctx, mis):
    """A stray byte at a row's first and at its last byte; a comma without a
    digit across a row boundary; 8-digit counts (the per-comma fallback), one
    of value 1 and one past the read; counts past the read's C's; an ML
    shorter than the entries need; bytes after the last count (ignored).
    Drops equal the oracle's; bad_mm counts the undecodable ones alone."""
    B = Batch()
    ML = lambda n, s: np.random.default_rng(s).integers(0, 256, n).tolist()  # noqa: E731

    def patched(seed, at_row_byte, make):
        """a 400-count entry, edited at the text byte that sits at row byte
        at_row_byte (256 = the second row's first byte)"""
        mm, sk = long_cm(400, seed)
        x = at_row_byte - mis
        while not (mm[x - 1].isdigit() and mm[x] == ","):        # the comma at or after the byte
            mm = mm[:5] + "0" + mm[5:]                           # one more leading zero moves the text on
        return make(mm, x), sk

    # a stray byte just before a comma, on the row's last / first byte
    for rb in (255, 256):
        mm, sk = patched(7 + rb, rb + 1, lambda t, x: t[:x - 1] + "x" + t[x:])
        assert mm[rb - mis] == "x"
        B.at(mis, mm, ML(len(sk), 1), n_pairs(sk), bad=True)
    # a stray byte in place of the row's first digit: ",x," is also a comma without a digit
    mm, sk = patched(31, 256, lambda t, x: t[:x - 1] + "x" + t[x:])
    B.at(mis, mm, ML(len(sk), 2), n_pairs(sk), bad=True)
    # ",," with the first comma on a row's last byte and the second on the next row's first
    mm, sk = patched(41, 255, lambda t, x: t[:x + 1] + t[x + 2:] if t[x + 2] == "," else t[:x + 1] + "," + t[x + 1:])
    assert mm[255 - mis:257 - mis] == ",,"
    B.at(mis, mm, ML(len(sk) + 1, 3), n_pairs(sk) + 2, bad=True)
    # 8-digit counts: value 1 (kept), and past the read (dropped, well-formed)
    sk = skips_for(90, 5)
    txt = [str(x) for x in sk]
    txt[40] = "00000001"
    sk[40] = 1
    B.at(mis, "C+m?," + ",".join(txt) + ";", ML(90, 4), n_pairs(sk), rev=True)
    txt[70] = "12345678"
    B.at(mis, "C+m?," + ",".join(txt) + ";", ML(90, 5), n_pairs(sk))
    # counts past the read's C's (well-formed: dropped, not counted)
    sk = skips_for(30, 6)
    B.at(mis, entry("C+m?", sk), ML(30, 6), sum(sk) + 20)
    B.at(mis, entry("C+m?", [5000]), [9], 8, rev=True)
    # ML shorter than the entries need
    sk = skips_for(70, 7)
    B.at(mis, entry("C+h?", sk) + entry("C+m?", sk), ML(139, 7), n_pairs(sk), bad=True)
    # bytes after the last count's digits are ignored
    B.at(mis, entry("C+m?", sk, end="x7;"), ML(70, 8), n_pairs(sk))
    B.at(mis, entry("C+m?", sk), ML(70, 9), n_pairs(sk), rev=True)     # and a plain one
    _, rec_read = check(oracle_lib, gpu_ctx, B, f"malformed mis {mis}")
    under_test = rec_read[1::2] != NONE                          # every other record is a filler
    assert (rec_read[0::2] != NONE).all()
    assert under_test.tolist() == [False, False, False, False, True, False, False, False, False, True, True]


# --------------------------------------------------------------------------
# 4. several C m entries: handed to pf_k0_multi
def test_second_cm_entry_is_handed_over(oracle_lib, gpu_ctx):
    """C+m?...;C-m?...; (short, long, forward, reverse, the second entry past
    a row): the main pass hands the record over, multi_cm counts it, and the
    merged calls equal the oracle's."""
    B = Batch()
    for k, (n1, n2) in enumerate([(1, 1), (3, 2), (64, 65), (150, 40), (300, 310), (639, 2)]):
        a, b_ = skips_for(n1, 20 + k), skips_for(n2, 40 + k)
        ml = np.random.default_rng(60 + k).integers(0, 256, n1 + n2).tolist()
        for rev in (False, True):
            B.at(k % 4, entry("C+m?", a) + entry("C-m?", b_), ml, n_pairs(a, b_), rev=rev, multi=True)
    _, rec_read = check(oracle_lib, gpu_ctx, B, "hand-over")
    assert (rec_read != NONE).all()


# --------------------------------------------------------------------------
# 5. the record's late fields (position, window, call slice, CIGAR, scratch
# slice) are read again at the walk and the epilogue
def late_field_records(B, win, k):
    sk = skips_for(700, 70 + k)
    ml = np.random.default_rng(80 + k).integers(0, 256, 700).tolist()
    # the HBM-list route: 700 calls
    B.add(entry("C+m?", sk), ml, n_pairs(sk), rev=bool(k), win=win)
    # implicit-canonical mode (a call outside CpG): bump-allocates from the arena's tail
    B.add("C+m?,1,0;", [220, 30], 0, seq="ACGACGTCAGCG" + "ACG" * k, win=win)
    # every call inside the leading soft clip: the lane-0 walk
    B.add("C+m?,0;", [250], 0, seq="ACGAAAAAA" + "A" * k, cigar=f"3S{6 + k}M", win=win)
    # ... and with implicit mode
    B.add("C+m?,0,0;", [200, 200], 0, seq="ACGACAACGAA", cigar="5S6M", win=win)
    # an empty CIGAR: dropped
    B.add("C+m?,0,0;", [200, 10], 0, seq="ACGTTCGA", cigar="", win=win)
    # plain reads either side, an insertion and a deletion in one
    B.add("C+m?,0,0,0;", [255, 0, 130], 0, seq="TTCGAACGTTACGA", cigar="2S4M1I2M2D5M", win=win)
    B.add(entry("C+m?", sk[:50]), ml[:50], n_pairs(sk[:50]), win=win)


def test_late_scalar_fields_in_two_windows(oracle_lib, gpu_ctx):
    B = Batch()
    for win in (0, 1):
        late_field_records(B, win, win)
    b, rec_read = check(oracle_lib, gpu_ctx, B, "late fields", implicit=4, seq_path=4, unsorted=0)
    assert np.diff(b.win_read_off.astype(np.int64)).tolist() == [6, 6]
    assert (rec_read != NONE).tolist() == [True, True, True, True, False, True, True] * 2


def test_unsorted_calls_take_the_sort_and_the_position_limit(gpu_ctx):
    """The only reads get_mod_poss_on_ref emits out of order are those whose
    first call wraps below position 0 (a reverse read at position 0 with a
    call on its first aligned base: 0 + cgoffset = 2^32 - 1), and such a
    position is past the 2^29 limit of the packed calls, which is an error of
    the run.  So the unsorted branch has no result to compare: the run must
    end in that error, after the sort has run on the record."""
    from pomfret_amd import Config, PomfretError
    aln = records_batch([(0, 1000, [dict(seq="GCGGCCCAGACCGCCC", cigar="2S11M3M", mm="C+m?,1,0,0;", ml=[200, 200, 200],
                                         pos=0, flag=16)])])
    db = gpu_ctx.upload_aln(Config(), aln, LOAD_CFG_SMALL)
    with pytest.raises(PomfretError):
        db.debug_calls()
    db.free()
