"""K0's CIGAR walk at the edges of its tiles and of its trigger passes.

The walk takes the CIGAR a tile of operations at a time (64, or 128 in the
explicit walk) and, inside a tile, the triggers that end in it 64 per pass.
The CIGARs below are `4M 2I 4M 2D` repeated to 63..300 operations, so a tile
edge falls on each of the four operations, and a call sits on every CpG C but
the first: on the first and third base of every M (forward) or its second and
last (reverse), inside every insertion (dropped) and right after every
deletion.  One call per operation survives, hence about as many calls as
operations.

Two calls of one C m entry cannot map to one reference position in the
explicit walk: a trigger on an operation's end belongs to that operation, the
next M's first own trigger is at least one base past its start, and an
insertion moves the offset back by exactly its length, so positions stay
strictly increasing.  What the tile and pass edges can get wrong is the
neighbour test itself, so the cases put calls one reference base apart (a
trigger on an M's end before an insertion, and the next M's first) across a
pass edge and across a tile edge instead.

Every batch is compared record by record with oracle.load_reads (kept
records, call offsets, positions, categories, first and last call, read start
and end, loader counters: tests/_k0_cases.check).
"""
import numpy as np
import pytest

from tests._aln_cases import LOAD_CFG_SMALL, records_batch
from tests._k0_cases import NONE, callable_positions, cg_read, check, oracle_view, record

N_OPS = [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300]
UNIT = [(4, "M"), (2, "I"), (4, "M"), (2, "D")]


def pattern(n, unit=UNIT):
    return [unit[i % len(unit)] for i in range(n)]


def qlen(ops):
    return sum(n for n, op in ops if op in "MIS=X")


def text(ops):
    return "".join(f"{n}{op}" for n, op in ops)


def full_record(ops, rev, k, seed=0, keep=lambda p: True, hdr="C+m?", seq=None):
    """The operations over a CG read, a call on every callable base that `keep` takes."""
    seq = seq or cg_read(qlen(ops))
    at = [p for p in callable_positions(seq, rev) if keep(p)]
    return record(seq, text(ops), at, rev, 1000 + 3000 * k, seed, hdr=hdr)


def pattern_records():
    return [full_record(pattern(n), rev, 2 * i + rev, seed=n) for i, n in enumerate(N_OPS) for rev in (False, True)]


def test_patterns_are_kept_by_the_oracle(oracle_lib):
    _, rec_read, n_calls = oracle_view(oracle_lib, pattern_records())
    assert (rec_read != NONE).all()
    assert n_calls.min() >= 63 and n_calls.max() <= 301
    assert (np.abs(n_calls - np.repeat(N_OPS, 2)) <= 2).all()       # one call per operation, give or take the ends


@pytest.mark.gpu
def test_operation_counts_around_the_tiles(oracle_lib, gpu_ctx):
    check(oracle_lib, gpu_ctx, pattern_records(), "patterns")


@pytest.mark.gpu
def test_trigger_counts_around_the_passes(oracle_lib, gpu_ctx):
    """63..129 triggers that end in one tile: a CIGAR of 120 operations and the
    first k callable bases, then 8 long operations more with no trigger."""
    recs = []
    for i, k in enumerate([63, 64, 65, 127, 128, 129]):
        for rev in (False, True):
            ops = pattern(120) + pattern(8, [(6, "M"), (3, "D")])
            seq = cg_read(qlen(ops))
            at = callable_positions(seq, rev)
            at = at[:k]
            assert at[-1] < qlen(pattern(120))
            recs.append(record(seq, text(ops), at, rev, 1000 + 3000 * (2 * i + rev), seed=k))
    check(oracle_lib, gpu_ctx, recs, "pass edges")


@pytest.mark.gpu
def test_neighbouring_positions_across_pass_and_tile_edges(oracle_lib, gpu_ctx):
    """`4M 1I` repeated: the call on an M's end (the inserted base) and the
    next M's second base are one reference base apart.  With every such pair
    called and the pattern moved along the read two bases at a time, pairs
    straddle the 64th and 128th trigger and the 64th and 128th operation."""
    recs = []
    for rev in (False, True):
        for lead in (2, 4, 6, 8, 10):
            ops = [(lead, "M")] + pattern(200, [(4, "M"), (1, "I")]) + [(6, "M")]
            recs.append(full_record(ops, rev, len(recs), seed=lead))
    b, _ = check(oracle_lib, gpu_ctx, recs, "neighbours", dup_chunks=0)
    co = b.read_call_off.astype(np.int64)
    for r in range(b.n_reads):
        assert (np.diff(np.sort(b.call_pos[co[r]:co[r + 1]])) == 1).sum() >= 30


@pytest.mark.gpu
def test_leading_soft_clip(oracle_lib, gpu_ctx):
    """A call on the clip's last base (dropped) and on the first aligned base
    (pushed at the read's start by the prologue), each where the base is
    callable: 4S puts a forward C on the first aligned base and a reverse G on
    the clip's last, 5S the other way round.  Then the stale-trigger case:
    every call inside the clip, walked by lane 0."""
    recs = []
    for clip in (4, 5):
        for rev in (False, True):
            ops = [(clip, "S")] + pattern(130)
            recs.append(full_record(ops, rev, len(recs), seed=clip))
            assert {clip - 1, clip} & set(callable_positions(cg_read(qlen(ops)), rev))
    for rev in (False, True):
        ops = [(8, "S")] + pattern(130)
        recs.append(full_record(ops, rev, len(recs), seed=9, keep=lambda p: p <= 7))
    check(oracle_lib, gpu_ctx, recs, "soft clip", seq_path=2)


STOPS = [62, 63, 64, 65, 126, 127, 128, 129]


@pytest.mark.gpu
@pytest.mark.parametrize("stop", ["N", "S"])
def test_stop_at_each_tile_edge(oracle_lib, gpu_ctx, stop):
    """N (more operations and calls follow it: none is taken) and a trailing
    S (calls inside it: none is taken) as operation 62..129."""
    recs = []
    for k in STOPS:
        for rev in (False, True):
            ops = pattern(k) + ([(100, "N")] + pattern(70) if stop == "N" else [(9, "S")])
            recs.append(full_record(ops, rev, len(recs), seed=k))
    b, _ = check(oracle_lib, gpu_ctx, recs, f"stop {stop}")
    n_calls = np.diff(b.read_call_off.astype(np.int64))
    assert (np.abs(n_calls - np.repeat(STOPS, 2)) <= 2).all()       # the calls before the stop alone


FATAL_OPS = [(3, "H"), (2, "="), (2, "X"), (1, "P")]


@pytest.mark.gpu
def test_other_operations_after_the_stop_are_ignored(oracle_lib, gpu_ctx):
    """H, =, X and P past an N: in the stop's tile (the next operation, and
    the next lane) and in later tiles, with and without triggers left."""
    recs = []
    for k in (3, 62, 63, 64, 126, 127, 128):
        for j, bad in enumerate(FATAL_OPS):
            for gap in (0, 1, 140):
                ops = pattern(k) + [(50, "N")] + pattern(gap) + [bad] + pattern(5)
                rev = bool((k + j + gap) & 1)
                # with gap 140 every other record has no call past the stop
                keep = (lambda p, lim=qlen(pattern(k)): p < lim) if (gap == 140 and j & 1) else (lambda p: True)
                recs.append(full_record(ops, rev, len(recs), seed=k, keep=keep))
    check(oracle_lib, gpu_ctx, recs, "after the stop")


@pytest.mark.gpu
@pytest.mark.parametrize("where", [3, 63, 64, 70, 127, 128, 129, 200])
def test_other_operations_before_the_stop_are_fatal(gpu_ctx, where):
    """H, =, X and P as operation `where`, before any stop: the run ends in an
    error (the reference exits), whether triggers are left at that tile or
    not (the calls of the second record end inside the first ten operations),
    and whether a stop follows in the same tile or not."""
    from pomfret_amd import Config, PomfretError
    for j, bad in enumerate(FATAL_OPS):
        for early in (False, True):
            ops = pattern(where) + [bad] + ([(50, "N")] if j & 1 else []) + pattern(60)
            rec = full_record(ops, bool(j & 1) != early, 0, seed=where,
                              keep=(lambda p: p < 24) if early else (lambda p: True))
            db = gpu_ctx.upload_aln(Config(), records_batch([(0, 1 << 28, [rec])]), LOAD_CFG_SMALL)
            try:
                with pytest.raises(PomfretError):
                    db.debug_calls()
            finally:
                db.free()


@pytest.mark.gpu
def test_read_end_counts_the_tiles_past_the_last_trigger(oracle_lib, gpu_ctx):
    """Calls in the first operations only, then up to 300 operations more
    (bam_endpos sums them all), with and without an N among them (it counts
    too, and the operations after it)."""
    recs = []
    for n in (64, 65, 128, 129, 193, 257, 300):
        for rev in (False, True):
            tail = pattern(n, [(5, "M"), (3, "D"), (1, "I")])
            if n & 1:
                tail[n // 2] = (77, "N")
            ops = pattern(6) + tail
            recs.append(full_record(ops, rev, len(recs), seed=n, keep=lambda p: p < 20))
    b, _ = check(oracle_lib, gpu_ctx, recs, "read end")
    want = [r["pos"] + sum(n for n, op in [(int(x[:-1]), x[-1]) for x in _split(r["cigar"])] if op in "MDN") for r in recs]
    assert b.read_end.tolist() == want


def _split(cigar):
    import re
    return re.findall(r"\d+[MIDNSHP=X]", cigar)


@pytest.mark.gpu
def test_implicit_multi_and_hbm_records(oracle_lib, gpu_ctx):
    """129 operations on an implicit-canonical read (`C+m.` with a call on a
    C before an A: tiles of 64 and the chunk merge), 129 operations on a
    record with two C m entries (pf_k0_multi), and more than 640 calls over
    257 operations (the HBM trigger list)."""
    recs = []
    for rev in (False, True):
        ops = pattern(129)
        seq = cg_read(qlen(ops))
        seq = seq[:202] + "TG" + seq[204:] if rev else seq[:200] + "CA" + seq[202:]
        assert seq[202:204] == "TG" if rev else seq[200:202] == "CA"    # a called G after a T / C before an A
        at = [p for p in callable_positions(seq, rev) if p % 6 < 2] + [203 if rev else 200]
        recs.append(record(seq, text(ops), at, rev, 1000 + 3000 * len(recs), seed=rev, hdr="C+m."))
    for rev in (False, True):
        ops = pattern(129)
        seq = cg_read(qlen(ops))
        at = callable_positions(seq, rev)
        a = record(seq, text(ops), at[::2], rev, 1000 + 3000 * len(recs), seed=3)
        b_ = record(seq, text(ops), at[1::3], rev, 0, seed=4, hdr="C-m?")
        a["mm"], a["ml"] = a["mm"] + b_["mm"], a["ml"] + b_["ml"]
        recs.append(a)
    for rev in (False, True):
        ops = pattern(257, [(12, "M"), (2, "I"), (12, "M"), (2, "D")])
        recs.append(full_record(ops, rev, len(recs), seed=5))
    b, _ = check(oracle_lib, gpu_ctx, recs, "implicit, multi, hbm", implicit=2, multi_cm=2)
    assert (np.diff(b.read_call_off.astype(np.int64))[4:] > 640).all()
