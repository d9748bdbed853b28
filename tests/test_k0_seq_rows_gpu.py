"""K0's SEQ pass at the edges of its rows, row pairs and blocks.

The pass reads a record's SEQ in blocks of 8 rows of 128 16-base words (2,048
bases a row, 16,384 a block) and counts the target bases of two rows per wave
scan; a forward read's blocks are walked from the start and a reverse read's
from the end.  Rows past the read hold no target, and a pair of them may be
skipped whole.  The lengths below end a read on a row, a row-pair and a block
edge and one base either side, odd lengths included, so that the last block
holds 1 to 8 rows with the last one full, one base short or one base long.

Every batch is compared record by record with oracle.load_reads (kept
records, call offsets, positions, categories, first and last call, read start
and end, loader counters: tests/_k0_cases.check).
"""
import numpy as np
import pytest

from tests._k0_cases import NONE, callable_positions, cg_read, check, oracle_view, record, spread

LENGTHS = [2047, 2048, 2049, 4095, 4096, 4097, 14337, 16383, 16384, 16385, 18433, 20481]
ROW = 2048


def edge_record(n, rev, k):
    """40 calls on a read of n bases: the first and the last callable base
    (forward: the read's second C and its last CpG; reverse: the same of the
    original read, at the stored read's other end), and the bases either side
    of the last row edge inside the read -- forward the C whose G is the row's
    last base and the C that is the next row's first base, reverse the G that
    is the row's last base and the G whose C is the next row's first."""
    seq = cg_read(n)
    cands = callable_positions(seq, rev)
    e = (n - 1) // ROW * ROW                             # first base of the last row that holds any
    beside = {p for p in ((e - 1, e + 1) if rev else (e - 2, e)) if p in cands} if e else set()
    assert bool(beside) == bool(e)                       # a read with a row edge inside has a call beside it
    must = {cands[0], cands[-1]} | beside
    return record(seq, f"{n}M", spread(cands, must, 40), rev, 1000 + 30_000 * k, seed=n + rev)


def length_records():
    return [edge_record(n, rev, 2 * i + rev) for i, n in enumerate(LENGTHS) for rev in (False, True)]


def test_lengths_are_kept_by_the_oracle(oracle_lib):
    _, rec_read, n_calls = oracle_view(oracle_lib, length_records())
    assert (rec_read != NONE).all()
    assert n_calls.tolist() == [40] * (2 * len(LENGTHS))


@pytest.mark.gpu
def test_row_pair_and_block_edges(oracle_lib, gpu_ctx):
    b, _ = check(oracle_lib, gpu_ctx, length_records(), "row edges")
    assert b.n_reads == 2 * len(LENGTHS)


@pytest.mark.gpu
def test_triggers_end_before_the_last_block(oracle_lib, gpu_ctx):
    """Three blocks of SEQ, every call inside the first one the pass reads
    (forward: the read's start; reverse: the stored read's end): the pass
    stops once the list is placed and never counts the other blocks."""
    recs = []
    for rev in (False, True):
        seq = cg_read(40_001)
        cands = [p for p in callable_positions(seq, rev) if (p > 30_100 if rev else p < 9_900)]
        recs.append(record(seq, "40001M", spread(cands, {cands[0], cands[-1]}, 40), rev, 1000 + 50_000 * rev, seed=rev))
    check(oracle_lib, gpu_ctx, recs, "early end")


@pytest.mark.gpu
def test_trigger_list_in_hbm(oracle_lib, gpu_ctx):
    """More than 640 calls: the ranks and triggers live in the record's HBM
    slice, over a last block of two rows and one base."""
    recs = []
    for rev in (False, True):
        seq = cg_read(20_481)
        cands = callable_positions(seq, rev)
        recs.append(record(seq, "20481M", spread(cands, {cands[0], cands[-1], cands[len(cands) // 2]}, 700), rev,
                           1000 + 30_000 * rev, seed=7 + rev))
    b, _ = check(oracle_lib, gpu_ctx, recs, "hbm list")
    assert np.diff(b.read_call_off.astype(np.int64)).tolist() == [700, 700]
