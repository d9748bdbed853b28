"""Hand-built records for the K0 row and tile tests, and their comparison
with the oracle loader.

Reads are "CG" repeats (an odd length ends in a C), so every C of a forward
read and every stored G of a reverse read (the original read's C's, counted
from the stored end) is in CpG context, except at the read's two ends.  Calls
are given as stored read positions and turned into the MM skip counts here,
which lets a case name the base a trigger sits on.
"""
import numpy as np

from tests._aln_cases import LOAD_CFG_SMALL, records_batch

NONE = 0xFFFFFFFF


def cg_read(n):
    return ("CG" * (n // 2 + 1))[:n]


def callable_positions(seq, rev):
    """Stored positions whose call is kept as an explicit CpG call: a C with a
    G after it (forward), a G with a C before it (reverse), not the read's
    first or last base."""
    n = len(seq)
    if rev:
        return [p for p in range(1, n - 1) if seq[p] == "G" and seq[p - 1] == "C"]
    return [p for p in range(1, n - 1) if seq[p] == "C" and seq[p + 1] == "G"]


def skips_of(seq, rev, positions):
    """MM skip counts that call the target bases at these stored positions."""
    tgt = "G" if rev else "C"
    at = [p for p in range(len(seq)) if seq[p] == tgt]
    if rev:
        at.reverse()
    rank = {p: k for k, p in enumerate(at)}
    ranks = sorted(rank[p] for p in set(positions))
    return np.diff(np.concatenate([[-1], ranks])) - 1


def record(seq, cigar, positions, rev, pos, seed, hdr="C+m?"):
    sk = skips_of(seq, rev, positions)
    ml = np.random.default_rng(seed).integers(0, 256, len(sk)).tolist()
    mm = hdr + "".join("," + str(x) for x in sk.tolist()) + ";"
    return dict(seq=seq, cigar=cigar, mm=mm, ml=ml, pos=pos, flag=16 if rev else 0)


def spread(cands, must, n):
    """n positions of cands: every one of must, the rest evenly spread."""
    must = sorted(set(must))
    assert set(must) <= set(cands) and len(must) <= n <= len(cands)
    out = set(must)
    for p in (cands[int(i)] for i in np.linspace(0, len(cands) - 1, 4 * n)):
        if len(out) == n:
            break
        out.add(p)
    assert len(out) == n
    return sorted(out)


def batch_of(recs):
    return records_batch([(0, 1 << 28, recs)])


def oracle_view(oracle_lib, recs, lcfg=LOAD_CFG_SMALL):
    """The oracle's reads of the records: (batch, record -> read, calls per read)."""
    b, rec_read = oracle_lib.load_reads(lcfg, batch_of(recs))
    return b, rec_read, np.diff(b.read_call_off.astype(np.int64))


def check(oracle_lib, gpu_ctx, recs, tag, dropped=(), lcfg=LOAD_CFG_SMALL, **want):
    """The records through K0 against the oracle, record by record: kept
    records, call offsets, positions, categories, first and last call, read
    start and end, and the loader's counters (`want`; bad_mm and multi_cm are 0
    unless given).  Every record but those at the indices in `dropped` must be
    kept by the oracle, with at least one call."""
    from pomfret_amd import Config
    aln = batch_of(recs)
    b, rec_read = oracle_lib.load_reads(lcfg, aln)
    kept = rec_read != NONE
    assert np.flatnonzero(~kept).tolist() == sorted(dropped), f"{tag}: the oracle's kept records"
    co = b.read_call_off.astype(np.int64)
    assert b.n_reads > 0 and (np.diff(co) > 0).all(), f"{tag}: a kept record without a call"
    pos, cat = b.call_pos.copy(), b.call_cat.copy()
    first = np.zeros(b.n_reads, np.uint32)
    last = np.zeros(b.n_reads, np.uint32)
    for r in range(b.n_reads):
        s = slice(co[r], co[r + 1])
        first[r], last[r] = b.call_pos[co[r]], b.call_pos[co[r + 1] - 1]
        o = np.lexsort((cat[s], pos[s]))
        pos[s], cat[s] = pos[s][o], cat[s][o]
    db = gpu_ctx.upload_aln(Config(), aln, lcfg)
    try:
        off, gpos, gcat, gfirst, glast = db.debug_calls()
        assert np.array_equal(db.read_recs(), np.flatnonzero(kept)), f"{tag}: kept records"
        assert np.array_equal(off, b.read_call_off), f"{tag}: call offsets"
        assert np.array_equal(gpos, pos), f"{tag}: positions differ at {np.flatnonzero(gpos != pos)[:5].tolist()}"
        assert np.array_equal(gcat, cat), f"{tag}: categories"
        assert np.array_equal(gfirst, first) and np.array_equal(glast, last), f"{tag}: first / last call"
        gstart, gend = db.debug_spans()
        assert np.array_equal(gstart, b.read_start), f"{tag}: read starts"
        assert np.array_equal(gend, b.read_end), f"{tag}: read ends differ at {np.flatnonzero(gend != b.read_end)[:5].tolist()}"
        c0 = db.load_counters()                          # the counters add up over the runs: one more run's increase
        db.debug_calls()
        c = {k: v - c0[k] for k, v in db.load_counters().items()}
        for k, v in dict(dict(bad_mm=0, multi_cm=0), **want).items():
            assert c[k] == v, f"{tag}: {k} {c[k]} != {v}"
        return b, rec_read
    finally:
        db.free()
