"""Shared inputs of the MD synthesis tests (tests/test_ref.py, test_ref_gpu.py)
-- TEST INFRASTRUCTURE: the MD rule of DESIGN.md transcribed in Python, the
hand-made read set, FASTA writing and MD stripping."""
from __future__ import annotations

import struct

import numpy as np

LETTERS = b"=ACMGRSVTWYHKDBN"
NIB_OF = {ord("A"): 1, ord("C"): 2, ord("G"): 4, ord("T"): 8}


class PastEnd(Exception):
    pass


def py_md(pos, cigar, seq_nib, ref_nib) -> bytes:
    """The rule: seq_nib / ref_nib are unpacked nibble arrays."""
    x, y, u = int(pos), 0, 0
    out = bytearray()
    l_seq, n = len(seq_nib), len(ref_nib)
    for w in cigar:
        op, l = int(w) & 15, int(w) >> 4
        if op in (0, 7, 8):
            if x + l > n:
                raise PastEnd
            for j in range(l):
                c1 = int(seq_nib[y + j]) if y + j < l_seq else 15
                c2 = int(ref_nib[x + j])
                if c1 == 0 or (c1 == c2 and c1 != 15):
                    u += 1
                else:
                    out += str(u).encode() + LETTERS[c2:c2 + 1]
                    u = 0
            x += l
            y += l
        elif op == 2:
            if x + l > n:
                raise PastEnd
            out += str(u).encode() + b"^" + bytes(LETTERS[int(c)] for c in ref_nib[x:x + l])
            u = 0
            x += l
        elif op in (1, 4):
            y += l
        elif op == 3:
            x += l
    return bytes(out + str(u).encode())


def pack_nib(nib: np.ndarray) -> np.ndarray:
    nib = np.asarray(nib, np.uint8)
    if len(nib) % 2:
        nib = np.concatenate([nib, np.zeros(1, np.uint8)])
    return (nib[0::2] << 4 | nib[1::2]).astype(np.uint8)


def nib_of_text(s: bytes) -> np.ndarray:
    """A C G T U (either case) -> 1 2 4 8 8, anything else 15."""
    t = np.full(256, 15, np.uint8)
    for ch, v in ((b"A", 1), (b"C", 2), (b"G", 4), (b"T", 8), (b"U", 8)):
        t[ch[0]] = v
        t[ch.lower()[0]] = v
    return t[np.frombuffer(s, np.uint8)]


def batch_of(reads):
    """[(pos, [cigar u32], unpacked seq nibbles)] -> ReadAlnBatch without MD."""
    from pomfret_amd.abi import ReadAlnBatch
    start, end, cig, co, seq, so, sl = [], [], [], [0], [], [0], []
    for pos, cg, sq in reads:
        rl = sum(w >> 4 for w in cg if (w & 15) in (0, 2, 3, 7, 8))
        start.append(pos)
        end.append(pos + rl)
        cig += list(cg)
        co.append(len(cig))
        p = pack_nib(sq)
        seq.append(p)
        so.append(so[-1] + len(p))
        sl.append(len(sq))
    return ReadAlnBatch(start=np.array(start), end=np.array(end), cigar_off=np.array(co),
                        cigar=np.array(cig, np.uint32), seq_off=np.array(so), seq_len=np.array(sl),
                        seq=np.concatenate(seq) if seq else np.zeros(0, np.uint8),
                        md_off=np.zeros(len(reads) + 1), md=np.zeros(0, np.uint8))


def _other(rng, c):
    return int(rng.choice([v for v in (1, 2, 4, 8) if v != c]))


def build_read(rng, ref, pos, ops, mism=(), force=None):
    """ops [(op, len)]; mism: offsets among the read's M/=/X bases that get
    another base; force {query index: nibble}.  -> (pos, cigar, seq nibbles)."""
    x, m, seq = pos, 0, []
    mism = set(mism)
    for op, l in ops:
        if op in (0, 7, 8):
            for j in range(l):
                c = int(ref[x + j]) if x + j < len(ref) else 1
                if m + j in mism:
                    c = _other(rng, c)
                seq.append(c)
            x += l
            m += l
        elif op in (1, 4):
            seq += [int(v) for v in rng.choice([1, 2, 4, 8], l)]
        elif op in (2, 3):
            x += l
    seq = np.array(seq, np.uint8)
    for q, v in (force or {}).items():
        seq[q] = v
    return pos, [l << 4 | op for op, l in ops], seq


HAND_REF_LEN = 120_000


def hand_made(seed: int = 21):
    """The hand-made set on a 120,000-base reference: (unpacked reference
    nibbles, [(pos, cigar, seq nibbles)]).  Reference N at 3,500 / 3,501."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.array([1, 2, 4, 8], np.uint8), HAND_REF_LEN)
    ref[3_500] = 15
    ref[3_501] = 15
    ref[3_510] = 1
    R = []
    # every op code 0-8, with H and P in the middle of the CIGAR as well
    R.append(build_read(rng, ref, 500, [(5, 5), (4, 3), (0, 10), (1, 2), (0, 5), (2, 3), (0, 5), (3, 7), (7, 6), (8, 2),
                                        (6, 1), (0, 4), (4, 3), (5, 2)], mism=[3, 26, 27]))
    # a leading and a trailing mismatch
    R.append(build_read(rng, ref, 1_000, [(0, 50)], mism=[0, 49]))
    # three mismatches in a row, at a 64-base step boundary too
    R.append(build_read(rng, ref, 1_200, [(0, 200)], mism=[10, 11, 12, 63, 64, 65, 127, 128]))
    # a mismatch right after an insertion and right after a deletion
    R.append(build_read(rng, ref, 2_000, [(0, 20), (1, 3), (0, 20), (2, 4), (0, 20)], mism=[20, 40]))
    # deletion, 1M, deletion (the M a match, then a mismatch); deletions back to back
    R.append(build_read(rng, ref, 3_000, [(0, 10), (2, 2), (0, 1), (2, 3), (0, 10)]))
    R.append(build_read(rng, ref, 3_100, [(0, 10), (2, 2), (0, 1), (2, 3), (0, 10)], mism=[10]))
    R.append(build_read(rng, ref, 3_200, [(0, 10), (2, 2), (2, 3), (0, 10)]))
    # a 300-base deletion, and one as the first and as the last op
    R.append(build_read(rng, ref, 4_000, [(0, 30), (2, 300), (0, 30)], mism=[30]))
    R.append(build_read(rng, ref, 5_000, [(2, 70), (0, 30), (2, 65)]))
    # an N skip between matches
    R.append(build_read(rng, ref, 6_000, [(0, 40), (3, 1_000), (0, 40)], mism=[39, 40]))
    # a read '=' nibble (always a match)
    R.append(build_read(rng, ref, 7_000, [(0, 30)], force={4: 0, 17: 0}))
    # a read N over reference A (3,510) and over reference N (3,500); a read A over reference N (3,501)
    R.append(build_read(rng, ref, 3_490, [(0, 40)], force={10: 15, 20: 15, 11: 1}))
    # match runs of 99, 100, 9,999 and 10,000 between mismatches, and one of 100,000
    at, mm = 0, []
    for r in (99, 100, 9_999, 10_000):
        at += r
        mm.append(at)
        at += 1
    R.append(build_read(rng, ref, 8_000, [(0, at + 5)], mism=mm))
    R.append(build_read(rng, ref, 15_000, [(0, 100_002)], mism=[0, 100_001]))
    # a CIGAR of 5,000 ops alternating 1M1I
    R.append(build_read(rng, ref, 9_000, [(0, 1), (1, 1)] * 2_500, mism=[0, 63, 64, 65, 700, 2_499]))
    # l_seq = 0 (SEQ '*'): every base reads as 15
    R.append((10_000, [20 << 4 | 0, 2 << 4 | 2, 5 << 4 | 0], np.zeros(0, np.uint8)))
    # SEQ shorter than the CIGAR's query length
    R.append((10_100, [30 << 4 | 0], np.array([int(v) for v in ref[10_100:10_110]], np.uint8)))
    # no CIGAR at all; an M that ends exactly at the contig's end
    R.append((11_000, [], np.zeros(0, np.uint8)))
    R.append(build_read(rng, ref, HAND_REF_LEN - 100, [(0, 100)], mism=[99]))
    return ref, R


def hand_expected():
    ref, R = hand_made()
    mds = [py_md(pos, cg, sq, ref) for pos, cg, sq in R]
    off = np.concatenate([[0], np.cumsum([len(m) for m in mds])]).astype(np.uint64)
    return ref, batch_of(R), off, np.frombuffer(b"".join(mds), np.uint8), mds


def u_batch(hac: bool):
    """The 200-read batch of the issue (SUP- or HAC-like errors): (known, reads,
    unpacked reference nibbles); the reference is the generator's first draw."""
    from pomfret_amd.synth_u import BASES, NIB, USpec, make_u_batch
    kw = dict(sub_err=0.02, indel_err=0.01) if hac else {}
    spec = USpec(ref_len=60_000, n_reads=200, mean_len=3_000, **kw)
    known, reads, _ = make_u_batch(spec)
    ref = BASES[np.random.default_rng(spec.seed).integers(0, 4, spec.ref_len)]      # the generator's first draw
    nib = np.zeros(spec.ref_len, np.uint8)
    for b, v in NIB.items():
        nib[ref == b] = v
    return known, reads, nib


def past_end(ref):
    """One read whose M runs one base past the contig's end."""
    rng = np.random.default_rng(3)
    return [build_read(rng, ref, len(ref) - 50, [(0, 51)])]


def write_fasta(path, contigs, width=60, eol="\n", gz=False, last_newline=True):
    """contigs [(header text after '>', sequence bytes)]; width 0: one line."""
    out = bytearray()
    for hdr, s in contigs:
        out += b">" + hdr.encode() + eol.encode()
        step = width or max(len(s), 1)
        for i in range(0, len(s), step):
            out += s[i:i + step] + eol.encode()
    if not last_newline and out.endswith(eol.encode()):
        out = out[:len(out) - len(eol)]
    if gz:
        import gzip
        with gzip.open(path, "wb") as f:
            f.write(bytes(out))
    else:
        with open(path, "wb") as f:
            f.write(bytes(out))


def strip_md(aux: bytes) -> bytes:
    """The aux block without its MD tag."""
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    o, out = 0, bytearray()
    while o < len(aux):
        tag, ty = aux[o:o + 2], chr(aux[o + 2])
        p = o + 3
        if ty in size:
            p += size[ty]
        elif ty in "ZH":
            p = aux.index(b"\0", p) + 1
        elif ty == "B":
            sub = chr(aux[p])
            n = struct.unpack_from("<I", aux, p + 1)[0]
            p += 5 + n * size[sub]
        else:
            raise ValueError(ty)
        if tag != b"MD":
            out += aux[o:p]
        o = p
    return bytes(out)


def stripped(recs):
    import copy
    out = []
    for r in recs:
        r2 = copy.copy(r)
        r2.aux = strip_md(r.aux)
        out.append(r2)
    return out
