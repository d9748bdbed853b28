"""ctypes binding of libpomfret_amd.so (the product: HIP kernels + C ABI).

The library is built in-tree (pomfret_amd/libpomfret_amd.so, see
__graft_entry__.build()).  There is no CPU fallback: if the library or a GPU
is missing, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

from .abi import (DMR_HMM_SITES, DMR_RUN_DTYPE, REGION_SUM_DTYPE, PfRegions, HmmConfig, PfDmrHmm, PfDmrHmmCfg, AlnBatch, AssignConfig, PfAssign, PfAssignCfg, Config, DmrConfig, KnownVars, LoadConfig, PfAlnBatch, PfCfg, PfDmr, PfDmrCfg,
                  PfKnownVars, PfLoadCfg, PfPerm, PfPileup, PfRank, PfRankExact, PfReadAlnBatch, PfTagcheck, PfWindowBatch, PfWindowOut, ReadAlnBatch,
                  WindowBatch, WindowResult)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpomfret_amd.so")
_lib = None


class PomfretError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PomfretError(f"{LIB_PATH} not built: run __graft_entry__.build() or "
                               f"`make -C pomfret_amd/csrc`")
        L = C.CDLL(LIB_PATH)
        L.pf_abi_version.restype = C.c_int
        L.pf_device_count.restype = C.c_int
        L.pf_strerror.restype = C.c_char_p
        L.pf_strerror.argtypes = [C.c_int]
        L.pf_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.pf_ctx_destroy.argtypes = [C.c_void_p]
        L.pf_selftest.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.pf_batch_upload.argtypes = [C.c_void_p, C.POINTER(PfCfg), C.POINTER(PfWindowBatch),
                                      C.POINTER(C.c_void_p)]
        L.pf_batch_free.argtypes = [C.c_void_p]
        L.pf_batch_n_windows.argtypes = [C.c_void_p]
        L.pf_batch_n_windows.restype = C.c_uint32
        L.pf_batch_n_reads.argtypes = [C.c_void_p]
        L.pf_batch_n_reads.restype = C.c_uint32
        L.pf_batch_n_calls.argtypes = [C.c_void_p]
        L.pf_batch_n_calls.restype = C.c_uint64
        L.pf_methphase_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PfWindowOut)]
        L.pf_methphase_launch.argtypes = [C.c_void_p, C.c_void_p]
        L.pf_methphase_finish.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PfWindowOut)]
        L.pf_methphase_windows.argtypes = [C.c_int, C.POINTER(PfCfg), C.POINTER(PfWindowBatch),
                                           C.POINTER(PfWindowOut)]
        L.pf_last_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p),
                                           C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.pf_batch_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.pf_batch_heavy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.pf_batch_k3_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.pf_batch_k12_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.pf_batch_k3_budget.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.pf_batch_set_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.pf_batch_masked_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.pf_batch_debug_sites.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_uint32]
        L.pf_batch_debug_methmers.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint64]
        L.pf_batch_debug_methmers.restype = C.c_int64
        L.pf_fisher_exact.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_double)] * 3
        L.pf_fisher_exact.restype = C.c_double
        L.pf_batch_upload_aln.argtypes = [C.c_void_p, C.POINTER(PfCfg), C.POINTER(PfLoadCfg),
                                          C.POINTER(PfAlnBatch), C.POINTER(C.c_void_p)]
        L.pf_batch_read_recs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.pf_batch_debug_calls.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint64]
        L.pf_batch_debug_calls.restype = C.c_int64
        L.pf_batch_debug_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.pf_batch_load_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pf_batch_debug_recs.argtypes = [C.c_void_p] * 16
        L.pf_bgzf_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        L.pf_batch_pileup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.POINTER(C.POINTER(PfPileup))]
        L.pf_pileup_free.argtypes = [C.POINTER(PfPileup)]
        L.pf_write_hapmeth.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PfPileup), C.c_uint32, C.c_uint32, C.c_int]
        L.pf_dmr_regions.argtypes = [C.c_void_p, C.POINTER(PfPileup), C.c_uint32, C.c_uint32, C.POINTER(PfDmrCfg),
                                     C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(PfDmr))]
        L.pf_dmr_regions_block.argtypes = [C.c_void_p, C.POINTER(PfPileup), C.c_uint32, C.c_uint32, C.POINTER(PfDmrCfg),
                                           C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(PfDmr))]
        L.pf_dmr_free.argtypes = [C.POINTER(PfDmr)]
        L.pf_dmr_hmm_regions.argtypes = [C.c_void_p, C.POINTER(PfPileup), C.c_uint32, C.c_uint32, C.POINTER(PfDmrCfg),
                                         C.POINTER(PfDmrHmmCfg), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.POINTER(PfDmrHmm))]
        L.pf_dmr_hmm_free.argtypes = [C.POINTER(PfDmrHmm)]
        L.pf_dmr_hmm_evidence.argtypes = [C.c_uint32] * 4
        L.pf_dmr_hmm_evidence.restype = C.c_int64
        L.pf_region_sums.argtypes = [C.c_void_p, C.POINTER(PfPileup), C.c_uint32, C.c_uint32, C.POINTER(PfDmrCfg),
                                     C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.POINTER(PfRegions))]
        L.pf_regions_free.argtypes = [C.POINTER(PfRegions)]
        L.pf_dmr_acc_new.argtypes = [C.POINTER(PfDmrCfg), C.c_void_p, C.c_uint32]
        L.pf_dmr_acc_new.restype = C.c_void_p
        L.pf_dmr_acc_add.argtypes = [C.c_void_p, C.POINTER(PfDmr)]
        L.pf_dmr_acc_flush.argtypes = [C.c_void_p, C.POINTER(C.POINTER(PfDmr))]
        L.pf_dmr_acc_free.argtypes = [C.c_void_p]
        L.pf_write_dmr.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PfDmr), C.c_double, C.c_int]
        L.pf_batch_permtest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(C.POINTER(PfPerm))]
        L.pf_perm_free.argtypes = [C.POINTER(PfPerm)]
        L.pf_write_dmr_perm.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PfDmr), C.POINTER(PfPerm), C.c_double, C.c_int]
        L.pf_batch_ranktest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                        C.POINTER(C.POINTER(PfRank))]
        L.pf_rank_free.argtypes = [C.POINTER(PfRank)]
        L.pf_batch_rankranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.POINTER(PfRank))]
        L.pf_batch_rankexact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.POINTER(C.POINTER(PfRankExact))]
        L.pf_rank_exact_free.argtypes = [C.POINTER(PfRankExact)]
        L.pf_rank_exact_p.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
        L.pf_rank_p.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64] + [C.POINTER(C.c_double)] * 3
        L.pf_batch_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(PfAssignCfg),
                                      C.POINTER(C.POINTER(PfAssign))]
        L.pf_assign_free.argtypes = [C.POINTER(PfAssign)]
        L.pf_ilog2_q16.argtypes = [C.c_uint32]
        L.pf_ilog2_q16.restype = C.c_uint32
        L.pf_assign_site_weights.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_int32)]
        L.pf_assign_site_weights.restype = None
        L.pf_write_assign.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PfAssign), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
        L.pf_batch_tagcheck.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(PfAssignCfg),
                                        C.POINTER(C.POINTER(PfTagcheck))]
        L.pf_tagcheck_free.argtypes = [C.POINTER(PfTagcheck)]
        L.pf_tagcheck_site_weights.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]
        L.pf_tagcheck_site_weights.restype = None
        L.pf_write_tagcheck.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PfTagcheck), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]
        L.pf_write_tagcheck_regions.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PfTagcheck), C.c_void_p, C.c_void_p,
                                                C.c_int, C.POINTER(C.c_uint64)]
        if hasattr(L, "pf_haptag_reads"):
            L.pf_haptag_reads.argtypes = [C.c_void_p, C.POINTER(PfKnownVars),
                                          C.POINTER(PfReadAlnBatch), C.c_void_p]
        _lib = L
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        raise PomfretError(f"{what}: {lib().pf_strerror(rc).decode()} ({rc})")


def _pile_to_c(pile: dict):
    """A pileup dict (DeviceBatch.pileup: win_off, pos, cnt) as a pf_pileup_t
    over its arrays; returns (struct, the arrays it points into)."""
    win_off = np.ascontiguousarray(pile["win_off"], np.uint64)
    pos = np.ascontiguousarray(pile["pos"], np.uint32)
    cnt = np.ascontiguousarray(np.asarray(pile["cnt"], np.uint32).reshape(-1))
    if cnt.size != 6 * pos.size or win_off.size < 1 or int(win_off[-1]) != pos.size:
        raise PomfretError("inconsistent pileup arrays")
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    p = PfPileup(win_off.size - 1, pos.size, win_off.ctypes.data_as(u64p), pos.ctypes.data_as(u32p),
                 cnt.ctypes.data_as(u32p), 0.0)
    return p, (win_off, pos, cnt)


def _breaks(breaks):
    """(array or None, pointer or None, n) of a sorted breaks list."""
    if breaks is None or np.size(breaks) == 0:
        return None, None, 0
    b = np.ascontiguousarray(breaks, np.uint32).ravel()
    return b, b.ctypes.data, b.size


def _dmr_dict(d) -> dict:
    """A pf_dmr_t as dict(start, end, n_sites, sign, sum [n, 4], open,
    n_informative, ms, ms_upload): copies."""
    n = int(d.n_runs)
    if n:
        rec = np.ctypeslib.as_array(C.cast(d.runs, C.POINTER(C.c_uint8)), (n * DMR_RUN_DTYPE.itemsize,)).copy()
        rec = rec.view(DMR_RUN_DTYPE)
    else:
        rec = np.zeros(0, DMR_RUN_DTYPE)
    return dict(start=rec["start"].copy(), end=rec["end"].copy(), n_sites=rec["n_sites"].copy(),
                sign=rec["sign"].copy(), sum=rec["sum"].copy().reshape(n, 4), open=rec["open"].copy(),
                n_informative=int(d.n_informative), ms=float(d.ms_kernels), ms_upload=float(d.ms_upload))


def _dmr_to_c(part: dict):
    """The inverse of _dmr_dict; returns (struct, the array it points into)."""
    n = int(np.size(part["start"]))
    rec = np.zeros(max(n, 1), DMR_RUN_DTYPE)
    for k in ("start", "end", "n_sites", "sign", "open"):
        rec[k][:n] = np.asarray(part[k]).ravel()
    rec["sum"][:n] = np.asarray(part["sum"], np.uint64).reshape(n, 4)
    from .abi import PfDmrRun
    d = PfDmr(n, C.cast(rec.ctypes.data, C.POINTER(PfDmrRun)), int(part.get("n_informative", 0)), 0.0, 0.0)
    return d, rec


class _PfGaps(C.Structure):
    _fields_ = [("n_contigs", C.c_uint32), ("names", C.POINTER(C.c_char_p)),
                ("abs_start", C.POINTER(C.c_uint32)), ("abs_end", C.POINTER(C.c_uint32)),
                ("raw_off", C.POINTER(C.c_uint64)), ("gap_off", C.POINTER(C.c_uint64)),
                ("drop_off", C.POINTER(C.c_uint64)),
                ("raw_start", C.POINTER(C.c_uint32)), ("raw_end", C.POINTER(C.c_uint32)),
                ("gap_start", C.POINTER(C.c_uint32)), ("gap_end", C.POINTER(C.c_uint32)),
                ("drop_start", C.POINTER(C.c_uint32)), ("drop_end", C.POINTER(C.c_uint32))]


def _gaps_lib():
    L = lib()
    if not getattr(L, "_pf_gaps_typed", False):
        L.pf_vcf_gaps.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.POINTER(_PfGaps))]
        L.pf_interval_gaps.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.POINTER(_PfGaps))]
        L.pf_gaps_free.argtypes = [C.POINTER(_PfGaps)]
        L.pf_phase_blocks.argtypes = [C.POINTER(_PfGaps), C.c_void_p, C.POINTER(C.POINTER(_PfBlocks))]
        L.pf_blocks_free.argtypes = [C.POINTER(_PfBlocks)]
        L.pf_write_gtf.argtypes = [C.POINTER(_PfGaps), C.POINTER(_PfBlocks), C.c_char_p]
        L.pf_write_tsv.argtypes = [C.POINTER(_PfGaps), C.POINTER(_PfBlocks), C.c_char_p]
        L.pf_write_vcf.argtypes = [C.c_char_p, C.POINTER(_PfGaps), C.POINTER(_PfBlocks), C.c_void_p,
                                   C.c_char_p, C.POINTER(C.c_int64)]
        L._pf_gaps_typed = True
    return L


class _PfBlocks(C.Structure):
    _fields_ = [("n_contigs", C.c_uint32),
                ("raw_off", C.POINTER(C.c_uint64)), ("dec_off", C.POINTER(C.c_uint64)),
                ("blk_off", C.POINTER(C.c_uint64)),
                ("raw_start", C.POINTER(C.c_uint32)), ("raw_end", C.POINTER(C.c_uint32)),
                ("dec_onraw", C.POINTER(C.c_int32)), ("flip", C.POINTER(C.c_int32)),
                ("blk_start", C.POINTER(C.c_uint32)), ("blk_end", C.POINTER(C.c_uint32))]


def _gaps_contigs(p):
    """pf_gaps_t* -> [dict(name, abs_start, abs_end, raw, gaps, dropped)]."""
    g = p.contents
    res = []
    for c in range(g.n_contigs):
        def sl(off, a, b):
            return [(int(a[k]), int(b[k])) for k in range(off[c], off[c + 1])]
        res.append(dict(name=g.names[c].decode(), abs_start=int(g.abs_start[c]), abs_end=int(g.abs_end[c]),
                        raw=sl(g.raw_off, g.raw_start, g.raw_end), gaps=sl(g.gap_off, g.gap_start, g.gap_end),
                        dropped=sl(g.drop_off, g.drop_start, g.drop_end)))
    return res


def _blocks_contigs(p):
    """pf_blocks_t* -> [dict(raw, decisions, flips, blocks)] per contig."""
    b = p.contents
    res = []
    for c in range(b.n_contigs):
        res.append(dict(
            raw=[(int(b.raw_start[k]), int(b.raw_end[k])) for k in range(b.raw_off[c], b.raw_off[c + 1])],
            decisions=[int(b.dec_onraw[k]) for k in range(b.dec_off[c], b.dec_off[c + 1])],
            flips=[int(b.flip[k]) for k in range(b.dec_off[c], b.dec_off[c + 1])],
            blocks=[(int(b.blk_start[k]), int(b.blk_end[k])) for k in range(b.blk_off[c], b.blk_off[c + 1])]))
    return res


class _PfRescue(C.Structure):
    _fields_ = [("off", C.c_void_p), ("pos", C.c_void_p), ("hap_of_ref", C.c_void_p)]


INTERVALS_VCF, INTERVALS_GTF, INTERVALS_TSV = 0, 1, 2


class Gaps:
    """Phase-block gaps of a phased VCF (pf_vcf_gaps), or of a GTF / 3-column
    TSV of phase blocks (pf_interval_gaps, fmt INTERVALS_GTF / _TSV), owned C
    object."""

    def __init__(self, path: str, readback: int = 50_000, fmt: int = INTERVALS_VCF):
        L = _gaps_lib()
        self._p = C.POINTER(_PfGaps)()
        _check(L.pf_interval_gaps(path.encode(), int(fmt), readback, C.byref(self._p)), "pf_interval_gaps")

    def contigs(self):
        return _gaps_contigs(self._p)

    @property
    def n_windows(self) -> int:
        g = self._p.contents
        return int(g.gap_off[g.n_contigs])

    def close(self):
        if self._p:
            _gaps_lib().pf_gaps_free(self._p)
            self._p = C.POINTER(_PfGaps)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Blocks:
    """New phase blocks from the join decisions (pf_phase_blocks)."""

    def __init__(self, gaps: Gaps, decision):
        L = _gaps_lib()
        self.gaps = gaps
        self._dec = np.ascontiguousarray(np.asarray(decision, np.int8))
        if self._dec.size != gaps.n_windows:
            raise PomfretError(f"pf_phase_blocks: {self._dec.size} decisions for {gaps.n_windows} windows")
        self._p = C.POINTER(_PfBlocks)()
        _check(L.pf_phase_blocks(gaps._p, self._dec.ctypes.data, C.byref(self._p)), "pf_phase_blocks")

    def contigs(self):
        return _blocks_contigs(self._p)

    def write_gtf(self, path: str):
        _check(_gaps_lib().pf_write_gtf(self.gaps._p, self._p, path.encode()), "pf_write_gtf")

    def write_tsv(self, path: str):
        _check(_gaps_lib().pf_write_tsv(self.gaps._p, self._p, path.encode()), "pf_write_tsv")

    def write_vcf(self, vcf_in: str, vcf_out: str, rescue=None):
        """rescue: optional per-contig list of {pos0: hap_of_ref} dicts."""
        L = _gaps_lib()
        rp = None
        keep = []
        if rescue is not None:
            off = np.zeros(len(rescue) + 1, np.uint64)
            pos, hap = [], []
            for c, m in enumerate(rescue):
                for k in sorted(m):
                    pos.append(k)
                    hap.append(m[k])
                off[c + 1] = len(pos)
            pa = np.asarray(pos, np.uint32) if pos else np.zeros(1, np.uint32)
            ha = np.asarray(hap, np.uint8) if hap else np.zeros(1, np.uint8)
            keep = [off, pa, ha]
            rp = C.byref(_PfRescue(off.ctypes.data, pa.ctypes.data, ha.ctypes.data))
        counts = (C.c_int64 * 3)()
        _check(L.pf_write_vcf(vcf_in.encode(), self.gaps._p, self._p, rp, vcf_out.encode(), counts), "pf_write_vcf")
        del keep
        return tuple(int(x) for x in counts)

    def close(self):
        if self._p:
            _gaps_lib().pf_blocks_free(self._p)
            self._p = C.POINTER(_PfBlocks)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vcf_gaps(path: str, readback: int = 50_000):
    """Phase-block gaps of a phased VCF per contig (pf_vcf_gaps): a list of
    dict(name, abs_start, abs_end, raw, gaps, dropped) with (start, end) pairs."""
    return interval_gaps(path, INTERVALS_VCF, readback)


def interval_gaps(path: str, fmt: int = INTERVALS_VCF, readback: int = 50_000):
    """The gaps of any phase-block file `methphase` takes (pf_interval_gaps):
    --vcf, --gtf or --tsv (blockjoin.c:1977-2176, 1305-1345)."""
    g = Gaps(path, readback, fmt)
    res = g.contigs()
    g.close()
    return res


def report_windows(abs_start: int, gaps, chunk_size: int, chunk_stride: int):
    """`pomfret report` chunk windows of one contig (pf_report_windows) from
    its raw gaps [(start, end), ...]."""
    L = lib()
    L.pf_report_windows.restype = C.c_int64
    L.pf_report_windows.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_uint64]
    gs = np.array([g[0] for g in gaps], np.uint32)
    ge = np.array([g[1] for g in gaps], np.uint32)
    n = L.pf_report_windows(abs_start, gs.ctypes.data, ge.ctypes.data, len(gaps), chunk_size, chunk_stride,
                            None, None, 0)
    _check(0 if n >= 0 else int(n), "pf_report_windows")
    ws = np.zeros(max(n, 1), np.uint32)
    we = np.zeros(max(n, 1), np.uint32)
    L.pf_report_windows(abs_start, gs.ctypes.data, ge.ctypes.data, len(gaps), chunk_size, chunk_stride,
                        ws.ctypes.data, we.ctypes.data, n)
    return list(zip(ws[:n].tolist(), we[:n].tolist()))


def device_count() -> int:
    return int(lib().pf_device_count())


def fisher_exact(n11, n12, n21, n22):
    l, r, t = C.c_double(), C.c_double(), C.c_double()
    q = lib().pf_fisher_exact(n11, n12, n21, n22, C.byref(l), C.byref(r), C.byref(t))
    return q, l.value, r.value, t.value


def rank_p(u2, n1, n2, ties):
    """(auc, z, p) of the rank-sum test from DeviceBatch.ranktest's integers
    (pf_rank_p, host only): the two-sided normal approximation with tie and
    continuity correction -- scipy.stats.mannwhitneyu(alternative="two-sided",
    method="asymptotic", use_continuity=True).  Asymptotic: approximate below
    about eight reads per haplotype; p underflows to 0 near z > 38."""
    for v, top in ((u2, 2 ** 64), (n1, 2 ** 32), (n2, 2 ** 32), (ties, 2 ** 64)):
        if not 0 <= int(v) < top:
            raise PomfretError("pf_rank_p: an argument is out of range")
    a, z, p = C.c_double(), C.c_double(), C.c_double()
    _check(lib().pf_rank_p(int(u2), int(n1), int(n2), int(ties), C.byref(a), C.byref(z), C.byref(p)), "pf_rank_p")
    return a.value, z.value, p.value


def rank_exact_p(count, total):
    """count / total as a double (pf_rank_exact_p, host only): an exact p-value
    of the rank-sum test from DeviceBatch.rankexact's integers -- two for the
    two-sided one, le and ge for the one-sided ones."""
    for v in (count, total):
        if not 0 <= int(v) < 2 ** 64:
            raise PomfretError("pf_rank_exact_p: an argument is out of range")
    p = C.c_double()
    _check(lib().pf_rank_exact_p(int(count), int(total), C.byref(p)), "pf_rank_exact_p")
    return p.value


class Context:
    """One device + one HIP stream (one process per GPU)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(lib().pf_ctx_create(int(device), C.byref(h)), "pf_ctx_create")
        self.handle = h
        self.device = device
        self._batches = weakref.WeakSet()

    def close(self):
        for b in list(self._batches):      # a batch must not outlive its context
            b.free()
        if self.handle:
            lib().pf_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, cfg: Config, batch: WindowBatch) -> "DeviceBatch":
        return DeviceBatch(self, cfg, batch)

    def upload_aln(self, cfg: Config, aln: AlnBatch, lcfg: LoadConfig = None) -> "DeviceBatch":
        """Record-level batch (pf_batch_upload_aln): K0 loads the reads on
        the device in every run."""
        return DeviceBatch(self, cfg, aln, lcfg=lcfg or LoadConfig())

    def bgzf_inflate(self, comp: bytes, out_cap: int = None):
        """Inflate every BGZF block of `comp` on the device (pf_bgzf_inflate).
        Returns (output bytes, per-block status array, inflate kernel ms);
        raises PomfretError when any block fails."""
        comp = np.frombuffer(bytes(comp), np.uint8)
        cap = out_cap if out_cap is not None else max(1, 65536 * (comp.size // 28 + 1))
        out = np.empty(cap, np.uint8)
        n = C.c_uint64()
        st = np.zeros(comp.size // 26 + 1, np.uint32)
        ms = C.c_float()
        rc = lib().pf_bgzf_inflate(self.handle, comp.ctypes.data, comp.size, out.ctypes.data, cap, C.byref(n),
                                   st.ctypes.data, st.size, C.byref(ms))
        self.last_inflate_status = st
        _check(rc, "pf_bgzf_inflate")
        return out[:n.value].tobytes(), st, ms.value

    def kernel_times(self):
        cap = 16
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = C.c_int(cap)
        _check(lib().pf_last_kernel_times(self.handle, names, ms, C.byref(n)), "kernel_times")
        return {names[i].decode(): float(ms[i]) for i in range(min(n.value, cap))}

    def selftest(self) -> int:
        """Mismatching (a, b) pairs of the kernels' 16-bit count division
        against correctly rounded fp32 division (pf_selftest); 0 expected."""
        n = C.c_uint64(0)
        _check(lib().pf_selftest(self.handle, C.byref(n)), "pf_selftest")
        return int(n.value)

    def dmr_regions(self, pile: dict, cfg: DmrConfig = None, breaks=None, w0: int = 0, w1: int = None,
                    block: int = 0) -> dict:
        """The allele-specific runs of the sites of windows [w0, w1) of a
        pileup dict (pf_dmr_regions; include/pomfret_amd.h has the rules):
        dict(start, end, n_sites, sign, sum [n, 4] = pooled m1, u1, m2, u2,
        open (bit 0 / 1: the run touches the range's first / last informative
        site), n_informative, ms the region kernels' time, ms_upload).  Runs
        below cfg.min_sites are returned only when open (pipeline.dmr_stitch).
        breaks: sorted positions no run crosses.  block: sites per workgroup
        (tests; 0: PF_DMR_BLOCK of the environment or the default)."""
        p, keep = _pile_to_c(pile)
        c = (cfg or DmrConfig()).to_c()
        b, bp, nb = _breaks(breaks)
        d = C.POINTER(PfDmr)()
        _check(lib().pf_dmr_regions_block(self.handle, C.byref(p), int(w0), p.n_windows if w1 is None else int(w1),
                                          C.byref(c), bp, nb, int(block), C.byref(d)), "pf_dmr_regions")
        try:
            return _dmr_dict(d.contents)
        finally:
            lib().pf_dmr_free(d)

    def dmr_hmm_regions(self, pile: dict, cfg: DmrConfig = None, hcfg: HmmConfig = None, breaks=None, w0: int = 0,
                        w1: int = None, block: int = 0, sites: bool = False) -> dict:
        """The allele-specific regions of the sites of windows [w0, w1) of a
        pileup dict by the hidden Markov model (pf_dmr_hmm_regions;
        include/pomfret_amd.h has the model): the dict of dmr_regions -- the
        kept runs only, open all 0 -- plus n_chains; with sites=True also
        state ([n_sites] uint8: 0 none, 1 h1>h2, 2 h1<h2, 255 a transparent
        site) and evidence ([n_sites] int64, Q16 bits).  The range is taken as
        a whole: there is no stitching."""
        p, keep = _pile_to_c(pile)
        c = (cfg or DmrConfig()).to_c()
        hc = (hcfg or HmmConfig()).to_c()
        b, bp, nb = _breaks(breaks)
        h = C.POINTER(PfDmrHmm)()
        _check(lib().pf_dmr_hmm_regions(self.handle, C.byref(p), int(w0), p.n_windows if w1 is None else int(w1),
                                        C.byref(c), C.byref(hc), bp, nb, int(block), DMR_HMM_SITES if sites else 0,
                                        C.byref(h)), "pf_dmr_hmm_regions")
        try:
            x = h.contents
            res = _dmr_dict(x)
            res["n_chains"] = int(x.n_chains)
            if sites:
                n = int(x.n_sites)
                res["state"] = np.ctypeslib.as_array(x.state, (n,)).copy() if n else np.zeros(0, np.uint8)
                res["evidence"] = np.ctypeslib.as_array(x.evidence, (n,)).copy() if n else np.zeros(0, np.int64)
            return res
        finally:
            lib().pf_dmr_hmm_free(h)

    def region_sums(self, pile: dict, cfg: DmrConfig = None, starts=(), ends=(), w0: int = 0, w1: int = None,
                    block: int = 0) -> dict:
        """The sums of the caller's regions [starts[i], ends[i]) over the sites
        of windows [w0, w1) of a pileup dict (pf_region_sums;
        include/pomfret_amd.h has the rules): dict(n_cpg, n_sites, n_pos,
        n_neg, sum [n, 4] = the informative sites' m1, u1, m2, u2, evidence
        (int64, Q16 bits), each in the caller's region order, n_informative,
        ms the kernels' time, ms_upload).  Regions may come in any order and
        overlap, nest and repeat.  Of cfg only min_cov and min_delta_pct are
        used.  block: sites per workgroup (tests; 0: PF_REG_BLOCK of the
        environment or the default)."""
        p, keep = _pile_to_c(pile)
        c = (cfg or DmrConfig()).to_c()
        s = np.ascontiguousarray(starts, np.uint32).ravel()
        e = np.ascontiguousarray(ends, np.uint32).ravel()
        if s.size != e.size:
            raise PomfretError("region_sums: starts and ends differ in length")
        r = C.POINTER(PfRegions)()
        _check(lib().pf_region_sums(self.handle, C.byref(p), int(w0), p.n_windows if w1 is None else int(w1), C.byref(c),
                                    s.ctypes.data if s.size else None, e.ctypes.data if e.size else None, s.size, int(block),
                                    C.byref(r)), "pf_region_sums")
        try:
            x = r.contents
            n = int(x.n)
            if n:
                rec = np.ctypeslib.as_array(C.cast(x.r, C.POINTER(C.c_uint8)), (n * REGION_SUM_DTYPE.itemsize,)).copy()
                rec = rec.view(REGION_SUM_DTYPE)
            else:
                rec = np.zeros(0, REGION_SUM_DTYPE)
            return dict(n_cpg=rec["n_cpg"].copy(), n_sites=rec["n_sites"].copy(), n_pos=rec["n_pos"].copy(),
                        n_neg=rec["n_neg"].copy(), sum=rec["sum"].copy().reshape(n, 4), evidence=rec["evidence"].copy(),
                        n_informative=int(x.n_informative), ms=float(x.ms_kernels), ms_upload=float(x.ms_upload))
        finally:
            lib().pf_regions_free(r)

    def haptag_reads(self, known: KnownVars, reads: ReadAlnBatch) -> np.ndarray:
        out = np.zeros(max(reads.n_reads, 1), np.uint8)
        k, r = known.to_c(), reads.to_c()
        _check(lib().pf_haptag_reads(self.handle, C.byref(k), C.byref(r), out.ctypes.data),
               "pf_haptag_reads")
        return out[:reads.n_reads]


class DeviceBatch:
    """A window batch resident in HBM (pf_dbatch_t)."""

    def __init__(self, ctx: Context, cfg: Config, batch, lcfg: LoadConfig = None):
        self.ctx = ctx
        self.n_windows = batch.n_windows
        c, b = cfg.to_c(), batch.to_c()
        h = C.c_void_p()
        if isinstance(batch, AlnBatch):
            lc = lcfg.to_c()
            _check(lib().pf_batch_upload_aln(ctx.handle, C.byref(c), C.byref(lc), C.byref(b), C.byref(h)),
                   "pf_batch_upload_aln")
        else:
            _check(lib().pf_batch_upload(ctx.handle, C.byref(c), C.byref(b), C.byref(h)),
                   "pf_batch_upload")
        self.handle = h
        self.record_level = isinstance(batch, AlnBatch)
        ctx._batches.add(self)

    @classmethod
    def _wrap(cls, ctx: Context, handle, n_windows: int) -> "DeviceBatch":
        """A record-level batch built by the library (e.g. the device fetch)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.n_windows = n_windows
        self.handle = handle
        self.record_level = True
        ctx._batches.add(self)
        return self

    def debug_recs(self) -> dict:
        """The record arrays of a record-level batch (pf_batch_debug_recs)."""
        sz = np.zeros(5, np.uint64)
        _check(lib().pf_batch_debug_recs(self.handle, sz.ctypes.data, *([None] * 14)), "pf_batch_debug_recs")
        n, nc, ns, nm, nl = (int(x) for x in sz)
        d = dict(flag=np.zeros(n, np.uint16), mapq=np.zeros(n, np.uint8), pos=np.zeros(n, np.uint32),
                 l_qseq=np.zeros(n, np.uint32), de=np.zeros(n, np.float32), hp=np.zeros(n, np.uint8),
                 cigar_off=np.zeros(n + 1, np.uint64), cigar=np.zeros(max(nc, 1), np.uint32),
                 seq_off=np.zeros(n + 1, np.uint64), seq=np.zeros(max(ns, 1), np.uint8),
                 mm_off=np.zeros(n + 1, np.uint64), mm=np.zeros(max(nm, 1), np.uint8),
                 ml_off=np.zeros(n + 1, np.uint64), ml=np.zeros(max(nl, 1), np.uint8))
        keys = ["flag", "mapq", "pos", "l_qseq", "de", "hp", "cigar_off", "cigar", "seq_off", "seq", "mm_off", "mm",
                "ml_off", "ml"]
        _check(lib().pf_batch_debug_recs(self.handle, sz.ctypes.data, *[d[k].ctypes.data for k in keys]),
               "pf_batch_debug_recs")
        d["cigar"], d["seq"], d["mm"], d["ml"] = d["cigar"][:nc], d["seq"][:ns], d["mm"][:nm], d["ml"][:nl]
        return d

    @property
    def n_reads(self) -> int:
        """Reads of the batch.  Record level: the kept records of the last
        finished run (K0 sizes the batch on the device in every run); before
        any run, the record count (an upper bound)."""
        return int(lib().pf_batch_n_reads(self.handle))

    def read_recs(self) -> np.ndarray:
        """Record index of every read of the batch (identity for window
        batches).  Record level: runs the loader first if no run has finished."""
        R = self.n_reads
        out = np.zeros(max(R, 1), np.uint32)
        rc = lib().pf_batch_read_recs(self.handle, out.ctypes.data, out.size)
        if rc != 0 and self.record_level:           # no run has finished yet: load once
            self.debug_calls(cap=0, probe=True)
            R = self.n_reads
            rc = lib().pf_batch_read_recs(self.handle, out.ctypes.data, out.size)
        _check(rc, "pf_batch_read_recs")
        return out[:R]

    def debug_calls(self, cap: int = None, probe: bool = False):
        """K0 output: (call_off, pos, cat, first, last), calls sorted by (pos, cat) per read.
        probe=True only runs the loader (sizes the batch)."""
        if cap is None:
            if self.record_level and not lib().pf_batch_n_calls(self.handle):
                self.debug_calls(cap=0, probe=True)
            cap = int(lib().pf_batch_n_calls(self.handle))
        R = self.n_reads
        off = np.zeros(R + 1, np.uint64)
        pos = np.zeros(max(cap, 1), np.uint32)
        cat = np.zeros(max(cap, 1), np.uint8)
        first = np.zeros(max(R, 1), np.uint32)
        last = np.zeros(max(R, 1), np.uint32)
        n = lib().pf_batch_debug_calls(self.handle, off.ctypes.data, pos.ctypes.data, cat.ctypes.data,
                                       first.ctypes.data, last.ctypes.data, cap)
        if probe:
            return None
        if n < 0:
            _check(int(n), "pf_batch_debug_calls")
        R = self.n_reads
        return off[:R + 1], pos[:n], cat[:n], first[:R], last[:R]

    def debug_spans(self):
        """K0 output: (read_start, read_end) of every read, after a run of the loader."""
        n = max(self.n_reads, 1)
        start, end = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _check(lib().pf_batch_debug_spans(self.handle, start.ctypes.data, end.ctypes.data, n), "pf_batch_debug_spans")
        R = self.n_reads
        return start[:R], end[:R]

    def load_counters(self) -> dict:
        out = np.zeros(8, np.uint64)
        _check(lib().pf_batch_load_counters(self.handle, out.ctypes.data, 8), "pf_batch_load_counters")
        return dict(seq_path=int(out[0]), unsorted=int(out[1]), implicit=int(out[2]), bad_mm=int(out[3]),
                    dup_chunks=int(out[4]), multi_cm=int(out[5]))

    def free(self):
        if self.handle:
            lib().pf_batch_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def run(self, out: WindowResult = None) -> WindowResult:
        fresh = out is None
        if fresh:
            out = WindowResult.alloc(self.n_windows, self.n_reads)
        o = out.to_c()
        _check(lib().pf_methphase_run(self.ctx.handle, self.handle, C.byref(o)), "pf_methphase_run")
        if fresh:
            out.read_hp = out.read_hp[:self.n_reads]
        return out

    def pileup(self, read_hp=None) -> dict:
        """Per-haplotype CpG methylation pileup of the batch's calls
        (pf_batch_pileup): dict(win_off [W+1], pos [n] ascending inside a
        window, cnt [n, 3, 2] indexed [site, h, cat] with h 0 / 1 / 2 = other
        and cat 0 meth / 1 unmeth, ms the pileup kernels' time).  read_hp:
        tags in read order that replace the batch's own for this call (e.g.
        a run's WindowResult.read_hp); a record-level batch runs its loader
        first."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            # one spare byte keeps the pointer valid (and non-NULL) for zero reads
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        p = C.POINTER(PfPileup)()
        _check(lib().pf_batch_pileup(self.ctx.handle, self.handle, hp_ptr, n_hp, C.byref(p)), "pf_batch_pileup")
        try:
            r = p.contents
            W, n = int(r.n_windows), int(r.n_sites)
            win_off = np.ctypeslib.as_array(r.win_off, (W + 1,)).copy()
            pos = np.ctypeslib.as_array(r.pos, (n,)).copy() if n else np.zeros(0, np.uint32)
            cnt = np.ctypeslib.as_array(r.cnt, (n * 6,)).copy() if n else np.zeros(0, np.uint32)
            return dict(win_off=win_off, pos=pos, cnt=cnt.reshape(n, 3, 2), ms=float(r.ms_kernels))
        finally:
            lib().pf_pileup_free(p)

    def permtest(self, n_perm: int, seed: int = 1, read_hp=None) -> dict:
        """Read-label permutation test of every window of the batch
        (pf_batch_permtest; include/pomfret_amd.h has the definition):
        dict(n_reads [W, 2] the participating reads tagged 0 / 1, sum [W, 4]
        their m1, u1, m2, u2 inside the window, hits [W] the permutations at
        least as extreme as the true labels, status [W] (0 tested, 1 nothing
        to test, 2 more than 4,096 participating reads), n_perm, seed, ms the
        kernel's time).  p = (hits + 1) / (n_perm + 1) where status is 0.
        read_hp as in pileup."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        if not 0 <= int(n_perm) <= 0xFFFFFFFF or not 0 <= int(seed) <= 0xFFFFFFFF:
            raise PomfretError("pf_batch_permtest: n_perm and seed are 32-bit unsigned")
        p = C.POINTER(PfPerm)()
        _check(lib().pf_batch_permtest(self.ctx.handle, self.handle, hp_ptr, n_hp, int(n_perm), int(seed), C.byref(p)),
               "pf_batch_permtest")
        try:
            r = p.contents
            W = int(r.n_windows)

            def arr(ptr, n, dt):
                return np.ctypeslib.as_array(ptr, (n,)).copy() if W else np.zeros(0, dt)
            return dict(n_reads=arr(r.n_reads, 2 * W, np.uint32).reshape(W, 2), sum=arr(r.sum, 4 * W, np.uint64).reshape(W, 4),
                        hits=arr(r.hits, W, np.uint32), status=arr(r.status, W, np.uint32), n_perm=int(r.n_perm),
                        seed=int(r.seed), ms=float(r.ms_kernels))
        finally:
            lib().pf_perm_free(p)

    def ranktest(self, min_calls: int = 3, read_hp=None) -> dict:
        """Read-level rank-sum (Mann-Whitney) test of every window of the
        batch (pf_batch_ranktest; include/pomfret_amd.h has the definition):
        dict(n_reads [W, 2] the counted reads tagged 0 / 1 (tag 0 or 1, at
        least min_calls call entries inside the window), n_short [W, 2] the
        reads below min_calls, cls [W, 2, 3] the all-meth, all-unmeth and mixed
        reads per tag, sum [W, 4] the counted reads' m1, u1, m2, u2, u2 [W]
        twice haplotype 1's U, ties [W] the tie term, status [W] (0 tested, 1
        a haplotype without a counted read, 2 more than 4,096 counted reads),
        min_calls, ms the kernel's time).  rank_p(u2, n1, n2, ties) gives auc,
        z and p where status is 0.  read_hp as in pileup."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        if not 0 <= int(min_calls) <= 0xFFFFFFFF:
            raise PomfretError("pf_batch_ranktest: min_calls is 32-bit unsigned")
        p = C.POINTER(PfRank)()
        _check(lib().pf_batch_ranktest(self.ctx.handle, self.handle, hp_ptr, n_hp, int(min_calls), C.byref(p)),
               "pf_batch_ranktest")
        try:
            r = p.contents
            W = int(r.n_windows)

            def arr(ptr, n, dt):
                return np.ctypeslib.as_array(ptr, (n,)).copy() if W else np.zeros(0, dt)
            return dict(n_reads=arr(r.n_reads, 2 * W, np.uint32).reshape(W, 2),
                        n_short=arr(r.n_short, 2 * W, np.uint32).reshape(W, 2),
                        cls=arr(r.cls, 6 * W, np.uint32).reshape(W, 2, 3), sum=arr(r.sum, 4 * W, np.uint64).reshape(W, 4),
                        u2=arr(r.u2, W, np.uint64), ties=arr(r.ties, W, np.uint64), status=arr(r.status, W, np.uint32),
                        min_calls=int(r.min_calls), ms=float(r.ms_kernels))
        finally:
            lib().pf_rank_free(p)

    def rankranges(self, off, starts, ends, min_calls: int = 3, read_hp=None) -> dict:
        """ranktest over position ranges inside the windows
        (pf_batch_rankranges): range i of window w, off[w] <= i < off[w + 1],
        is tested over window w's reads as a window [starts[i], ends[i]) would
        be.  off is [W + 1], starting at 0 and non-decreasing; the ranges of a
        window may overlap, be empty or be missing.  Returns ranktest's dict
        with one entry per range, in range order."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        if not 0 <= int(min_calls) <= 0xFFFFFFFF:
            raise PomfretError("pf_batch_rankranges: min_calls is 32-bit unsigned")
        o = np.ascontiguousarray(off, np.uint64).ravel()
        s, e = np.ascontiguousarray(starts, np.uint32).ravel(), np.ascontiguousarray(ends, np.uint32).ravel()
        if o.size == 0 or s.size != e.size or int(o[-1]) != s.size:
            raise PomfretError("pf_batch_rankranges: off is [n_windows + 1] and off[-1] the number of ranges")
        s, e = np.concatenate([s, np.zeros(1, np.uint32)]), np.concatenate([e, np.zeros(1, np.uint32)])   # never empty
        p = C.POINTER(PfRank)()
        _check(lib().pf_batch_rankranges(self.ctx.handle, self.handle, hp_ptr, n_hp, int(min_calls), o.ctypes.data,
                                         s.ctypes.data, e.ctypes.data, C.byref(p)), "pf_batch_rankranges")
        try:
            r = p.contents
            W = int(r.n_windows)

            def arr(ptr, n, dt):
                return np.ctypeslib.as_array(ptr, (n,)).copy() if W else np.zeros(0, dt)
            return dict(n_reads=arr(r.n_reads, 2 * W, np.uint32).reshape(W, 2),
                        n_short=arr(r.n_short, 2 * W, np.uint32).reshape(W, 2),
                        cls=arr(r.cls, 6 * W, np.uint32).reshape(W, 2, 3), sum=arr(r.sum, 4 * W, np.uint64).reshape(W, 4),
                        u2=arr(r.u2, W, np.uint64), ties=arr(r.ties, W, np.uint64), status=arr(r.status, W, np.uint32),
                        min_calls=int(r.min_calls), ms=float(r.ms_kernels))
        finally:
            lib().pf_rank_free(p)

    def rankexact(self, min_calls: int = 3, max_reads: int = 64, read_hp=None) -> dict:
        """The rank-sum test's exact null distribution for every window of at
        most max_reads (2 .. 64) counted reads (pf_batch_rankexact;
        include/pomfret_amd.h has the definition): dict(n_reads [W, 2], n_short
        [W, 2] and u2 [W] as ranktest gives them, total [W] = C(n, n1), le, ge
        and two [W] the assignments of the counted reads whose statistic is at
        most / at least / at least as far from its centre as the observed one,
        status [W] (0 tested, 1 a haplotype without a counted read, 2 more
        than max_reads counted reads; the counts are 0 unless 0), min_calls,
        max_reads, ms the kernel's time).  rank_exact_p(two, total) is the
        two-sided p-value where status is 0.  read_hp as in pileup."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        if not 0 <= int(min_calls) <= 0xFFFFFFFF or not 0 <= int(max_reads) <= 0xFFFFFFFF:
            raise PomfretError("pf_batch_rankexact: min_calls and max_reads are 32-bit unsigned")
        p = C.POINTER(PfRankExact)()
        _check(lib().pf_batch_rankexact(self.ctx.handle, self.handle, hp_ptr, n_hp, int(min_calls), int(max_reads),
                                        C.byref(p)), "pf_batch_rankexact")
        try:
            r = p.contents
            W = int(r.n_windows)

            def arr(ptr, n, dt):
                return np.ctypeslib.as_array(ptr, (n,)).copy() if W else np.zeros(0, dt)
            return dict(n_reads=arr(r.n_reads, 2 * W, np.uint32).reshape(W, 2),
                        n_short=arr(r.n_short, 2 * W, np.uint32).reshape(W, 2), u2=arr(r.u2, W, np.uint64),
                        total=arr(r.total, W, np.uint64), le=arr(r.le, W, np.uint64), ge=arr(r.ge, W, np.uint64),
                        two=arr(r.two, W, np.uint64), status=arr(r.status, W, np.uint32), min_calls=int(r.min_calls),
                        max_reads=int(r.max_reads), ms=float(r.ms_kernels))
        finally:
            lib().pf_rank_exact_free(p)

    def assign(self, cfg: AssignConfig = None, read_hp=None) -> dict:
        """Tags for the batch's untagged reads from each window's
        allele-specific methylation (pf_batch_assign; include/pomfret_amd.h
        has the definition): dict(win_read_off [W+1], n_used [R] the read's
        call entries at informative sites (0 for a read that is no
        candidate), llr [R] the score S in Q16 bits (int64; positive:
        haplotype 1), hp [R] the new tag of a candidate and the input tag of
        every other read -- pileup's read_hp --, win_n [W, 3] the candidates
        with n_used >= 1, assigned 0, assigned 1, ms the assign kernels'
        time).  read_hp as in pileup."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        c = (cfg or AssignConfig()).to_c()
        p = C.POINTER(PfAssign)()
        _check(lib().pf_batch_assign(self.ctx.handle, self.handle, hp_ptr, n_hp, C.byref(c), C.byref(p)), "pf_batch_assign")
        try:
            r = p.contents
            W, R = int(r.n_windows), int(r.n_reads)

            def arr(ptr, n, dt):
                return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dt)
            return dict(win_read_off=arr(r.win_read_off, W + 1, np.uint32), n_used=arr(r.n_used, R, np.uint32),
                        llr=arr(r.llr, R, np.int64), hp=arr(r.hp, R, np.uint8),
                        win_n=arr(r.win_n, 3 * W, np.uint32).reshape(W, 3), ms=float(r.ms_kernels))
        finally:
            lib().pf_assign_free(p)

    def tagcheck(self, cfg: AssignConfig = None, read_hp=None) -> dict:
        """Leave-one-out check of the batch's tagged reads under cfg, the rule
        assign applies (pf_batch_tagcheck; include/pomfret_amd.h has the
        definition): dict(win_read_off [W+1], n_used [R] the read's usable
        entries, llr [R] the score S in Q16 bits (int64; positive: haplotype
        1), verdict [R] 0 ok / 1 flip / 2 undecided / 255 not scored, hp [R]
        the tags the call ran under, win_n [W, 2, 4] per tag the window's
        reads, those with n_used >= 1, ok, flip, ms the tag-check kernels'
        time).  read_hp as in pileup."""
        hp_ptr, n_hp = None, 0
        if read_hp is not None:
            hp = np.zeros(np.size(read_hp) + 1, np.uint8)
            hp[:-1] = np.asarray(read_hp, np.uint8).ravel()
            hp_ptr, n_hp = hp.ctypes.data, hp.size - 1
        c = (cfg or AssignConfig()).to_c()
        p = C.POINTER(PfTagcheck)()
        _check(lib().pf_batch_tagcheck(self.ctx.handle, self.handle, hp_ptr, n_hp, C.byref(c), C.byref(p)),
               "pf_batch_tagcheck")
        try:
            r = p.contents
            W, R = int(r.n_windows), int(r.n_reads)

            def arr(ptr, n, dt):
                return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dt)
            return dict(win_read_off=arr(r.win_read_off, W + 1, np.uint32), n_used=arr(r.n_used, R, np.uint32),
                        llr=arr(r.llr, R, np.int64), verdict=arr(r.verdict, R, np.uint8), hp=arr(r.hp, R, np.uint8),
                        win_n=arr(r.win_n, 8 * W, np.uint32).reshape(W, 2, 4), ms=float(r.ms_kernels))
        finally:
            lib().pf_tagcheck_free(p)

    def stats(self) -> np.ndarray:
        """Per-(window, dir) counters of the last run: [W, 2, 8] (see pf_batch_stats)."""
        out = np.zeros((max(self.n_windows, 1), 2, 8), np.uint64)
        _check(lib().pf_batch_stats(self.handle, out.ctypes.data, out.size), "pf_batch_stats")
        return out[:self.n_windows]

    def k12_paths(self) -> np.ndarray:
        """Per-window sites path of the last run's K12: 1 / 2 the fast path
        over one / two segments, 3 the dense path, 0 none (pf_batch_k12_paths)."""
        out = np.zeros(max(self.n_windows, 1), np.uint8)
        _check(lib().pf_batch_k12_paths(self.handle, out.ctypes.data, out.size), "pf_batch_k12_paths")
        return out[:self.n_windows]

    def k12_chunk_items(self) -> int:
        """The read chunks the last run's K12 handed to pf_k12_chunks
        (pf_batch_k12_chunk_items); 0: every methmer phase ran in K12."""
        f = lib().pf_batch_k12_chunk_items
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        n = C.c_uint32(0)
        _check(f(self.handle, C.byref(n)), "pf_batch_k12_chunk_items")
        return int(n.value)

    def set_mask(self, pos, win_rng=None):
        """Masked reference positions (pf_batch_set_mask): a position that
        qualifies as a methylation site and is in `pos` (strictly ascending,
        0-based, below 2^29) is no site.  win_rng: [n_windows, 2] index ranges
        into `pos`, window w seeing pos[win_rng[w, 0]:win_rng[w, 1]]; None:
        every window sees all of it.  An empty `pos` clears the mask.  The
        mask stays in force for later runs until replaced."""
        pos = np.ascontiguousarray(np.asarray(pos, np.int64).ravel())
        if pos.size and (pos.min() < 0 or pos.max() > 0xFFFFFFFF):
            raise PomfretError("pf_batch_set_mask: positions must fit 32 bits")
        p32 = np.ascontiguousarray(pos.astype(np.uint32))
        rng = None
        if win_rng is not None:
            rng = np.ascontiguousarray(np.asarray(win_rng, np.uint32).reshape(-1))
            if rng.size != 2 * self.n_windows:
                raise PomfretError(f"pf_batch_set_mask: win_rng needs {self.n_windows} (begin, end) pairs")
        _check(lib().pf_batch_set_mask(self.handle, p32.ctypes.data if p32.size else None, p32.size,
                                       rng.ctypes.data if rng is not None and rng.size else None),
               "pf_batch_set_mask")

    def masked_sites(self) -> np.ndarray:
        """Per window, the qualifying positions the mask removed in the last
        finished run (pf_batch_masked_sites); zeros with no mask."""
        out = np.zeros(max(self.n_windows, 1), np.uint32)
        _check(lib().pf_batch_masked_sites(self.handle, out.ctypes.data, out.size), "pf_batch_masked_sites")
        return out[:self.n_windows]

    def k3_paths(self) -> np.ndarray:
        """Per-(window, dir) slot-list source of the last run's greedy loop:
        [W, 2] of 1 LDS lists, 2 candidate cache, 3 HBM lists, 4 general
        body, 5 one-wave kernel, 6 candidate cache with the count table in
        HBM, 0 no sites (pf_batch_k3_paths)."""
        out = np.zeros(max(2 * self.n_windows, 2), np.uint8)
        _check(lib().pf_batch_k3_paths(self.handle, out.ctypes.data, out.size), "pf_batch_k3_paths")
        return out[:2 * self.n_windows].reshape(-1, 2)

    def k3_budget(self) -> dict:
        """The greedy launch of this batch (pf_batch_k3_budget): the main
        kernel's dynamic LDS per problem and its resident workgroups, the
        heavy kernel's LDS and problem count."""
        out = np.zeros(4, np.uint32)
        _check(lib().pf_batch_k3_budget(self.handle, out.ctypes.data, out.size), "pf_batch_k3_budget")
        return {"lds": int(out[0]), "resident": int(out[1]), "lds_heavy": int(out[2]), "n_heavy": int(out[3])}

    def heavy_problems(self) -> np.ndarray:
        """Greedy problems (w<<1 | dir) run in pf_k3_heavy: the windows with at
        least 2,000 reads (1,100 when the batch's 90th-percentile window has
        <= 400), see pf_batch_heavy."""
        n = lib().pf_batch_heavy(self.handle, None, 0)
        out = np.zeros(max(n, 1), np.uint32)
        if n:
            lib().pf_batch_heavy(self.handle, out.ctypes.data, n)
        return out[:n]

    def debug_sites(self, w: int, direction: int, cap: int = 1 << 22):
        real = np.zeros(cap, np.uint32)
        starts = np.zeros(cap, np.uint32)
        lens = np.zeros(cap, np.uint8)
        n = lib().pf_batch_debug_sites(self.handle, w, direction, real.ctypes.data,
                                       starts.ctypes.data, lens.ctypes.data, cap)
        if n < 0:
            _check(n, "pf_batch_debug_sites")
        return real[:n], starts[:n], lens[:n]

    def debug_methmers(self, direction: int, cap: int = 1 << 26):
        n = np.zeros(max(self.n_reads, 1), np.uint32)
        st = np.zeros(max(self.n_reads, 1), np.uint32)
        keys = np.zeros(cap, np.uint32)
        tot = lib().pf_batch_debug_methmers(self.handle, direction, n.ctypes.data, st.ctypes.data,
                                            keys.ctypes.data, cap)
        if tot < 0:
            _check(int(tot), "pf_batch_debug_methmers")
        return n[:self.n_reads], st[:self.n_reads], keys[:tot]

    def launch(self):
        _check(lib().pf_methphase_launch(self.ctx.handle, self.handle), "pf_methphase_launch")

    def finish(self, out: WindowResult = None) -> WindowResult:
        fresh = out is None
        if fresh:
            out = WindowResult.alloc(self.n_windows, self.n_reads)
        o = out.to_c()
        _check(lib().pf_methphase_finish(self.ctx.handle, self.handle, C.byref(o)),
               "pf_methphase_finish")
        if fresh:
            out.read_hp = out.read_hp[:self.n_reads]
        return out


def methphase_windows(cfg: Config, batch: WindowBatch, device: int = 0, mask=None) -> WindowResult:
    """One-shot: upload + run + free (pf_methphase_windows).  mask: masked
    reference positions for every window (DeviceBatch.set_mask)."""
    if mask is not None:
        ctx = Context(device)
        try:
            db = ctx.upload(cfg, batch)
            db.set_mask(mask)
            return db.run()
        finally:
            ctx.close()
    out = WindowResult.alloc(batch.n_windows, batch.n_reads)
    c, b, o = cfg.to_c(), batch.to_c(), out.to_c()
    _check(lib().pf_methphase_windows(int(device), C.byref(c), C.byref(b), C.byref(o)),
           "pf_methphase_windows")
    return out
