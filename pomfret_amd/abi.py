"""ctypes mirror of include/pomfret_amd.h plus numpy-side batch containers.

This module only describes the C ABI; it never computes anything.  The
product entry points live in pomfret_amd/_lib.py (libpomfret_amd.so); the CPU
oracle (tests / bench baseline only) reuses these struct definitions.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

PF_OK = 0
PF_ERR_ARG = -1
PF_ERR_HIP = -2
PF_ERR_NOMEM = -3
PF_ERR_UNSUPPORTED = -4
PF_ERR_LIMIT = -5
PF_ERR_INTERNAL = -6

HAPTAG_UNPHASED = 254  # reference blockjoin.c:26


class PfCfg(C.Structure):
    """pf_cfg_t  (mirrors mmr_config_t, reference blockjoin.h:7-16)."""
    _fields_ = [
        ("k", C.c_int32),
        ("k_span", C.c_int32),
        ("cov_for_selection", C.c_int32),
        ("cov_for_runtime", C.c_int32),
        ("n_cand", C.c_int32),
        ("hard_cov", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32),
    ]


class PfWindowBatch(C.Structure):
    _fields_ = [
        ("n_windows", C.c_uint32),
        ("n_reads", C.c_uint32),
        ("n_calls", C.c_uint64),
        ("win_start", C.c_void_p),
        ("win_end", C.c_void_p),
        ("win_read_off", C.c_void_p),
        ("win_cov_sel", C.c_void_p),
        ("win_cov_rt", C.c_void_p),
        ("win_n_cand", C.c_void_p),
        ("read_start", C.c_void_p),
        ("read_end", C.c_void_p),
        ("read_hp", C.c_void_p),
        ("read_call_off", C.c_void_p),
        ("call_pos", C.c_void_p),
        ("call_cat", C.c_void_p),
    ]


class PfWindowOut(C.Structure):
    _fields_ = [
        ("decision", C.c_void_p),
        ("read_hp", C.c_void_p),
        ("dir_table", C.c_void_p),
        ("dir_join", C.c_void_p),
        ("dir_which_way", C.c_void_p),
        ("dir_fisher_p", C.c_void_p),
        ("dir_score", C.c_void_p),
        ("win_n_sites", C.c_void_p),
        ("win_n_reads", C.c_void_p),
    ]


class PfKnownVars(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("pos", C.c_void_p),
        ("len", C.c_void_p),
        ("op", C.c_void_p),
        ("haptag", C.c_void_p),
        ("char_off", C.c_void_p),
        ("chars", C.c_void_p),
    ]


class PfReadAlnBatch(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint32),
        ("start", C.c_void_p),
        ("end", C.c_void_p),
        ("cigar_off", C.c_void_p),
        ("cigar", C.c_void_p),
        ("seq_off", C.c_void_p),
        ("seq_len", C.c_void_p),
        ("seq", C.c_void_p),
        ("md_off", C.c_void_p),
        ("md", C.c_void_p),
    ]


def _ptr(a: Optional[np.ndarray]) -> Optional[int]:
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays must be C-contiguous"
    return a.ctypes.data


@dataclass
class Config:
    """Hot-path parameters.  Defaults = `pomfret methphase -c 60` (cli.c:270-275,
    blockjoin.c:4656-4659): cov_for_selection 6, cov_for_runtime 12, n_cand 15."""
    k: int = 3
    k_span: int = 5000
    cov_for_selection: int = 6
    cov_for_runtime: int = 12
    n_cand: int = 15
    hard_cov: int = 15

    @staticmethod
    def from_coverage(cov: int, report: bool = False, given: bool = True) -> "Config":
        """Parameter derivation of the reference.
        methphase -c C   : C/10, 2*(C/10), C/4          (cli.c:270-275, blockjoin.c:4657)
        methphase (auto) : est/10+1, 2*(...), est/4+1   (blockjoin.c:4373-4375)
        report           : c/10+1, 2*(...), c/4+1       (blockjoin.c:5045-5051)
        followed by the clamps of blockjoin.c:4381-4390."""
        if report or not given:
            sel, nc = cov // 10 + 1, cov // 4 + 1
        else:
            sel, nc = cov // 10, cov // 4
        rt = 2 * sel
        if sel <= 0:
            sel = 1
        if nc <= 1:
            nc = 2
        return Config(cov_for_selection=sel, cov_for_runtime=rt, n_cand=nc)

    def to_c(self) -> PfCfg:
        return PfCfg(self.k, self.k_span, self.cov_for_selection, self.cov_for_runtime,
                     self.n_cand, self.hard_cov, 0, 0)


@dataclass
class WindowBatch:
    """Host SoA of a batch of windows (see pf_window_batch_t)."""
    win_start: np.ndarray      # u32 [W]
    win_end: np.ndarray        # u32 [W]
    win_read_off: np.ndarray   # u32 [W+1]
    read_start: np.ndarray     # u32 [R]
    read_end: np.ndarray       # u32 [R]
    read_hp: np.ndarray        # u8  [R]
    read_call_off: np.ndarray  # u64 [R+1]
    call_pos: np.ndarray       # u32 [N]
    call_cat: np.ndarray       # u8  [N]
    win_cov_sel: Optional[np.ndarray] = None  # i32 [W]
    win_cov_rt: Optional[np.ndarray] = None
    win_n_cand: Optional[np.ndarray] = None
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        self.win_start = np.ascontiguousarray(self.win_start, dtype=np.uint32)
        self.win_end = np.ascontiguousarray(self.win_end, dtype=np.uint32)
        self.win_read_off = np.ascontiguousarray(self.win_read_off, dtype=np.uint32)
        self.read_start = np.ascontiguousarray(self.read_start, dtype=np.uint32)
        self.read_end = np.ascontiguousarray(self.read_end, dtype=np.uint32)
        self.read_hp = np.ascontiguousarray(self.read_hp, dtype=np.uint8)
        self.read_call_off = np.ascontiguousarray(self.read_call_off, dtype=np.uint64)
        self.call_pos = np.ascontiguousarray(self.call_pos, dtype=np.uint32)
        self.call_cat = np.ascontiguousarray(self.call_cat, dtype=np.uint8)
        for name in ("win_cov_sel", "win_cov_rt", "win_n_cand"):
            v = getattr(self, name)
            if v is not None:
                setattr(self, name, np.ascontiguousarray(v, dtype=np.int32))

    @property
    def n_windows(self) -> int:
        return int(self.win_start.shape[0])

    @property
    def n_reads(self) -> int:
        return int(self.read_start.shape[0])

    @property
    def n_calls(self) -> int:
        return int(self.call_pos.shape[0])

    def to_c(self) -> PfWindowBatch:
        b = PfWindowBatch()
        b.n_windows = self.n_windows
        b.n_reads = self.n_reads
        b.n_calls = self.n_calls
        b.win_start = _ptr(self.win_start)
        b.win_end = _ptr(self.win_end)
        b.win_read_off = _ptr(self.win_read_off)
        b.win_cov_sel = _ptr(self.win_cov_sel)
        b.win_cov_rt = _ptr(self.win_cov_rt)
        b.win_n_cand = _ptr(self.win_n_cand)
        b.read_start = _ptr(self.read_start)
        b.read_end = _ptr(self.read_end)
        b.read_hp = _ptr(self.read_hp)
        b.read_call_off = _ptr(self.read_call_off)
        b.call_pos = _ptr(self.call_pos)
        b.call_cat = _ptr(self.call_cat)
        return b

    def select(self, windows) -> "WindowBatch":
        """Sub-batch with the given window indices (reads/calls re-packed)."""
        windows = np.asarray(windows, dtype=np.int64)
        ro = self.win_read_off.astype(np.int64)
        co = self.read_call_off.astype(np.int64)
        reads = [np.arange(ro[w], ro[w + 1]) for w in windows]
        reads = np.concatenate(reads) if reads else np.zeros(0, np.int64)
        rcount = np.array([ro[w + 1] - ro[w] for w in windows], dtype=np.int64)
        ccount = co[reads + 1] - co[reads]
        calls = [np.arange(co[r], co[r + 1]) for r in reads]
        calls = np.concatenate(calls) if len(calls) else np.zeros(0, np.int64)
        sub = lambda a: None if a is None else a[windows]
        return WindowBatch(
            win_start=self.win_start[windows], win_end=self.win_end[windows],
            win_read_off=np.concatenate([[0], np.cumsum(rcount)]),
            read_start=self.read_start[reads], read_end=self.read_end[reads],
            read_hp=self.read_hp[reads],
            read_call_off=np.concatenate([[0], np.cumsum(ccount)]),
            call_pos=self.call_pos[calls], call_cat=self.call_cat[calls],
            win_cov_sel=sub(self.win_cov_sel), win_cov_rt=sub(self.win_cov_rt),
            win_n_cand=sub(self.win_n_cand), meta=dict(self.meta))


@dataclass
class WindowResult:
    decision: np.ndarray      # i8  [W]
    read_hp: np.ndarray       # u8  [R]
    dir_table: np.ndarray     # i32 [W,2,4]
    dir_join: np.ndarray      # i32 [W,2]
    dir_which_way: np.ndarray # i32 [W,2]
    dir_fisher_p: np.ndarray  # f64 [W,2]
    dir_score: np.ndarray     # f32 [W,2]
    win_n_sites: np.ndarray   # u32 [W]
    win_n_reads: np.ndarray   # u32 [W]

    @staticmethod
    def alloc(n_windows: int, n_reads: int) -> "WindowResult":
        W, R = n_windows, n_reads
        return WindowResult(
            decision=np.full(W, -2, np.int8), read_hp=np.full(R, 255, np.uint8),
            dir_table=np.full((W, 2, 4), -1, np.int32), dir_join=np.full((W, 2), -5, np.int32),
            dir_which_way=np.full((W, 2), -5, np.int32), dir_fisher_p=np.full((W, 2), -1.0),
            dir_score=np.full((W, 2), -1.0, np.float32), win_n_sites=np.zeros(W, np.uint32),
            win_n_reads=np.zeros(W, np.uint32))

    def to_c(self) -> PfWindowOut:
        o = PfWindowOut()
        o.decision = _ptr(self.decision)
        o.read_hp = _ptr(self.read_hp)
        o.dir_table = _ptr(self.dir_table)
        o.dir_join = _ptr(self.dir_join)
        o.dir_which_way = _ptr(self.dir_which_way)
        o.dir_fisher_p = _ptr(self.dir_fisher_p)
        o.dir_score = _ptr(self.dir_score)
        o.win_n_sites = _ptr(self.win_n_sites)
        o.win_n_reads = _ptr(self.win_n_reads)
        return o


@dataclass
class KnownVars:
    pos: np.ndarray       # u32
    len: np.ndarray       # u32
    op: np.ndarray        # u8
    haptag: np.ndarray    # u8
    char_off: np.ndarray  # u64 [n+1]
    chars: np.ndarray     # u8

    def __post_init__(self):
        self.pos = np.ascontiguousarray(self.pos, np.uint32)
        self.len = np.ascontiguousarray(self.len, np.uint32)
        self.op = np.ascontiguousarray(self.op, np.uint8)
        self.haptag = np.ascontiguousarray(self.haptag, np.uint8)
        self.char_off = np.ascontiguousarray(self.char_off, np.uint64)
        self.chars = np.ascontiguousarray(self.chars if len(self.chars) else np.zeros(1, np.uint8), np.uint8)

    def to_c(self) -> PfKnownVars:
        k = PfKnownVars()
        k.n = int(self.pos.shape[0])
        k.pos, k.len, k.op, k.haptag = _ptr(self.pos), _ptr(self.len), _ptr(self.op), _ptr(self.haptag)
        k.char_off, k.chars = _ptr(self.char_off), _ptr(self.chars)
        return k


@dataclass
class ReadAlnBatch:
    start: np.ndarray      # u32
    end: np.ndarray        # u32
    cigar_off: np.ndarray  # u64
    cigar: np.ndarray      # u32
    seq_off: np.ndarray    # u64
    seq_len: np.ndarray    # u32
    seq: np.ndarray        # u8 packed nibbles
    md_off: np.ndarray     # u64
    md: np.ndarray         # u8 (ASCII)

    def __post_init__(self):
        self.start = np.ascontiguousarray(self.start, np.uint32)
        self.end = np.ascontiguousarray(self.end, np.uint32)
        self.cigar_off = np.ascontiguousarray(self.cigar_off, np.uint64)
        self.cigar = np.ascontiguousarray(self.cigar if len(self.cigar) else np.zeros(1, np.uint32), np.uint32)
        self.seq_off = np.ascontiguousarray(self.seq_off, np.uint64)
        self.seq_len = np.ascontiguousarray(self.seq_len, np.uint32)
        self.seq = np.ascontiguousarray(self.seq if len(self.seq) else np.zeros(1, np.uint8), np.uint8)
        self.md_off = np.ascontiguousarray(self.md_off, np.uint64)
        self.md = np.ascontiguousarray(self.md if len(self.md) else np.zeros(1, np.uint8), np.uint8)

    @property
    def n_reads(self) -> int:
        return int(self.start.shape[0])

    def to_c(self) -> PfReadAlnBatch:
        r = PfReadAlnBatch()
        r.n_reads = self.n_reads
        r.start, r.end = _ptr(self.start), _ptr(self.end)
        r.cigar_off, r.cigar = _ptr(self.cigar_off), _ptr(self.cigar)
        r.seq_off, r.seq_len, r.seq = _ptr(self.seq_off), _ptr(self.seq_len), _ptr(self.seq)
        r.md_off, r.md = _ptr(self.md_off), _ptr(self.md)
        return r


class PfLoadCfg(C.Structure):
    """pf_load_cfg_t (mmr_config_t's loader fields, reference blockjoin.h:7-16)."""
    _fields_ = [("min_mapq", C.c_int32), ("min_len", C.c_int32),
                ("qual_lo", C.c_int32), ("qual_hi", C.c_int32)]


@dataclass
class LoadConfig:
    """Loader parameters; defaults are the CLI's (cli.c:56-70): -q 10, -L 15000,
    ML bands lo 100 / hi 156."""
    min_mapq: int = 10
    min_len: int = 15000
    qual_lo: int = 100
    qual_hi: int = 156

    def to_c(self) -> PfLoadCfg:
        return PfLoadCfg(self.min_mapq, self.min_len, self.qual_lo, self.qual_hi)


class PfPileup(C.Structure):
    """pf_pileup_t: the per-haplotype pileup's CSR (pf_batch_pileup)."""
    _fields_ = [("n_windows", C.c_uint32), ("n_sites", C.c_uint64), ("win_off", C.POINTER(C.c_uint64)),
                ("pos", C.POINTER(C.c_uint32)), ("cnt", C.POINTER(C.c_uint32)), ("ms_kernels", C.c_float)]


class PfHapmethOpts(C.Structure):
    """pf_hapmeth_opts_t (pf_hapmeth_main)."""
    _fields_ = [("bam_path", C.c_char_p), ("out_prefix", C.c_char_p), ("region", C.c_char_p),
                ("chunk_size", C.c_uint32), ("job_windows", C.c_uint32), ("load", PfLoadCfg),
                ("threads", C.c_int32), ("host_fetch", C.c_int32), ("device", C.c_int32), ("verbose", C.c_int32)]


class PfHapmethStats(C.Structure):
    """pf_hapmeth_stats_t."""
    _fields_ = [("n_windows", C.c_uint64), ("n_skipped", C.c_uint64), ("n_records", C.c_uint64),
                ("n_sites", C.c_uint64), ("ms_kernels", C.c_double)]


class PfDmrCfg(C.Structure):
    """pf_dmr_cfg_t."""
    _fields_ = [("min_cov", C.c_uint32), ("min_delta_pct", C.c_uint32), ("max_gap", C.c_uint32),
                ("min_sites", C.c_uint32)]


@dataclass
class DmrConfig:
    """Parameters of the allele-specific region call (pf_dmr_regions): a CpG
    takes part with min_cov calls on each haplotype, carries a direction when
    the haplotypes' methylation differs by min_delta_pct percent, and chains
    to the next one of its direction within max_gap bases; a region needs
    min_sites CpGs."""
    min_cov: int = 5
    min_delta_pct: int = 40
    max_gap: int = 500
    min_sites: int = 5

    def to_c(self) -> PfDmrCfg:
        return PfDmrCfg(self.min_cov, self.min_delta_pct, self.max_gap, self.min_sites)


class PfDmrRun(C.Structure):
    """pf_dmr_run_t."""
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("n_sites", C.c_uint32), ("sign", C.c_int32),
                ("sum", C.c_uint64 * 4), ("open", C.c_uint32), ("reserved", C.c_uint32)]


DMR_RUN_DTYPE = np.dtype([("start", np.uint32), ("end", np.uint32), ("n_sites", np.uint32), ("sign", np.int32),
                          ("sum", np.uint64, (4,)), ("open", np.uint32), ("reserved", np.uint32)])


class PfDmr(C.Structure):
    """pf_dmr_t: the runs of one range (pf_dmr_regions) or the stitched regions."""
    _fields_ = [("n_runs", C.c_uint64), ("runs", C.POINTER(PfDmrRun)), ("n_informative", C.c_uint64),
                ("ms_kernels", C.c_float), ("ms_upload", C.c_float)]


class PfHapmethDmr(C.Structure):
    """pf_hapmeth_dmr_t (pf_hapmeth_run)."""
    _fields_ = [("cfg", PfDmrCfg), ("max_p", C.c_double), ("blocks_path", C.c_char_p)]


class PfHapmethDmrStats(C.Structure):
    """pf_hapmeth_dmr_stats_t."""
    _fields_ = [("n_regions", C.c_uint64), ("n_informative", C.c_uint64), ("ms_kernels", C.c_double)]


class PfDmrHmmCfg(C.Structure):
    """pf_dmr_hmm_cfg_t."""
    _fields_ = [("site_cost_q16", C.c_int32), ("switch_q16", C.c_int32)]


@dataclass
class HmmConfig:
    """Parameters of the hidden Markov model of pf_dmr_hmm_regions, in bits
    (Q16 inside: round(bits * 65536)): site_cost is what every CpG of a region
    pays, switch what opening and what closing a region pays; both in
    [0, 64].  The defaults are choices made on simulated data, not measured on
    real samples."""
    site_cost: float = 2.0
    switch: float = 8.0

    def to_c(self) -> PfDmrHmmCfg:
        return PfDmrHmmCfg(int(round(self.site_cost * 65536)), int(round(self.switch * 65536)))


DMR_HMM_SITES = 1


class PfDmrHmm(C.Structure):
    """pf_dmr_hmm_t: the kept runs of one range under the model (pf_dmr_hmm_regions)."""
    _fields_ = [("n_runs", C.c_uint64), ("runs", C.POINTER(PfDmrRun)), ("n_informative", C.c_uint64),
                ("n_chains", C.c_uint64), ("n_sites", C.c_uint64), ("state", C.POINTER(C.c_uint8)),
                ("evidence", C.POINTER(C.c_int64)), ("ms_kernels", C.c_float), ("ms_upload", C.c_float)]


class PfRegionSum(C.Structure):
    """pf_region_sum_t."""
    _fields_ = [("n_cpg", C.c_uint32), ("n_sites", C.c_uint32), ("n_pos", C.c_uint32), ("n_neg", C.c_uint32),
                ("sum", C.c_uint64 * 4), ("evidence", C.c_int64)]


REGION_SUM_DTYPE = np.dtype([("n_cpg", np.uint32), ("n_sites", np.uint32), ("n_pos", np.uint32), ("n_neg", np.uint32),
                             ("sum", np.uint64, (4,)), ("evidence", np.int64)])


class PfRegions(C.Structure):
    """pf_regions_t: the sums of the caller's regions over one range (pf_region_sums)."""
    _fields_ = [("n", C.c_uint64), ("r", C.POINTER(PfRegionSum)), ("n_informative", C.c_uint64),
                ("ms_kernels", C.c_float), ("ms_upload", C.c_float)]


class PfRegionRec(C.Structure):
    """pf_region_rec_t: one line of {prefix}.hapmeth.regions.bed (pf_write_regions)."""
    _fields_ = [("chrom", C.c_char_p), ("name", C.c_char_p), ("start", C.c_uint32), ("end", C.c_uint32),
                ("s", PfRegionSum), ("flags", C.c_uint32), ("reads", C.c_uint32 * 2), ("hits", C.c_uint32),
                ("status", C.c_uint32)]


REGION_SPLIT, REGION_ELIGIBLE = 1, 2
REGION_TEST_MAX_SPAN = 1_000_000


class PfHapmethRegions(C.Structure):
    """pf_hapmeth_regions_t (pf_hapmeth_run_regions)."""
    _fields_ = [("bed_path", C.c_char_p)]


class PfHapmethRegionsStats(C.Structure):
    """pf_hapmeth_regions_stats_t."""
    _fields_ = [("n_regions", C.c_uint64), ("n_unknown_contig", C.c_uint64), ("n_outside", C.c_uint64),
                ("n_split", C.c_uint64), ("n_tested", C.c_uint64), ("n_untested", C.c_uint64),
                ("ms_kernels", C.c_double)]


class PfHapmethHmm(C.Structure):
    """pf_hapmeth_hmm_t (pf_hapmeth_run_hmm)."""
    _fields_ = [("cfg", PfDmrHmmCfg)]


class PfHapmethHmmStats(C.Structure):
    """pf_hapmeth_hmm_stats_t."""
    _fields_ = [("n_chains", C.c_uint64), ("ms_kernels", C.c_double)]


class PfPerm(C.Structure):
    """pf_perm_t: the permutation test of a batch's windows (pf_batch_permtest)."""
    _fields_ = [("n_windows", C.c_uint32), ("n_perm", C.c_uint32), ("seed", C.c_uint32),
                ("n_reads", C.POINTER(C.c_uint32)), ("sum", C.POINTER(C.c_uint64)), ("hits", C.POINTER(C.c_uint32)),
                ("status", C.POINTER(C.c_uint32)), ("ms_kernels", C.c_float)]


class PfHapmethPerm(C.Structure):
    """pf_hapmeth_perm_t (pf_hapmeth_run_perm)."""
    _fields_ = [("n_perm", C.c_uint32), ("seed", C.c_uint32)]


class PfHapmethPermStats(C.Structure):
    """pf_hapmeth_perm_stats_t."""
    _fields_ = [("n_tested", C.c_uint64), ("n_untested", C.c_uint64), ("n_records", C.c_uint64),
                ("ms_kernels", C.c_double)]


class PfRank(C.Structure):
    """pf_rank_t: the rank-sum test of a batch's windows (pf_batch_ranktest)."""
    _fields_ = [("n_windows", C.c_uint32), ("min_calls", C.c_uint32), ("n_reads", C.POINTER(C.c_uint32)),
                ("n_short", C.POINTER(C.c_uint32)), ("cls", C.POINTER(C.c_uint32)), ("sum", C.POINTER(C.c_uint64)),
                ("u2", C.POINTER(C.c_uint64)), ("ties", C.POINTER(C.c_uint64)), ("status", C.POINTER(C.c_uint32)),
                ("ms_kernels", C.c_float)]


class PfRankRec(C.Structure):
    """pf_rank_rec_t: one line of {prefix}.hapmeth.rank.tsv (pf_write_rank)."""
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_uint32), ("end", C.c_uint32), ("reads", C.c_uint32 * 2),
                ("n_short", C.c_uint32 * 2), ("cls", C.c_uint32 * 6), ("status", C.c_uint32), ("u2", C.c_uint64),
                ("ties", C.c_uint64)]


class PfHapmethRank(C.Structure):
    """pf_hapmeth_rank_t (pf_hapmeth_run_rank)."""
    _fields_ = [("min_calls", C.c_uint32)]


class PfHapmethRankStats(C.Structure):
    """pf_hapmeth_rank_stats_t."""
    _fields_ = [("n_tested", C.c_uint64), ("n_untested", C.c_uint64), ("n_records", C.c_uint64),
                ("ms_kernels", C.c_double)]


class PfRankExact(C.Structure):
    """pf_rank_exact_t: the exact rank-sum counts of a batch's windows (pf_batch_rankexact)."""
    _fields_ = [("n_windows", C.c_uint32), ("min_calls", C.c_uint32), ("max_reads", C.c_uint32),
                ("n_reads", C.POINTER(C.c_uint32)), ("n_short", C.POINTER(C.c_uint32)), ("status", C.POINTER(C.c_uint32)),
                ("u2", C.POINTER(C.c_uint64)), ("total", C.POINTER(C.c_uint64)), ("le", C.POINTER(C.c_uint64)),
                ("ge", C.POINTER(C.c_uint64)), ("two", C.POINTER(C.c_uint64)), ("ms_kernels", C.c_float)]


class PfRankExactRec(C.Structure):
    """pf_rank_exact_rec_t: the exact test beside a PfRankRec (pf_write_rank_exact)."""
    _fields_ = [("two", C.c_uint64), ("total", C.c_uint64), ("status", C.c_uint32)]


class PfHapmethRankExact(C.Structure):
    """pf_hapmeth_rank_exact_t (pf_hapmeth_run_rank_exact)."""
    _fields_ = [("max_reads", C.c_uint32)]


class PfHapmethRankExactStats(C.Structure):
    """pf_hapmeth_rank_exact_stats_t."""
    _fields_ = [("n_exact", C.c_uint64), ("n_over", C.c_uint64), ("ms_kernels", C.c_double)]


class PfRankTileRec(C.Structure):
    """pf_rank_tile_rec_t: a tile's counts and split flag beside a PfRankRec (pf_write_rank_tiles)."""
    _fields_ = [("sum", C.c_uint64 * 4), ("split", C.c_uint32)]


class PfHapmethTiles(C.Structure):
    """pf_hapmeth_tiles_t (pf_hapmeth_run_tiles)."""
    _fields_ = [("tile", C.c_uint32), ("min_calls", C.c_uint32), ("blocks_path", C.c_char_p)]


class PfHapmethTilesStats(C.Structure):
    """pf_hapmeth_tiles_stats_t."""
    _fields_ = [("n_tiles", C.c_uint64), ("n_written", C.c_uint64), ("n_tested", C.c_uint64), ("n_split", C.c_uint64),
                ("ms_kernels", C.c_double)]


class PfAssignCfg(C.Structure):
    """pf_assign_cfg_t."""
    _fields_ = [("min_cov", C.c_uint32), ("min_calls", C.c_uint32), ("min_llr_q16", C.c_int64)]


@dataclass
class AssignConfig:
    """Parameters of the tag assignment (pf_batch_assign): a CpG enters the
    model with min_cov calls on each haplotype (hapmeth_files takes the
    DmrConfig's instead), an untagged read gets a tag with at least min_calls
    calls at such CpGs and log2 odds of at least min_llr bits (Q16 inside:
    round(min_llr * 65536)).  The two defaults -- odds of 8:1, two calls --
    are choices, not measured optima."""
    min_cov: int = 5
    min_calls: int = 2
    min_llr: float = 3.0

    @property
    def min_llr_q16(self) -> int:
        return int(round(self.min_llr * 65536))

    def to_c(self) -> PfAssignCfg:
        return PfAssignCfg(self.min_cov, self.min_calls, self.min_llr_q16)


class PfAssign(C.Structure):
    """pf_assign_t: the scores and new tags of a batch's untagged reads (pf_batch_assign)."""
    _fields_ = [("n_windows", C.c_uint32), ("n_reads", C.c_uint32), ("win_read_off", C.POINTER(C.c_uint32)),
                ("n_used", C.POINTER(C.c_uint32)), ("llr", C.POINTER(C.c_int64)), ("hp", C.POINTER(C.c_uint8)),
                ("win_n", C.POINTER(C.c_uint32)), ("ms_kernels", C.c_float)]


class PfHapmethAssign(C.Structure):
    """pf_hapmeth_assign_t (pf_hapmeth_run_assign)."""
    _fields_ = [("min_llr_q16", C.c_int64), ("min_calls", C.c_uint32), ("reserved", C.c_uint32)]


class PfHapmethAssignStats(C.Structure):
    """pf_hapmeth_assign_stats_t."""
    _fields_ = [("n_lines", C.c_uint64), ("n_h1", C.c_uint64), ("n_h2", C.c_uint64), ("n_records", C.c_uint64),
                ("ms_kernels", C.c_double)]


class PfTagcheck(C.Structure):
    """pf_tagcheck_t: the leave-one-out scores and verdicts of a batch's tagged reads (pf_batch_tagcheck)."""
    _fields_ = [("n_windows", C.c_uint32), ("n_reads", C.c_uint32), ("win_read_off", C.POINTER(C.c_uint32)),
                ("n_used", C.POINTER(C.c_uint32)), ("llr", C.POINTER(C.c_int64)), ("verdict", C.POINTER(C.c_uint8)),
                ("hp", C.POINTER(C.c_uint8)), ("win_n", C.POINTER(C.c_uint32)), ("ms_kernels", C.c_float)]


TAGCHECK_OK, TAGCHECK_FLIP, TAGCHECK_UNDECIDED, TAGCHECK_NOT_SCORED = 0, 1, 2, 255
HAPMETH_TAGCHECK_RULE_ONLY = 1


class PfHapmethTagcheck(C.Structure):
    """pf_hapmeth_tagcheck_t (pf_hapmeth_run_tagcheck)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PfHapmethTagcheckStats(C.Structure):
    """pf_hapmeth_tagcheck_stats_t."""
    _fields_ = [("n_lines", C.c_uint64), ("n_regions", C.c_uint64), ("n_ok", C.c_uint64 * 2), ("n_flip", C.c_uint64 * 2),
                ("n_undecided", C.c_uint64 * 2), ("n_records", C.c_uint64), ("ms_kernels", C.c_double)]


class PfAlnBatch(C.Structure):
    _fields_ = [("n_windows", C.c_uint32), ("n_recs", C.c_uint32)] + [
        (n, C.c_void_p) for n in (
            "win_start", "win_end", "win_rec_off", "win_cov_sel", "win_cov_rt", "win_n_cand",
            "flag", "mapq", "pos", "l_qseq", "de", "hp", "cigar_off", "cigar", "seq_off", "seq",
            "mm_off", "mm", "ml_off", "ml")]


_ALN_FIELDS = {
    "win_start": np.uint32, "win_end": np.uint32, "win_rec_off": np.uint32,
    "flag": np.uint16, "mapq": np.uint8, "pos": np.uint32, "l_qseq": np.uint32, "de": np.float32,
    "hp": np.uint8, "cigar_off": np.uint64, "cigar": np.uint32, "seq_off": np.uint64, "seq": np.uint8,
    "mm_off": np.uint64, "mm": np.uint8, "ml_off": np.uint64, "ml": np.uint8,
}


@dataclass
class AlnBatch:
    """Record-level host SoA of a batch of windows (pf_aln_batch_t): the BAM
    records each window's region query returned, in BAM order."""
    win_start: np.ndarray
    win_end: np.ndarray
    win_rec_off: np.ndarray
    flag: np.ndarray
    mapq: np.ndarray
    pos: np.ndarray
    l_qseq: np.ndarray
    de: np.ndarray
    hp: np.ndarray
    cigar_off: np.ndarray
    cigar: np.ndarray
    seq_off: np.ndarray
    seq: np.ndarray
    mm_off: np.ndarray
    mm: np.ndarray
    ml_off: np.ndarray
    ml: np.ndarray
    win_cov_sel: Optional[np.ndarray] = None
    win_cov_rt: Optional[np.ndarray] = None
    win_n_cand: Optional[np.ndarray] = None
    meta: dict = field(default_factory=dict)

    def __post_init__(self):
        for name, dt in _ALN_FIELDS.items():
            a = np.ascontiguousarray(getattr(self, name), dtype=dt)
            if name in ("cigar", "seq", "mm", "ml") and a.size == 0:
                a = np.zeros(1, dt)      # keep a valid pointer for empty arenas
            setattr(self, name, a)
        for name in ("win_cov_sel", "win_cov_rt", "win_n_cand"):
            v = getattr(self, name)
            if v is not None:
                setattr(self, name, np.ascontiguousarray(v, dtype=np.int32))

    @property
    def n_windows(self) -> int:
        return int(self.win_start.shape[0])

    @property
    def n_recs(self) -> int:
        return int(self.pos.shape[0])

    def to_c(self) -> PfAlnBatch:
        b = PfAlnBatch()
        b.n_windows = self.n_windows
        b.n_recs = self.n_recs
        for name in _ALN_FIELDS:
            setattr(b, name, _ptr(getattr(self, name)))
        for name in ("win_cov_sel", "win_cov_rt", "win_n_cand"):
            setattr(b, name, _ptr(getattr(self, name)))
        return b

    def nbytes(self) -> int:
        return int(sum(getattr(self, n).nbytes for n in _ALN_FIELDS))

    def select(self, windows) -> "AlnBatch":
        """Sub-batch with the given window indices (records re-packed)."""
        windows = np.asarray(windows, dtype=np.int64)
        wo = self.win_rec_off.astype(np.int64)
        recs = [np.arange(wo[w], wo[w + 1]) for w in windows]
        recs = np.concatenate(recs) if recs else np.zeros(0, np.int64)
        cnt = np.array([wo[w + 1] - wo[w] for w in windows], dtype=np.int64)

        def gather(off, data):
            off = np.asarray(off, np.int64)
            lo, hi = off[recs], off[recs + 1]
            sizes = hi - lo
            noff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
            parts = [data[a:b] for a, b in zip(lo.tolist(), hi.tolist())]
            return noff, (np.concatenate(parts) if parts else data[:0])

        co, cg = gather(self.cigar_off, self.cigar)
        lq = self.l_qseq.astype(np.int64)
        so = np.asarray(self.seq_off, np.int64)
        sparts = [self.seq[so[r]:so[r] + (lq[r] + 1) // 2] for r in recs.tolist()]
        sq = np.concatenate(sparts) if sparts else self.seq[:0]
        soff = np.concatenate([[0], np.cumsum([(lq[r] + 1) // 2 for r in recs.tolist()])]).astype(np.uint64)
        mo, mm = gather(self.mm_off, self.mm)
        lo_, ml = gather(self.ml_off, self.ml)
        opt = {n: (None if getattr(self, n) is None else getattr(self, n)[windows])
               for n in ("win_cov_sel", "win_cov_rt", "win_n_cand")}
        return AlnBatch(win_start=self.win_start[windows], win_end=self.win_end[windows],
                        win_rec_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32),
                        flag=self.flag[recs], mapq=self.mapq[recs], pos=self.pos[recs], l_qseq=self.l_qseq[recs],
                        de=self.de[recs], hp=self.hp[recs], cigar_off=co, cigar=cg, seq_off=soff, seq=sq,
                        mm_off=mo, mm=mm, ml_off=lo_, ml=ml, **opt)
