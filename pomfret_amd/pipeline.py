"""`pomfret methphase` / `pomfret report` end to end: a thin binding of the C
pipeline driver (pomfret_amd/csrc/pf_pipeline.c, the pf_methphase_main /
pf_mp_* entry points of include/pomfret_amd.h).  The host side is C:

    f3  pf_vcf_gaps                 phase-block gaps of the phased VCF
                                    (load_intervals_from_file + merge_close_intervals,
                                    blockjoin.c:4442-4523)
    -u  pf_haptag_reads per contig  K4 pre-pass, qname first-wins per contig,
                                    merged in contig order (1841-1898, 2069-2080)
    f1  pf_bam_fetch_windows        each job's records (1053-1076), overlapped
                                    with the previous job's kernels
    GPU pf_batch_upload_aln + pf_methphase_run: K0 loader, K12, K3 (the kt_for
                                    worker, 4340-4426)
    a1  first-wins qname -> hp of joined windows, in (contig, window) order
                                    (4408-4423, 4572-4595), a C table (pf_tags_t)
    f2  pf_phase_blocks, pf_write_gtf / _tsv / _vcf + pf_rescue_dropped
                                    (lift_decisions ... output_modify_vcf, 4685-4717)

`methphase_files` runs everything in this process (one host thread per GPU
it drives).  `methphase_files_dist` is the one-process-per-GPU form: every
rank builds the same plan, runs the jobs its static LPT shard owns, and the
job results (per-window decisions + the joined windows' qname/tag lists)
are gathered over torch.distributed to rank 0, which merges them in window
order and writes the outputs -- the merged tables equal the single-process
ones exactly.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional

import numpy as np

from ._lib import (INTERVALS_GTF, INTERVALS_TSV, INTERVALS_VCF, PomfretError, _blocks_contigs, _check,  # noqa: F401
                   _breaks, _dmr_dict, _dmr_to_c, _gaps_contigs, _PfBlocks, _PfGaps, lib)
from .abi import (Config, DmrConfig, LoadConfig, PfCfg, PfDmr, PfHapmethDmr, PfHapmethDmrStats, PfHapmethOpts,
                  AssignConfig, HAPMETH_TAGCHECK_RULE_ONLY, PfAssign, PfHapmethAssign, PfHapmethAssignStats,
                  PfHapmethTagcheck, PfHapmethTagcheckStats, PfTagcheck, PfHapmethPerm, PfHapmethPermStats, PfHapmethStats, PfLoadCfg, PfPerm, PfPileup,
                  HmmConfig, PfHapmethHmm, PfHapmethHmmStats, PfHapmethRegions, PfHapmethRegionsStats, PfRegionRec,
                  PfHapmethRank, PfHapmethRankStats, PfRankRec, PfHapmethRankExact, PfHapmethRankExactStats, PfRankExactRec,
                  PfHapmethTiles, PfHapmethTilesStats, PfRankTileRec, REGION_ELIGIBLE, REGION_SPLIT)

MODE_METHPHASE, MODE_REPORT = 0, 1
JOB_WINDOWS, JOB_HAPTAG = 0, 1


class PfMethphaseOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("bam_path", C.c_char_p), ("vcf_path", C.c_char_p),
                ("out_prefix", C.c_char_p), ("cov_for_selection", C.c_int32), ("cov_for_runtime", C.c_int32),
                ("n_cand", C.c_int32), ("cov", C.c_int32), ("k", C.c_int32), ("k_span", C.c_int32),
                ("load", PfLoadCfg), ("untagged", C.c_int32), ("write_tsv", C.c_int32), ("write_bam", C.c_int32),
                ("chunk_size", C.c_int32), ("chunk_stride", C.c_int32), ("threads", C.c_int32),
                ("n_devices", C.c_int32), ("devices", C.c_void_p), ("ctxs", C.c_void_p), ("n_ctxs", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32), ("job_windows", C.c_uint32), ("verbose", C.c_int32),
                ("host_fetch", C.c_int32), ("interval_path", C.c_char_p), ("interval_format", C.c_int32),
                ("write_input_tagging", C.c_int32), ("bam_threads", C.c_int32),
                ("mask_path", C.c_char_p), ("mask_variants", C.c_int32),
                ("ref_path", C.c_char_p)]


class PfQnameTagsC(C.Structure):
    _fields_ = [("n", C.c_uint32), ("off", C.c_void_p), ("names", C.c_void_p), ("hp", C.c_void_p)]


class PfMpJobInfo(C.Structure):
    _fields_ = [("contig", C.c_uint32), ("contig_name", C.c_char_p), ("w0", C.c_uint32), ("w1", C.c_uint32),
                ("rank", C.c_int32), ("lpt_pos", C.c_uint32), ("cost", C.c_double), ("done", C.c_int32),
                ("cfg", PfCfg)]


class PfMpStats(C.Structure):
    _fields_ = [("s_plan", C.c_double), ("s_estimate", C.c_double), ("s_haptag", C.c_double),
                ("s_windows", C.c_double), ("s_finish", C.c_double), ("fetch_ms", (C.c_double * 7) * 2),
                ("comp_bytes", C.c_uint64 * 2), ("inflated_bytes", C.c_uint64 * 2), ("run_ms", C.c_double * 2),
                ("n_fetch", C.c_uint64 * 2), ("arena_hits", C.c_uint64), ("arena_misses", C.c_uint64),
                ("reread_bytes", C.c_uint64), ("steals", C.c_uint64)]


class PfMpJobResult(C.Structure):
    _fields_ = [("n_windows", C.c_uint32), ("decision", C.c_void_p), ("tag_off", C.c_void_p),
                ("tags", PfQnameTagsC), ("n_limit", C.c_uint32)]


_bound = False


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    L.pf_methphase_main.argtypes = [C.POINTER(PfMethphaseOpts), C.POINTER(vp)]
    L.pf_mp_plan.argtypes = [C.POINTER(PfMethphaseOpts), C.POINTER(vp)]
    L.pf_mp_free.argtypes = [vp]
    L.pf_mp_n_jobs.argtypes = [vp, i32]
    L.pf_mp_n_jobs.restype = u32
    L.pf_mp_job_info.argtypes = [vp, i32, u32, C.POINTER(PfMpJobInfo)]
    L.pf_mp_windows.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32)]
    L.pf_mp_run_mine.argtypes = [vp, C.POINTER(PfMethphaseOpts), i32]
    L.pf_mp_run_job.argtypes = [vp, vp, u32]
    L.pf_mp_run_haptag_job.argtypes = [vp, vp, u32]
    L.pf_mp_merge_raw.argtypes = [vp]
    L.pf_mp_get_job_result.argtypes = [vp, i32, u32, C.POINTER(PfMpJobResult)]
    L.pf_mp_set_job_result.argtypes = [vp, i32, u32, C.POINTER(PfMpJobResult)]
    L.pf_mp_finish.argtypes = [vp]
    L.pf_mp_decisions.argtypes = [vp, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.pf_mp_gaps.argtypes = [vp]
    L.pf_mp_gaps.restype = C.POINTER(_PfGaps)
    L.pf_mp_blocks.argtypes = [vp]
    L.pf_mp_blocks.restype = C.POINTER(_PfBlocks)
    L.pf_mp_qname_hp.argtypes = [vp]
    L.pf_mp_qname_hp.restype = vp
    L.pf_mp_raw_hp.argtypes = [vp]
    L.pf_mp_raw_hp.restype = vp
    L.pf_mp_report_counts.argtypes = [vp, C.POINTER(C.c_double)]
    L.pf_mp_stats.argtypes = [vp, C.POINTER(PfMpStats)]
    L.pf_mp_masked_sites.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.pf_mask_load.argtypes = [C.c_char_p, C.c_char_p, u32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.pf_mask_contig.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.pf_mask_free.argtypes = [vp]
    L.pf_hapmeth_main.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethStats)]
    L.pf_hapmeth_run.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethStats),
                                 C.POINTER(PfHapmethDmrStats)]
    L.pf_hapmeth_run_perm.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethPerm),
                                      C.POINTER(PfHapmethStats), C.POINTER(PfHapmethDmrStats),
                                      C.POINTER(PfHapmethPermStats)]
    L.pf_hapmeth_run_assign.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethPerm),
                                        C.POINTER(PfHapmethAssign), C.POINTER(PfHapmethStats),
                                        C.POINTER(PfHapmethDmrStats), C.POINTER(PfHapmethPermStats),
                                        C.POINTER(PfHapmethAssignStats)]
    L.pf_hapmeth_run_tagcheck.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethPerm),
                                          C.POINTER(PfHapmethAssign), C.POINTER(PfHapmethTagcheck),
                                          C.POINTER(PfHapmethStats), C.POINTER(PfHapmethDmrStats),
                                          C.POINTER(PfHapmethPermStats), C.POINTER(PfHapmethAssignStats),
                                          C.POINTER(PfHapmethTagcheckStats)]
    L.pf_hapmeth_run_hmm.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethHmm),
                                     C.POINTER(PfHapmethPerm), C.POINTER(PfHapmethAssign), C.POINTER(PfHapmethTagcheck),
                                     C.POINTER(PfHapmethStats), C.POINTER(PfHapmethDmrStats), C.POINTER(PfHapmethHmmStats),
                                     C.POINTER(PfHapmethPermStats), C.POINTER(PfHapmethAssignStats),
                                     C.POINTER(PfHapmethTagcheckStats)]
    L.pf_hapmeth_run_regions.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethHmm),
                                         C.POINTER(PfHapmethPerm), C.POINTER(PfHapmethAssign), C.POINTER(PfHapmethTagcheck),
                                         C.POINTER(PfHapmethRegions), C.POINTER(PfHapmethStats),
                                         C.POINTER(PfHapmethDmrStats), C.POINTER(PfHapmethHmmStats),
                                         C.POINTER(PfHapmethPermStats), C.POINTER(PfHapmethAssignStats),
                                         C.POINTER(PfHapmethTagcheckStats), C.POINTER(PfHapmethRegionsStats)]
    L.pf_hapmeth_run_rank.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethHmm),
                                      C.POINTER(PfHapmethPerm), C.POINTER(PfHapmethAssign), C.POINTER(PfHapmethTagcheck),
                                      C.POINTER(PfHapmethRegions), C.POINTER(PfHapmethRank), C.POINTER(PfHapmethStats),
                                      C.POINTER(PfHapmethDmrStats), C.POINTER(PfHapmethHmmStats),
                                      C.POINTER(PfHapmethPermStats), C.POINTER(PfHapmethAssignStats),
                                      C.POINTER(PfHapmethTagcheckStats), C.POINTER(PfHapmethRegionsStats),
                                      C.POINTER(PfHapmethRankStats)]
    L.pf_hapmeth_run_rank_exact.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethHmm),
                                            C.POINTER(PfHapmethPerm), C.POINTER(PfHapmethAssign),
                                            C.POINTER(PfHapmethTagcheck), C.POINTER(PfHapmethRegions),
                                            C.POINTER(PfHapmethRank), C.POINTER(PfHapmethRankExact), C.POINTER(PfHapmethStats),
                                            C.POINTER(PfHapmethDmrStats), C.POINTER(PfHapmethHmmStats),
                                            C.POINTER(PfHapmethPermStats), C.POINTER(PfHapmethAssignStats),
                                            C.POINTER(PfHapmethTagcheckStats), C.POINTER(PfHapmethRegionsStats),
                                            C.POINTER(PfHapmethRankStats), C.POINTER(PfHapmethRankExactStats)]
    L.pf_write_rank_exact.argtypes = [C.c_char_p, C.POINTER(PfRankRec), C.POINTER(PfRankExactRec), C.c_uint64, C.c_int,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.pf_hapmeth_run_tiles.argtypes = [C.POINTER(PfHapmethOpts), C.POINTER(PfHapmethDmr), C.POINTER(PfHapmethHmm),
                                       C.POINTER(PfHapmethPerm), C.POINTER(PfHapmethAssign), C.POINTER(PfHapmethTagcheck),
                                       C.POINTER(PfHapmethRegions), C.POINTER(PfHapmethRank), C.POINTER(PfHapmethRankExact),
                                       C.POINTER(PfHapmethTiles), C.POINTER(PfHapmethStats), C.POINTER(PfHapmethDmrStats),
                                       C.POINTER(PfHapmethHmmStats), C.POINTER(PfHapmethPermStats),
                                       C.POINTER(PfHapmethAssignStats), C.POINTER(PfHapmethTagcheckStats),
                                       C.POINTER(PfHapmethRegionsStats), C.POINTER(PfHapmethRankStats),
                                       C.POINTER(PfHapmethRankExactStats), C.POINTER(PfHapmethTilesStats)]
    L.pf_write_rank_tiles.argtypes = [C.c_char_p, C.POINTER(PfRankRec), C.POINTER(PfRankTileRec), C.c_uint64,
                                      C.POINTER(C.c_uint64)]
    L.pf_bh_adjust_p.argtypes = [vp, vp, C.c_uint64, vp]
    L.pf_write_rank.argtypes = [C.c_char_p, C.POINTER(PfRankRec), C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.pf_regions_load.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(vp)]
    L.pf_regions_contig.argtypes = [vp, C.c_uint32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)),
                                    C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.c_uint64)]
    L.pf_regions_unknown.argtypes = [vp]
    L.pf_regions_unknown.restype = C.c_uint64
    L.pf_region_list_free.argtypes = [vp]
    L.pf_bh_adjust.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp]
    L.pf_write_regions.argtypes = [C.c_char_p, C.POINTER(PfRegionRec), C.c_uint64, C.c_int, C.c_uint32,
                                   C.POINTER(C.c_uint64)]
    L.pf_tags_new.restype = vp
    L.pf_tags_free.argtypes = [vp]
    L.pf_tags_size.argtypes = [vp]
    L.pf_tags_size.restype = C.c_uint64
    L.pf_tags_put_first.argtypes = [vp, u32, vp, vp, vp]
    L.pf_tags_put_first.restype = C.c_int64
    L.pf_tags_get.argtypes = [vp, u32, vp, vp, C.c_uint8, vp]
    L.pf_tags_get.restype = C.c_int64
    L.pf_tags_view.argtypes = [vp, C.POINTER(PfQnameTagsC)]
    _bound = True
    return L


def _arr(ptr, n, dt) -> np.ndarray:
    n = int(n)
    if n == 0 or not ptr:
        return np.zeros(0, dt)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), (n,)).copy()


def _names_list(off: np.ndarray, names: np.ndarray) -> List[str]:
    b = names.tobytes()
    return [b[off[i]:off[i + 1]].decode("ascii", "replace") for i in range(len(off) - 1)]


def _pack_names(names: List[str]):
    enc = [q.encode() for q in names]
    off = np.zeros(len(enc) + 1, np.uint64)
    if enc:
        off[1:] = np.cumsum([len(q) for q in enc])
    buf = np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy()
    return off, buf


def tags_dict(t) -> Dict[str, int]:
    """A pf_tags_t as {qname: hp} in insertion order."""
    L = _bind()
    if not t:
        return {}
    v = PfQnameTagsC()
    _check(L.pf_tags_view(t, C.byref(v)), "pf_tags_view")
    off = _arr(v.off, v.n + 1, np.uint64)
    names = _arr(v.names, off[-1] if v.n else 0, np.uint8)
    hp = _arr(v.hp, v.n, np.uint8)
    return dict(zip(_names_list(off, names), hp.tolist()))


class Tags:
    """Owned pf_tags_t (first-wins qname -> hp)."""

    def __init__(self):
        self.h = _bind().pf_tags_new()
        if not self.h:
            raise PomfretError("pf_tags_new")

    def put_first(self, names: List[str], hp) -> int:
        off, buf = _pack_names(names)
        hp = np.ascontiguousarray(np.asarray(hp, np.uint8) if len(names) else np.zeros(1, np.uint8))
        r = lib().pf_tags_put_first(self.h, len(names), off.ctypes.data, buf.ctypes.data, hp.ctypes.data)
        if r < 0:
            _check(int(r), "pf_tags_put_first")
        return int(r)

    def get(self, names: List[str], default: int = 254) -> np.ndarray:
        off, buf = _pack_names(names)
        out = np.zeros(max(len(names), 1), np.uint8)
        r = lib().pf_tags_get(self.h, len(names), off.ctypes.data, buf.ctypes.data, default, out.ctypes.data)
        if r < 0:
            _check(int(r), "pf_tags_get")
        return out[:len(names)]

    def __len__(self):
        return int(lib().pf_tags_size(self.h))

    def to_dict(self) -> Dict[str, int]:
        return tags_dict(self.h)

    def close(self):
        if self.h:
            lib().pf_tags_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_opts(bam_path: str, vcf_path: str, out_prefix: Optional[str], cfg: Optional[Config],
              lcfg: Optional[LoadConfig] = None, mode: int = MODE_METHPHASE, untagged: bool = False,
              tsv: bool = False, threads: int = 8, n_devices: int = 0, ctxs=None, rank: int = 0, world: int = 1,
              job_windows: int = 0, cov: int = 0, chunk_size: int = 50_000, chunk_stride: int = 1_000_000,
              verbose: int = 0, host_fetch: bool = False, intervals=None, write_input_tagging: bool = False,
              mask_bed: Optional[str] = None, mask_variants: bool = False, ref: Optional[str] = None):
    """pf_methphase_opts_t from Python values.  cfg None: per-contig
    parameters from the BAM's coverage estimate (runs without -c).
    intervals: (path, INTERVALS_GTF | INTERVALS_TSV), the --gtf / --tsv phase
    blocks (vcf_path may then be None unless untagged).  mask_bed /
    mask_variants: --mask-bed / --mask-variants, reference positions no
    methylation site may lie on (load_mask).  ref: --ref, a reference FASTA
    the -u pre-pass and the rescue synthesise MD from (the BAM then needs no
    MD:Z tags)."""
    lcfg = lcfg or LoadConfig()
    o = PfMethphaseOpts()
    o.mode = mode
    o.bam_path = bam_path.encode()
    o.vcf_path = vcf_path.encode() if vcf_path else None
    if intervals is not None:
        o.interval_path = intervals[0].encode()
        o.interval_format = int(intervals[1])
    o.write_input_tagging = int(bool(write_input_tagging))
    o.out_prefix = out_prefix.encode() if out_prefix else None
    if cfg is not None:
        o.cov_for_selection, o.cov_for_runtime, o.n_cand = cfg.cov_for_selection, cfg.cov_for_runtime, cfg.n_cand
        o.k, o.k_span = cfg.k, cfg.k_span
    else:
        o.cov_for_selection, o.cov_for_runtime, o.n_cand, o.k, o.k_span = -1, 0, 15, 3, 5000
    o.cov = int(cov)
    o.load = lcfg.to_c()
    o.untagged = int(bool(untagged))
    o.write_tsv = int(bool(tsv))
    o.chunk_size, o.chunk_stride = int(chunk_size), int(chunk_stride)
    o.threads = int(threads)
    o.n_devices = int(n_devices)
    keep = None
    if ctxs:
        keep = (C.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
        o.ctxs = C.cast(keep, C.c_void_p)
        o.n_ctxs = len(ctxs)
    o.rank, o.world = int(rank), int(world)
    o.job_windows = int(job_windows)
    o.verbose = int(verbose)
    o.host_fetch = int(bool(host_fetch))
    o.mask_path = mask_bed.encode() if mask_bed else None
    o.mask_variants = int(bool(mask_variants))
    o.ref_path = ref.encode() if ref else None
    o._keep = keep
    return o


class Plan:
    """A pf_mp_plan_t: the deterministic job list of one run and its results."""

    def __init__(self, opts: PfMethphaseOpts, handle=None):
        L = _bind()
        self.opts = opts
        if handle is None:
            h = C.c_void_p()
            _check(L.pf_mp_plan(C.byref(opts), C.byref(h)), "pf_mp_plan")
            handle = h
        self.h = handle

    def n_jobs(self, kind: int = JOB_WINDOWS) -> int:
        return int(lib().pf_mp_n_jobs(self.h, kind))

    def job_info(self, kind: int, j: int) -> dict:
        i = PfMpJobInfo()
        _check(lib().pf_mp_job_info(self.h, kind, j, C.byref(i)), "pf_mp_job_info")
        c = i.cfg
        return dict(contig=int(i.contig), contig_name=i.contig_name.decode(), w0=int(i.w0), w1=int(i.w1),
                    rank=int(i.rank), lpt_pos=int(i.lpt_pos), cost=float(i.cost), done=bool(i.done),
                    cfg=Config(k=c.k, k_span=c.k_span, cov_for_selection=c.cov_for_selection,
                               cov_for_runtime=c.cov_for_runtime, n_cand=c.n_cand))

    def windows(self):
        ws, we, co, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        _check(lib().pf_mp_windows(self.h, C.byref(ws), C.byref(we), C.byref(co), C.byref(n)), "pf_mp_windows")
        nc = int(lib().pf_mp_gaps(self.h).contents.n_contigs)
        return _arr(ws, n.value, np.uint32), _arr(we, n.value, np.uint32), _arr(co, nc + 1, np.uint64)

    def run_mine(self, kind: int, n_devices: int = 0, ctxs=None):
        o = make_opts("", "", None, None, threads=self.opts.threads, n_devices=n_devices, ctxs=ctxs,
                      rank=self.opts.rank, world=self.opts.world)
        _check(lib().pf_mp_run_mine(self.h, C.byref(o), kind), "pf_mp_run_mine")

    def merge_raw(self):
        _check(lib().pf_mp_merge_raw(self.h), "pf_mp_merge_raw")

    def get_result(self, kind: int, j: int) -> dict:
        r = PfMpJobResult()
        _check(lib().pf_mp_get_job_result(self.h, kind, j, C.byref(r)), "pf_mp_get_job_result")
        n, t = int(r.n_windows), r.tags
        off = _arr(t.off, t.n + 1, np.uint64)
        return dict(decision=_arr(r.decision, n, np.int8), tag_off=_arr(r.tag_off, n + 1, np.uint64),
                    off=off, names=_arr(t.names, off[-1] if t.n else 0, np.uint8), hp=_arr(t.hp, t.n, np.uint8),
                    n_limit=int(r.n_limit))

    def set_result(self, kind: int, j: int, res: dict):
        dec = np.ascontiguousarray(res["decision"], np.int8)
        n = dec.shape[0]
        to = np.ascontiguousarray(res.get("tag_off", np.zeros(n + 1, np.uint64)), np.uint64)
        off = np.ascontiguousarray(res["off"], np.uint64)
        names = np.ascontiguousarray(res["names"] if len(res["names"]) else np.zeros(1, np.uint8), np.uint8)
        hp = np.ascontiguousarray(res["hp"] if len(res["hp"]) else np.zeros(1, np.uint8), np.uint8)
        decp = np.ascontiguousarray(dec if n else np.zeros(1, np.int8))
        r = PfMpJobResult(n, decp.ctypes.data, to.ctypes.data,
                          PfQnameTagsC(len(off) - 1, off.ctypes.data, names.ctypes.data, hp.ctypes.data),
                          int(res.get("n_limit", 0)))
        _check(lib().pf_mp_set_job_result(self.h, kind, j, C.byref(r)), "pf_mp_set_job_result")

    def finish(self):
        _check(lib().pf_mp_finish(self.h), "pf_mp_finish")

    def decisions(self) -> np.ndarray:
        d, n, nl = C.c_void_p(), C.c_uint32(), C.c_uint32()
        _check(lib().pf_mp_decisions(self.h, C.byref(d), C.byref(n), C.byref(nl)), "pf_mp_decisions")
        self.n_limit = int(nl.value)
        return _arr(d, n.value, np.int8)

    def qname_hp(self) -> Dict[str, int]:
        return tags_dict(lib().pf_mp_qname_hp(self.h))

    def raw_hp(self) -> Dict[str, int]:
        return tags_dict(lib().pf_mp_raw_hp(self.h))

    def contigs(self):
        return _blocks_contigs(lib().pf_mp_blocks(self.h))

    def gaps(self):
        return _gaps_contigs(lib().pf_mp_gaps(self.h))

    def report_counts(self):
        c = (C.c_double * 3)()
        _check(lib().pf_mp_report_counts(self.h, c), "pf_mp_report_counts")
        return dict(correct=int(c[0]), switch=int(c[1]), fail=int(c[2]))

    def masked_sites(self) -> int:
        """Qualifying positions the mask removed, over the window jobs this
        process ran (pf_mp_masked_sites); 0 with no mask."""
        t = C.c_uint64()
        _check(lib().pf_mp_masked_sites(self.h, C.byref(t)), "pf_mp_masked_sites")
        return int(t.value)

    def stats(self) -> Dict:
        """Wall seconds per phase and the device-fetch sums of the run
        (pf_mp_stats; a measurement hook)."""
        st = PfMpStats()
        _check(lib().pf_mp_stats(self.h, C.byref(st)), "pf_mp_stats")
        names = ("read", "inflate", "chain", "decode", "select", "build", "total")
        out = {k: round(getattr(st, k), 4) for k in ("s_plan", "s_estimate", "s_haptag", "s_windows", "s_finish")}
        out.update({k: int(getattr(st, k)) for k in ("arena_hits", "arena_misses", "reread_bytes", "steals")})
        for i, kind in enumerate(("windows", "haptag")):
            out[kind] = dict({f"{n}_ms": round(st.fetch_ms[i][j], 2) for j, n in enumerate(names)},
                             comp_bytes=int(st.comp_bytes[i]), inflated_bytes=int(st.inflated_bytes[i]),
                             run_ms=round(st.run_ms[i], 2), n_fetch=int(st.n_fetch[i]))
        return out

    def close(self):
        if self.h:
            lib().pf_mp_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _result(plan: Plan, mode: int) -> Dict:
    dec = plan.decisions()
    if mode == MODE_REPORT:
        return dict(decision=dec, counts=plan.report_counts(), n_limit=plan.n_limit,
                    masked_sites=plan.masked_sites())
    return dict(decision=dec, contigs=plan.contigs(), qname_hp=plan.qname_hp(), raw_hp=plan.raw_hp(),
                n_limit=plan.n_limit, stats=plan.stats(), masked_sites=plan.masked_sites())


def load_mask(names: List[str], bed_path: Optional[str] = None, vcf_path: Optional[str] = None) -> List[np.ndarray]:
    """Masked reference positions per contig of `names` (pf_mask_load): the
    sorted unique union of the BED's intervals (chrom, start, end; 0-based
    half-open; plain or gzipped) and of [pos, pos+len) of every phased variant
    of the VCF.  Returns one uint32 array per contig, as DeviceBatch.set_mask
    takes them."""
    L = _bind()
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    h = C.c_void_p()
    _check(L.pf_mask_load(bed_path.encode() if bed_path else None, vcf_path.encode() if vcf_path else None,
                          len(names), arr, C.byref(h)), "pf_mask_load")
    try:
        out = []
        for c in range(len(names)):
            p, n = C.c_void_p(), C.c_uint64()
            _check(L.pf_mask_contig(h, c, C.byref(p), C.byref(n)), "pf_mask_contig")
            out.append(_arr(p, n.value, np.uint32))
        return out
    finally:
        L.pf_mask_free(h)


def methphase_files(bam_path: str, vcf_path: str, out_prefix: Optional[str], cfg: Optional[Config],
                    lcfg: Optional[LoadConfig] = None, device: int = 0, threads: int = 8, ctx=None,
                    untagged: bool = False, tsv: bool = False, n_devices: int = 1, job_windows: int = 0,
                    host_fetch: bool = False, ctxs=None, intervals=None,
                    write_input_tagging: bool = False, mask_bed: Optional[str] = None,
                    mask_variants: bool = False, ref: Optional[str] = None) -> Dict:
    """`pomfret methphase` over every gap of vcf_path with the reads of
    bam_path, in this process (pf_methphase_main).  Writes out_prefix +
    .mp.gtf / .mp.vcf (and .mp.tsv with tsv=True, the reference's
    --output-tsv) unless out_prefix is None.  cfg None: no -c, per-contig
    parameters from the coverage estimate (4358-4390).  ctx: drive that
    context; ctxs: drive those contexts, one host thread each, over one job
    queue (two contexts of one device exercise the multi-GPU dispatcher);
    else n_devices GPUs from `device` on (0: all visible).
    Returns dict(decision=int8[n_gaps], contigs=[...], qname_hp={qname: hp},
    raw_hp={qname: hp} (the -u table), n_limit).  intervals=(path,
    INTERVALS_GTF | INTERVALS_TSV): the --gtf / --tsv phase blocks instead of
    the VCF's (vcf_path None: no VCF written); write_input_tagging: -U.
    mask_bed / mask_variants: --mask-bed / --mask-variants; the result's
    masked_sites counts the sites they removed.  ref: --ref, the reference
    FASTA MD is synthesised from (a BAM without MD:Z tags)."""
    L = _bind()
    devs = None
    if ctx is not None:
        ctxs = [ctx]
    if not ctxs and device and n_devices >= 1:
        devs = (C.c_int32 * n_devices)(*range(device, device + n_devices))
    o = make_opts(bam_path, vcf_path, out_prefix, cfg, lcfg, untagged=untagged, tsv=tsv, threads=threads,
                  n_devices=0 if ctxs else n_devices, ctxs=ctxs or None,
                  job_windows=job_windows, host_fetch=host_fetch, intervals=intervals,
                  write_input_tagging=write_input_tagging, mask_bed=mask_bed, mask_variants=mask_variants, ref=ref)
    if devs is not None:
        o.devices = C.cast(devs, C.c_void_p)
    h = C.c_void_p()
    _check(L.pf_methphase_main(C.byref(o), C.byref(h)), "pf_methphase_main")
    plan = Plan(o, handle=h)
    try:
        return _result(plan, MODE_METHPHASE)
    finally:
        plan.close()


def report_files(bam_path: str, vcf_path: str, out_prefix: Optional[str], cov: int = 0,
                 chunk_size: int = 50_000, chunk_stride: int = 1_000_000, lcfg: Optional[LoadConfig] = None,
                 untagged: bool = False, threads: int = 8, ctx=None, n_devices: int = 1, k: int = 3,
                 k_span: int = 5000, host_fetch: bool = False, ctxs=None, mask_bed: Optional[str] = None,
                 mask_variants: bool = False, ref: Optional[str] = None) -> Dict:
    """`pomfret report` (main_methreport, 4901-5089): chunk windows inside the
    phased blocks, one methphase decision each; writes
    {out_prefix}.report.tsv and the running totals to stdout.  cov: -c
    (0: the per-contig estimate).  mask_bed / mask_variants: --mask-bed /
    --mask-variants.  ref: --ref (with untagged: MD synthesised from the
    FASTA).  Returns dict(decision, counts, n_limit, masked_sites)."""
    L = _bind()
    if ctx is not None:
        ctxs = [ctx]
    o = make_opts(bam_path, vcf_path, out_prefix, Config(k=k, k_span=k_span), lcfg, mode=MODE_REPORT,
                  untagged=untagged, threads=threads, n_devices=0 if ctxs else n_devices,
                  ctxs=ctxs or None, cov=cov, chunk_size=chunk_size, chunk_stride=chunk_stride,
                  host_fetch=host_fetch, mask_bed=mask_bed, mask_variants=mask_variants, ref=ref)
    h = C.c_void_p()
    _check(L.pf_methphase_main(C.byref(o), C.byref(h)), "pf_methphase_main")
    plan = Plan(o, handle=h)
    try:
        return _result(plan, MODE_REPORT)
    finally:
        plan.close()


def hapmeth_files(bam: str, out_prefix: str, region: Optional[str] = None, chunk_size: int = 100_000,
                  lcfg: Optional[LoadConfig] = None, host_fetch: bool = False, threads: int = 1, device: int = 0,
                  job_windows: int = 0, dmr: Optional[DmrConfig] = None, dmr_max_p: float = 1.0,
                  dmr_blocks: Optional[str] = None, dmr_perm: int = 0, dmr_seed: int = 1,
                  assign: Optional[AssignConfig] = None, tag_check=False,
                  dmr_hmm: Optional[HmmConfig] = None, regions: Optional[str] = None, dmr_rank: bool = False,
                  dmr_rank_min_calls: int = 3, rank_exact: bool = False, rank_exact_max: int = 64, tile: int = 0,
                  tile_min_calls: int = 3) -> Dict:
    """`pomfret-amd hapmeth` (pf_hapmeth_run_tiles): the per-haplotype CpG
    methylation of a haplotagged BAM, written to out_prefix + .hapmeth.bed
    (chrom, start, end, meth / unmeth calls of haplotype 1, haplotype 2 and
    the other reads, the two-sided Fisher p of haplotype 1 against 2).
    region: chrom or chrom:beg-end (1-based inclusive), None: every contig.
    chunk_size: bases per window, the fetch unit.  lcfg None: -q 10, -L 0,
    ML bands 100 / 156.  Returns dict(path, n_windows, n_skipped (windows the
    index holds no chunk for: not fetched), n_records, n_sites, ms_kernels).
    dmr: a DmrConfig also writes out_prefix + .hapmeth.dmr.bed, the regions
    where the haplotypes differ (`--dmr`; dmr_max_p drops regions whose
    pooled_p -- a ranking score, not a calibrated p-value -- is above it;
    dmr_blocks: a phase-block GTF no region crosses a block edge of), and adds
    dmr_path, n_regions, n_informative and dmr_ms_kernels to the dict.
    dmr_perm: permutations of the reads' haplotype labels per region
    (`--dmr-perm`, 1 .. 1,000,000; 0: off; needs dmr): the region file gains
    the columns reads_h1, reads_h2 and perm_p = (hits + 1) / (dmr_perm + 1), a
    p-value that holds under the correlation of one read's calls, and the dict
    n_tested (lines with a numeric perm_p), n_untested (lines with "."),
    perm_records (records the second pass fetched) and perm_ms_kernels;
    dmr_seed seeds the permutations.
    assign: an AssignConfig (`--assign`; needs dmr, whose min_cov is the one
    used) also writes out_prefix + .hapmeth.assign.tsv, one line per region
    and untagged read with a call at one of its member CpGs (qname, chrom,
    start, end, n_calls, llr in bits, hp 1 / 2 / "."), and adds assign_path,
    n_assign_lines, n_assigned (n_assigned_h1 + n_assigned_h2), assign_records
    and assign_ms_kernels to the dict.
    tag_check: True (`--tag-check`; needs dmr) also writes out_prefix +
    .hapmeth.tagcheck.tsv, one line per region and tagged read of it with a
    usable call, scored leave-one-out under assign's thresholds (AssignConfig's
    defaults when assign is None; an AssignConfig in place of True names the
    rule without turning assign on): qname, chrom, start, end, hp, n_calls, llr,
    verdict ok / flip / "."; and out_prefix + .hapmeth.tagcheck.regions.tsv, one
    line per region with the reads, scored, ok and flip counts of each
    haplotype.  Adds tagcheck_path, tagcheck_regions_path, n_tagcheck_lines,
    n_tagcheck_regions, tagcheck_ok / _flip / _undecided (each [h1, h2]),
    tagcheck_concordance (ok / (ok + flip), None when both are 0),
    tagcheck_records and tagcheck_ms_kernels to the dict.
    dmr_hmm: an HmmConfig (`--dmr-hmm`; needs dmr) finds the regions with the
    hidden Markov model of pf_dmr_hmm_regions, one call per contig, instead of
    the per-CpG threshold; dmr.min_delta_pct then applies to a region's pooled
    difference.  The region file keeps its name and columns and everything
    after it works on these regions.  Adds n_chains and hmm_ms_kernels to the
    dict (dmr_ms_kernels counts the model's kernels too).
    regions: a BED path (`--regions`) makes the caller's regions the source
    instead: out_prefix + .hapmeth.regions.bed gets one line per region of the
    BED (pf_write_regions has the columns), no .hapmeth.dmr.bed is written, and
    dmr (DmrConfig's defaults when None) gives min_cov, min_delta_pct and
    min_sites; max_gap is not used and dmr_hmm is refused.  dmr_perm, assign
    and tag_check work on the eligible regions (not split by a dmr_blocks
    block, min_sites informative CpGs, pooled_p <= dmr_max_p, at most
    1,000,000 bases); dmr_perm adds reads_h1, reads_h2, perm_p and perm_q, the
    Benjamini-Hochberg q-value over the run's tested regions.  Adds
    regions_path, n_regions, n_regions_unknown_contig, n_regions_outside (not
    wholly inside `region`), n_regions_split, n_tested, n_untested and
    regions_ms_kernels to the dict, in place of the dmr entries.
    dmr_rank: True (`--dmr-rank`; needs dmr or regions) also writes out_prefix +
    .hapmeth.rank.tsv, one line per region of the second pass (the ones
    dmr_perm tests) with the read-level Mann-Whitney rank-sum test between the
    haplotypes (pf_write_rank has the columns): every read counts once, with
    its own methylation fraction inside the region, if it has at least
    dmr_rank_min_calls calls there (1 .. 65535; a choice, not a measured
    optimum).  rank_p is the asymptotic two-sided p-value (approximate below
    about eight reads per haplotype), rank_q its Benjamini-Hochberg q-value
    with regions, "." with found regions.  Adds rank_path, rank_tested,
    rank_untested, rank_records and rank_ms_kernels to the dict.
    rank_exact: True (`--dmr-rank-exact`; needs dmr_rank) adds exact_p, best_p
    and best_q to the rank file (pf_write_rank_exact): the exact two-sided
    p-value of the same test for regions of at most rank_exact_max (2 .. 64)
    counted reads, exact_p where there is one and rank_p elsewhere, and its
    q-value with regions.  The file's first 17 columns and every other file
    stay the same bytes.  Adds rank_exact (lines with an exact_p),
    rank_exact_over (regions over rank_exact_max) and rank_exact_ms_kernels.
    tile: a tile width in bases (`--tile`; 0: off) also writes out_prefix +
    .hapmeth.tiles.tsv, the genome-wide scan (pf_hapmeth_run_tiles,
    pf_write_rank_tiles): every tile of each contig, or of `region` counted
    from its start, that holds a tagged read's call, under dmr_rank's test in
    the first pass, with the counted reads' calls, delta, block (split by a
    dmr_blocks phase block: counted, not tested) and rank_q over the run's
    tested tiles.  tile is 100 .. chunk_size and chunk_size a multiple of it;
    a read counts with at least tile_min_calls calls in the tile.  Needs no
    dmr, goes with every other option and changes no other file.  Adds
    tiles_path, n_tiles (planned), tiles_written, tiles_tested, tiles_split and
    tiles_ms_kernels to the dict."""
    L = _bind()
    if tile:
        cs = int(chunk_size) if chunk_size else 100_000
        if not 100 <= int(tile) <= cs or cs % int(tile):
            raise PomfretError("hapmeth_files: tile is 100 .. chunk_size, and chunk_size must be a multiple of tile")
        if not 1 <= int(tile_min_calls) <= 65535:
            raise PomfretError("hapmeth_files: tile_min_calls is 1 .. 65535")
    if regions is not None:
        if dmr_hmm is not None:
            raise PomfretError("hapmeth_files: regions gives the regions: it excludes dmr_hmm")
        if dmr is None:
            dmr = DmrConfig()
    if dmr_perm and dmr is None:
        raise PomfretError("hapmeth_files: dmr_perm needs dmr")
    if assign is not None and dmr is None:
        raise PomfretError("hapmeth_files: assign needs dmr")
    if tag_check and dmr is None:
        raise PomfretError("hapmeth_files: tag_check needs dmr")
    if dmr_hmm is not None and dmr is None:
        raise PomfretError("hapmeth_files: dmr_hmm needs dmr")
    if isinstance(tag_check, AssignConfig) and assign is not None:
        raise PomfretError("hapmeth_files: with assign, tag_check checks assign's rule: pass True")
    if dmr_rank and dmr is None:
        raise PomfretError("hapmeth_files: dmr_rank needs dmr or regions")
    if rank_exact and not dmr_rank:
        raise PomfretError("hapmeth_files: rank_exact needs dmr_rank")
    if rank_exact and not 2 <= int(rank_exact_max) <= 64:
        raise PomfretError("hapmeth_files: rank_exact_max is 2 .. 64")
    if dmr_rank and not 1 <= int(dmr_rank_min_calls) <= 65535:
        raise PomfretError("hapmeth_files: dmr_rank_min_calls is 1 .. 65535")
    lc = lcfg or LoadConfig(min_len=0)
    o = PfHapmethOpts(bam.encode(), out_prefix.encode(), region.encode() if region else None, int(chunk_size),
                      int(job_windows), lc.to_c(), int(threads), int(bool(host_fetch)), int(device), 0)
    st = PfHapmethStats()
    # every combination is one call: the earlier entry points are this one with NULLs
    d = PfHapmethDmr(dmr.to_c(), float(dmr_max_p), dmr_blocks.encode() if dmr_blocks else None) if dmr is not None else None
    pm = PfHapmethPerm(int(dmr_perm), int(dmr_seed))
    rule = assign if assign is not None else tag_check if isinstance(tag_check, AssignConfig) else AssignConfig()
    am = PfHapmethAssign(rule.min_llr_q16, int(rule.min_calls), 0)
    tm = PfHapmethTagcheck(0 if assign is not None else HAPMETH_TAGCHECK_RULE_ONLY, 0)
    rg = PfHapmethRegions(regions.encode()) if regions is not None else None
    hm = PfHapmethHmm(dmr_hmm.to_c()) if dmr_hmm is not None else None
    km, xm = PfHapmethRank(int(dmr_rank_min_calls)), PfHapmethRankExact(int(rank_exact_max))
    lm = PfHapmethTiles(int(tile), int(tile_min_calls), dmr_blocks.encode() if dmr_blocks else None)
    dst, pst, hst, ast = PfHapmethDmrStats(), PfHapmethPermStats(), PfHapmethHmmStats(), PfHapmethAssignStats()
    tst, rst, kst, xst = PfHapmethTagcheckStats(), PfHapmethRegionsStats(), PfHapmethRankStats(), PfHapmethRankExactStats()
    lst = PfHapmethTilesStats()

    def ref(x, on=True):
        return C.byref(x) if on and x is not None else None
    _check(L.pf_hapmeth_run_tiles(C.byref(o), ref(d), ref(hm), ref(pm, dmr_perm), ref(am, assign is not None or tag_check),
                                  ref(tm, tag_check), ref(rg), ref(km, dmr_rank), ref(xm, rank_exact), ref(lm, tile),
                                  C.byref(st), C.byref(dst), C.byref(hst), C.byref(pst), C.byref(ast), C.byref(tst),
                                  C.byref(rst), C.byref(kst), C.byref(xst), C.byref(lst)), "pf_hapmeth_run_tiles")
    res = dict(path=out_prefix + ".hapmeth.bed", n_windows=int(st.n_windows), n_skipped=int(st.n_skipped),
               n_records=int(st.n_records), n_sites=int(st.n_sites), ms_kernels=float(st.ms_kernels))
    if tile:
        res.update(tiles_path=out_prefix + ".hapmeth.tiles.tsv", n_tiles=int(lst.n_tiles), tiles_written=int(lst.n_written),
                   tiles_tested=int(lst.n_tested), tiles_split=int(lst.n_split), tiles_ms_kernels=float(lst.ms_kernels))
    if dmr is not None:
        if regions is not None:
            res.update(regions_path=out_prefix + ".hapmeth.regions.bed", n_regions=int(rst.n_regions),
                       n_regions_unknown_contig=int(rst.n_unknown_contig), n_regions_outside=int(rst.n_outside),
                       n_regions_split=int(rst.n_split), n_tested=int(rst.n_tested), n_untested=int(rst.n_untested),
                       regions_ms_kernels=float(rst.ms_kernels))
        else:
            res.update(dmr_path=out_prefix + ".hapmeth.dmr.bed", n_regions=int(dst.n_regions),
                       n_informative=int(dst.n_informative), dmr_ms_kernels=float(dst.ms_kernels))
        if dmr_hmm is not None:
            res.update(n_chains=int(hst.n_chains), hmm_ms_kernels=float(hst.ms_kernels))
        if dmr_perm:
            res.update(n_tested=int(pst.n_tested), n_untested=int(pst.n_untested), perm_records=int(pst.n_records),
                       perm_ms_kernels=float(pst.ms_kernels))
        if dmr_rank:
            res.update(rank_path=out_prefix + ".hapmeth.rank.tsv", rank_tested=int(kst.n_tested),
                       rank_untested=int(kst.n_untested), rank_records=int(kst.n_records),
                       rank_ms_kernels=float(kst.ms_kernels))
        if rank_exact:
            res.update(rank_exact=int(xst.n_exact), rank_exact_over=int(xst.n_over),
                       rank_exact_ms_kernels=float(xst.ms_kernels))
        if assign is not None:
            res.update(assign_path=out_prefix + ".hapmeth.assign.tsv", n_assign_lines=int(ast.n_lines),
                       n_assigned=int(ast.n_h1 + ast.n_h2), n_assigned_h1=int(ast.n_h1), n_assigned_h2=int(ast.n_h2),
                       assign_records=int(ast.n_records),
                       assign_ms_kernels=float(ast.ms_kernels))
        if tag_check:
            ok, flip = [int(x) for x in tst.n_ok], [int(x) for x in tst.n_flip]
            res.update(tagcheck_path=out_prefix + ".hapmeth.tagcheck.tsv",
                       tagcheck_regions_path=out_prefix + ".hapmeth.tagcheck.regions.tsv",
                       n_tagcheck_lines=int(tst.n_lines), n_tagcheck_regions=int(tst.n_regions), tagcheck_ok=ok,
                       tagcheck_flip=flip, tagcheck_undecided=[int(x) for x in tst.n_undecided],
                       tagcheck_concordance=sum(ok) / (sum(ok) + sum(flip)) if sum(ok) + sum(flip) else None,
                       tagcheck_records=int(tst.n_records), tagcheck_ms_kernels=float(tst.ms_kernels))
    return res


def dmr_stitch(parts, cfg: Optional[DmrConfig] = None, breaks=None) -> Dict:
    """The regions of one contig from the Context.dmr_regions results of its
    consecutive ranges, in ascending order (pf_dmr_acc_*, host only): the same
    whatever the cut.  Returns the dict of Context.dmr_regions (open all 0,
    every run at least cfg.min_sites long)."""
    L = _bind()
    c = (cfg or DmrConfig()).to_c()
    b, bp, nb = _breaks(breaks)
    acc = L.pf_dmr_acc_new(C.byref(c), bp, nb)
    if not acc:
        raise PomfretError("pf_dmr_acc_new: bad arguments (breaks must be sorted)")
    try:
        for part in parts:
            d, keep = _dmr_to_c(part)
            _check(L.pf_dmr_acc_add(acc, C.byref(d)), "pf_dmr_acc_add")
        fin = C.POINTER(PfDmr)()
        _check(L.pf_dmr_acc_flush(acc, C.byref(fin)), "pf_dmr_acc_flush")
        try:
            return _dmr_dict(fin.contents)
        finally:
            L.pf_dmr_free(fin)
    finally:
        L.pf_dmr_acc_free(acc)


def write_dmr(path: str, chrom: str, dmr: Dict, max_p: float = 1.0, header: bool = True):
    """Regions (dmr_stitch's dict) as hapmeth --dmr BED lines (pf_write_dmr,
    host only): chrom, start, end, n_sites, dir, the pooled counts, delta and
    pooled_p (a ranking score, not a calibrated p-value); regions with
    pooled_p > max_p are dropped.  header: create the file with the column
    names first; else append."""
    L = _bind()
    d, keep = _dmr_to_c(dmr)
    _check(L.pf_write_dmr(path.encode(), chrom.encode(), C.byref(d), float(max_p), int(bool(header))), "pf_write_dmr")


def write_dmr_perm(path: str, chrom: str, dmr: Dict, perm: Dict, max_p: float = 1.0, header: bool = True):
    """write_dmr's lines followed by reads_h1, reads_h2 and perm_p
    (pf_write_dmr_perm, host only).  perm: DeviceBatch.permtest's dict of a
    batch whose window k is region k of dmr (n_reads, hits, status, n_perm);
    perm_p = (hits + 1) / (n_perm + 1), "." where status is not 0."""
    L = _bind()
    d, keep = _dmr_to_c(dmr)
    if perm is None:
        _check(L.pf_write_dmr_perm(path.encode(), chrom.encode(), C.byref(d), None, float(max_p), int(bool(header))),
               "pf_write_dmr_perm")
        return
    W = int(np.size(perm["hits"]))
    nr = np.zeros(2 * W + 1, np.uint32)
    hits, stat, sm = np.zeros(W + 1, np.uint32), np.zeros(W + 1, np.uint32), np.zeros(4 * W + 1, np.uint64)
    nr[:2 * W] = np.asarray(perm["n_reads"], np.uint32).ravel()
    hits[:W] = np.asarray(perm["hits"], np.uint32).ravel()
    stat[:W] = np.asarray(perm["status"], np.uint32).ravel()
    if "sum" in perm:
        sm[:4 * W] = np.asarray(perm["sum"], np.uint64).ravel()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    p = PfPerm(W, int(perm["n_perm"]), int(perm.get("seed", 0)), nr.ctypes.data_as(u32p), sm.ctypes.data_as(u64p),
               hits.ctypes.data_as(u32p), stat.ctypes.data_as(u32p), 0.0)
    _check(L.pf_write_dmr_perm(path.encode(), chrom.encode(), C.byref(d), C.byref(p), float(max_p), int(bool(header))),
           "pf_write_dmr_perm")


def regions_load(bed: str, names) -> Dict:
    """The regions of a `--regions` BED for the contigs `names`
    (pf_regions_load, host only; include/pomfret_amd.h has the format):
    dict(contigs=[dict(start, end, name) per contig of names, each stably
    sorted by (start, end)], n_unknown_contig)."""
    L = _bind()
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    h = C.c_void_p()
    _check(L.pf_regions_load(bed.encode(), len(names), arr, C.byref(h)), "pf_regions_load")
    try:
        out = []
        for c in range(len(names)):
            s, e = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
            nm, n = C.POINTER(C.c_char_p)(), C.c_uint64()
            _check(L.pf_regions_contig(h, c, C.byref(s), C.byref(e), C.byref(nm), C.byref(n)), "pf_regions_contig")
            k = int(n.value)
            out.append(dict(start=[int(s[i]) for i in range(k)], end=[int(e[i]) for i in range(k)],
                            name=[nm[i].decode() for i in range(k)]))
        return dict(contigs=out, n_unknown_contig=int(L.pf_regions_unknown(h)))
    finally:
        L.pf_region_list_free(h)


def bh_adjust(hits, tested, n_perm: int) -> np.ndarray:
    """Benjamini-Hochberg q-values of the tested entries from the permutation
    test's hits (pf_bh_adjust, host only): p = (hits + 1) / (n_perm + 1); NaN
    for an untested entry."""
    L = _bind()
    h = np.ascontiguousarray(hits, np.uint32).ravel()
    t = np.ascontiguousarray(tested, np.uint8).ravel()
    if h.size != t.size:
        raise PomfretError("bh_adjust: hits and tested differ in length")
    q = np.zeros(max(h.size, 1), np.float64)
    _check(L.pf_bh_adjust(h.ctypes.data, t.ctypes.data, h.size, int(n_perm), q.ctypes.data), "pf_bh_adjust")
    return q[:h.size]


def bh_adjust_p(p, tested) -> np.ndarray:
    """Benjamini-Hochberg q-values of the tested entries from p-values given as
    doubles (pf_bh_adjust_p, host only): bh_adjust's rule and order of
    operations; NaN for an untested entry."""
    L = _bind()
    pv = np.ascontiguousarray(p, np.float64).ravel()
    t = np.ascontiguousarray(tested, np.uint8).ravel()
    if pv.size != t.size:
        raise PomfretError("bh_adjust_p: p and tested differ in length")
    pv = np.concatenate([pv, np.zeros(1)])                    # never an empty buffer
    t = np.concatenate([t, np.zeros(1, np.uint8)])
    q = np.zeros(pv.size, np.float64)
    _check(L.pf_bh_adjust_p(pv.ctypes.data, t.ctypes.data, pv.size - 1, q.ctypes.data), "pf_bh_adjust_p")
    return q[:-1]


def write_rank(path: str, recs, bh: bool = False) -> int:
    """{prefix}.hapmeth.rank.tsv from records (pf_write_rank, host only).  recs:
    dicts of chrom, start, end, n_reads [2], n_short [2], cls [6] (or [2][3]),
    u2, ties and status -- a window of DeviceBatch.ranktest and its region.
    bh: rank_q by Benjamini-Hochberg over the status-0 records, else ".".
    Returns the records with a numeric rank_p."""
    L = _bind()
    arr = (PfRankRec * max(len(recs), 1))()
    for k, r in enumerate(recs):
        x = arr[k]
        x.chrom, x.start, x.end = r["chrom"].encode(), int(r["start"]), int(r["end"])
        for j in range(2):
            x.reads[j], x.n_short[j] = int(r["n_reads"][j]), int(r["n_short"][j])
        for j, v in enumerate(np.asarray(r["cls"]).ravel().tolist()):
            x.cls[j] = int(v)
        x.status, x.u2, x.ties = int(r["status"]), int(r["u2"]), int(r["ties"])
    n = C.c_uint64()
    _check(L.pf_write_rank(path.encode(), arr, len(recs), int(bool(bh)), C.byref(n)), "pf_write_rank")
    return int(n.value)


def write_rank_tiles(path: str, recs) -> int:
    """{prefix}.hapmeth.tiles.tsv from records (pf_write_rank_tiles, host only).
    recs: write_rank's dicts with sum [4] (the counted reads' m1, u1, m2, u2)
    and optionally split (bool) beside them -- a range of
    DeviceBatch.rankranges and its tile.  rank_q by Benjamini-Hochberg over the
    status-0 records that are not split.  Returns the records with a numeric
    rank_p."""
    L = _bind()
    arr = (PfRankRec * max(len(recs), 1))()
    tarr = (PfRankTileRec * max(len(recs), 1))()
    for k, r in enumerate(recs):
        x = arr[k]
        x.chrom, x.start, x.end = r["chrom"].encode(), int(r["start"]), int(r["end"])
        for j in range(2):
            x.reads[j], x.n_short[j] = int(r["n_reads"][j]), int(r["n_short"][j])
        for j, v in enumerate(np.asarray(r["cls"]).ravel().tolist()):
            x.cls[j] = int(v)
        x.status, x.u2, x.ties = int(r["status"]), int(r["u2"]), int(r["ties"])
        for j in range(4):
            tarr[k].sum[j] = int(r["sum"][j])
        tarr[k].split = int(bool(r.get("split", False)))
    n = C.c_uint64()
    _check(L.pf_write_rank_tiles(path.encode(), arr, tarr, len(recs), C.byref(n)), "pf_write_rank_tiles")
    return int(n.value)


def write_rank_exact(path: str, recs, bh: bool = False):
    """The rank file with exact_p, best_p and best_q (pf_write_rank_exact, host
    only).  recs: write_rank's dicts with the exact test's two, total and
    exact_status beside them -- a window of DeviceBatch.rankexact.  Returns
    (the records with a numeric rank_p, those with a numeric exact_p)."""
    L = _bind()
    arr = (PfRankRec * max(len(recs), 1))()
    xarr = (PfRankExactRec * max(len(recs), 1))()
    for k, r in enumerate(recs):
        x = arr[k]
        x.chrom, x.start, x.end = r["chrom"].encode(), int(r["start"]), int(r["end"])
        for j in range(2):
            x.reads[j], x.n_short[j] = int(r["n_reads"][j]), int(r["n_short"][j])
        for j, v in enumerate(np.asarray(r["cls"]).ravel().tolist()):
            x.cls[j] = int(v)
        x.status, x.u2, x.ties = int(r["status"]), int(r["u2"]), int(r["ties"])
        xarr[k].two, xarr[k].total, xarr[k].status = int(r["two"]), int(r["total"]), int(r["exact_status"])
    n, nx = C.c_uint64(), C.c_uint64()
    _check(L.pf_write_rank_exact(path.encode(), arr, xarr, len(recs), int(bool(bh)), C.byref(n), C.byref(nx)),
           "pf_write_rank_exact")
    return int(n.value), int(nx.value)


def write_regions(path: str, recs, perm: bool = False, n_perm: int = 0) -> int:
    """{prefix}.hapmeth.regions.bed from records (pf_write_regions, host only).
    recs: dicts of chrom, start, end, name, n_cpg, n_sites, n_pos, n_neg, sum
    [4], evidence, and optionally split (bool) and test = (reads_h1, reads_h2,
    hits, status) for a region the second pass took.  perm: the four
    permutation columns as well.  Returns the records with a numeric perm_p."""
    L = _bind()
    arr = (PfRegionRec * max(len(recs), 1))()
    for k, r in enumerate(recs):
        x = arr[k]
        x.chrom, x.name, x.start, x.end = r["chrom"].encode(), r["name"].encode(), int(r["start"]), int(r["end"])
        x.s.n_cpg, x.s.n_sites, x.s.n_pos, x.s.n_neg = int(r["n_cpg"]), int(r["n_sites"]), int(r["n_pos"]), int(r["n_neg"])
        for j in range(4):
            x.s.sum[j] = int(r["sum"][j])
        x.s.evidence = int(r["evidence"])
        x.flags = (REGION_SPLIT if r.get("split") else 0) | (REGION_ELIGIBLE if r.get("test") is not None else 0)
        if r.get("test") is not None:
            x.reads[0], x.reads[1], x.hits, x.status = (int(v) for v in r["test"])
    n = C.c_uint64()
    _check(L.pf_write_regions(path.encode(), arr, len(recs), int(bool(perm)), int(n_perm), C.byref(n)), "pf_write_regions")
    return int(n.value)


def write_assign(path: str, chrom: str, res: Optional[Dict], win_start, win_end, qnames, rec_of_read=None,
                 header: bool = True) -> int:
    """The scored reads of a DeviceBatch.assign dict as hapmeth --assign lines
    (pf_write_assign, host only): qname, chrom, the window's start and end,
    n_calls, llr = S / 65536 as %.4f and hp 1 / 2 / "."; one line per window
    and read of it with n_used >= 1.  qnames: the records' names (str or
    bytes); rec_of_read: each read's record, None for the identity.  res None
    (with header): the header alone.  Returns the lines written."""
    L = _bind()
    n = C.c_uint64(0)
    if res is None:
        _check(L.pf_write_assign(path.encode(), chrom.encode(), None, None, None, None, None, None, int(bool(header)),
                                 C.byref(n)), "pf_write_assign")
        return 0
    names = [q if isinstance(q, bytes) else str(q).encode() for q in qnames]
    qoff = np.zeros(len(names) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in names])
    blob = b"".join(names) + b"\0"
    wro = np.ascontiguousarray(np.append(np.asarray(res["win_read_off"], np.uint32), 0).astype(np.uint32))
    W, R = wro.size - 2, int(np.size(res["hp"]))
    pad = lambda a, dt: np.ascontiguousarray(np.append(np.asarray(a, dt).ravel(), 0).astype(dt))
    nu, llr, hp = pad(res["n_used"], np.uint32), pad(res["llr"], np.int64), pad(res["hp"], np.uint8)
    wn = pad(res.get("win_n", np.zeros(3 * W)), np.uint32)
    ws, we = pad(win_start, np.uint32), pad(win_end, np.uint32)
    if ws.size - 1 != W or we.size - 1 != W or nu.size - 1 != R or llr.size - 1 != R:
        raise PomfretError("inconsistent assign arrays")
    rr = None if rec_of_read is None else pad(rec_of_read, np.uint32)
    recs = np.arange(R) if rr is None else rr[:R]
    if R and int(np.max(recs)) >= len(names):
        raise PomfretError("write_assign: a read's record has no qname")
    u32p = C.POINTER(C.c_uint32)
    a = PfAssign(W, R, wro.ctypes.data_as(u32p), nu.ctypes.data_as(u32p), llr.ctypes.data_as(C.POINTER(C.c_int64)),
                 hp.ctypes.data_as(C.POINTER(C.c_uint8)), wn.ctypes.data_as(u32p), 0.0)
    _check(L.pf_write_assign(path.encode(), chrom.encode(), C.byref(a), ws.ctypes.data, we.ctypes.data,
                             None if rr is None else rr.ctypes.data, qoff.ctypes.data, blob, int(bool(header)), C.byref(n)),
           "pf_write_assign")
    return int(n.value)


def write_tagcheck(path: str, regions_path: Optional[str], chrom: str, res: Optional[Dict], win_start, win_end, qnames,
                   rec_of_read=None, header: bool = True):
    """The scored reads of a DeviceBatch.tagcheck dict as hapmeth --tag-check
    lines (pf_write_tagcheck, host only): qname, chrom, the window's start and
    end, hp 1 / 2, n_calls, llr = S / 65536 as %.4f and the verdict ok / flip /
    "."; one line per window and tagged read of it with n_used >= 1; and, with
    regions_path, the windows' counters (pf_write_tagcheck_regions), one line
    per window.  qnames, rec_of_read, res None as in write_assign.  Returns
    (read lines, region lines) written."""
    L = _bind()
    n, nr = C.c_uint64(0), C.c_uint64(0)
    if res is None:
        _check(L.pf_write_tagcheck(path.encode(), chrom.encode(), None, None, None, None, None, None, int(bool(header)),
                                   C.byref(n)), "pf_write_tagcheck")
        if regions_path:
            _check(L.pf_write_tagcheck_regions(regions_path.encode(), chrom.encode(), None, None, None, int(bool(header)),
                                               C.byref(nr)), "pf_write_tagcheck_regions")
        return 0, 0
    names = [q if isinstance(q, bytes) else str(q).encode() for q in qnames]
    qoff = np.zeros(len(names) + 1, np.uint64)
    qoff[1:] = np.cumsum([len(q) for q in names])
    blob = b"".join(names) + b"\0"
    wro = np.ascontiguousarray(np.append(np.asarray(res["win_read_off"], np.uint32), 0).astype(np.uint32))
    W, R = wro.size - 2, int(np.size(res["verdict"]))
    pad = lambda a, dt: np.ascontiguousarray(np.append(np.asarray(a, dt).ravel(), 0).astype(dt))
    nu, llr = pad(res["n_used"], np.uint32), pad(res["llr"], np.int64)
    vd, hp = pad(res["verdict"], np.uint8), pad(res["hp"], np.uint8)
    wn = pad(res["win_n"], np.uint32)
    ws, we = pad(win_start, np.uint32), pad(win_end, np.uint32)
    if (ws.size - 1 != W or we.size - 1 != W or nu.size - 1 != R or llr.size - 1 != R or hp.size - 1 != R
            or wn.size - 1 != 8 * W):
        raise PomfretError("inconsistent tagcheck arrays")
    rr = None if rec_of_read is None else pad(rec_of_read, np.uint32)
    recs = np.arange(R) if rr is None else rr[:R]
    if R and int(np.max(recs)) >= len(names):
        raise PomfretError("write_tagcheck: a read's record has no qname")
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    t = PfTagcheck(W, R, wro.ctypes.data_as(u32p), nu.ctypes.data_as(u32p), llr.ctypes.data_as(C.POINTER(C.c_int64)),
                   vd.ctypes.data_as(u8p), hp.ctypes.data_as(u8p), wn.ctypes.data_as(u32p), 0.0)
    _check(L.pf_write_tagcheck(path.encode(), chrom.encode(), C.byref(t), ws.ctypes.data, we.ctypes.data,
                               None if rr is None else rr.ctypes.data, qoff.ctypes.data, blob, int(bool(header)), C.byref(n)),
           "pf_write_tagcheck")
    if regions_path:
        _check(L.pf_write_tagcheck_regions(regions_path.encode(), chrom.encode(), C.byref(t), ws.ctypes.data, we.ctypes.data,
                                           int(bool(header)), C.byref(nr)), "pf_write_tagcheck_regions")
    return int(n.value), int(nr.value)


def write_hapmeth(path: str, chrom: str, pile: Dict, header: bool = True, w0: int = 0, w1: Optional[int] = None):
    """The sites of windows [w0, w1) of a pileup (DeviceBatch.pileup's dict:
    win_off, pos, cnt) as hapmeth BED lines (pf_write_hapmeth, host only).
    header: create the file with the column names first; else append."""
    L = _bind()
    win_off = np.ascontiguousarray(pile["win_off"], np.uint64)
    pos = np.ascontiguousarray(pile["pos"], np.uint32)
    cnt = np.ascontiguousarray(np.asarray(pile["cnt"], np.uint32).reshape(-1))
    if cnt.size != 6 * pos.size or win_off.size < 1 or int(win_off[-1]) != pos.size:
        raise PomfretError("pf_write_hapmeth: inconsistent pileup arrays")
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    p = PfPileup(win_off.size - 1, pos.size, win_off.ctypes.data_as(u64p), pos.ctypes.data_as(u32p),
                 cnt.ctypes.data_as(u32p), 0.0)
    _check(L.pf_write_hapmeth(path.encode(), chrom.encode(), C.byref(p), int(w0),
                              win_off.size - 1 if w1 is None else int(w1), int(bool(header))), "pf_write_hapmeth")


def methphase_files_dist(bam_path: str, vcf_path: str, out_prefix: Optional[str], cfg: Optional[Config],
                         lcfg: Optional[LoadConfig] = None, untagged: bool = False, tsv: bool = False,
                         threads: int = 8, ctx=None, group=None, job_windows: int = 0, mode: int = MODE_METHPHASE,
                         cov: int = 0, chunk_size: int = 50_000, chunk_stride: int = 1_000_000,
                         runner: Optional[Callable] = None, writer: int = 0, host_fetch: bool = False,
                         intervals=None, write_input_tagging: bool = False, mask_bed: Optional[str] = None,
                         mask_variants: bool = False) -> Dict:
    """One process per GPU (torch.distributed initialised; RCCL on GPUs,
    gloo on CPU).  Every rank plans the same jobs and runs the ones its
    static LPT shard owns on `ctx` (or its LOCAL_RANK device); -u tables are
    all-gathered so every rank loads with the merged table; window-job
    results are gathered to `writer`, which merges them in (contig, window)
    order, writes the outputs and broadcasts the decisions.
    `runner(plan, kind, j) -> result dict` replaces the device for a job
    (the CPU tests plug the oracle in here).  mask_bed / mask_variants:
    every rank loads the same mask; the result's masked_sites counts the
    writer's own jobs only."""
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    o = make_opts(bam_path, vcf_path, out_prefix if rank == writer else None, cfg, lcfg, mode=mode,
                  untagged=untagged, tsv=tsv, threads=threads, rank=rank, world=world, job_windows=job_windows,
                  cov=cov, chunk_size=chunk_size, chunk_stride=chunk_stride, host_fetch=host_fetch,
                  intervals=intervals, write_input_tagging=write_input_tagging, mask_bed=mask_bed,
                  mask_variants=mask_variants)
    plan = Plan(o)
    try:
        def run(kind):
            mine = [j for j in range(plan.n_jobs(kind)) if plan.job_info(kind, j)["rank"] == rank]
            if runner is not None:
                for j in mine:
                    plan.set_result(kind, j, runner(plan, kind, j))
            elif mine:
                if ctx is None:
                    import os
                    from ._lib import Context
                    run.ctx = getattr(run, "ctx", None) or Context(int(os.environ.get("LOCAL_RANK", "0")))
                    plan.run_mine(kind, ctxs=[run.ctx])
                else:
                    plan.run_mine(kind, ctxs=[ctx])
            return {j: plan.get_result(kind, j) for j in mine}

        if untagged:
            got = [None] * world
            dist.all_gather_object(got, run(JOB_HAPTAG), group=group)
            for r, part in enumerate(got):
                if r != rank:
                    for j, res in part.items():
                        plan.set_result(JOB_HAPTAG, j, res)
            plan.merge_raw()
        mine = run(JOB_WINDOWS)
        got = [None] * world if rank == writer else None
        dist.gather_object(mine, got, dst=writer, group=group)
        out = [None]
        if rank == writer:
            for r, part in enumerate(got):
                if r != rank:
                    for j, res in part.items():
                        plan.set_result(JOB_WINDOWS, j, res)
            plan.finish()
            out = [_result(plan, mode)]
        dist.broadcast_object_list(out, src=writer, group=group)
        return out[0]
    finally:
        if getattr(run, "ctx", None) is not None:
            run.ctx.close()
        plan.close()
