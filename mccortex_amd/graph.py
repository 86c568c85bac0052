"""ctypes mirror of include/mcx_gpu.h (one Python method per C entry point)."""
import ctypes as C
import os

import numpy as np

from . import _build

MCX_OK, MCX_ERR_ARG, MCX_ERR_NODEVICE, MCX_ERR_NOMEM, MCX_ERR_FULL, MCX_ERR_HIP, MCX_ERR_SINK, MCX_ERR_INVAL = 0, -1, -2, -3, -4, -5, -6, -7

_LIB = None

SYMBOLS = [
    "mcx_last_error", "mcx_version", "mcx_device_count", "mcx_device_memory", "mcx_graph_create", "mcx_graph_create_multi", "mcx_graph_ndevices",
    "mcx_graph_create_shard", "mcx_graph_shard_layout", "mcx_graph_shard_bins_dev", "mcx_graph_add_segments_dev",
    "mcx_graph_key_owner", "mcx_graph_insert_tuple_segments_dev", "mcx_graph_add_records", "mcx_graph_kmer_covg", "mcx_graph_covg_histogram", "mcx_sort_records",
    "mcx_records_sorted", "mcx_graph_intersect_finish", "mcx_superk_supported", "mcx_superk_record_bytes", "mcx_superk_owner", "mcx_graph_checksum", "mcx_records_checksum",
    "mcx_graph_superk_layout", "mcx_graph_superk_bins_dev", "mcx_graph_add_superk_dev", "mcx_graph_destroy",
    "mcx_graph_reset", "mcx_graph_configure", "mcx_graph_profile", "mcx_graph_capacity", "mcx_graph_add_reads", "mcx_graph_add_reads_pcr", "mcx_graph_pcr_reset", "mcx_graph_add_stream_dev",
    "mcx_graph_partition_stream_dev", "mcx_graph_insert_tuples_dev", "mcx_key_owner", "mcx_graph_sync",
    "mcx_graph_nkmers", "mcx_graph_device_stats", "mcx_graph_stream", "mcx_graph_export",
    "mcx_kmer_from_str", "mcx_kmer_canonical", "mcx_kmer_hash", "mcx_pack_bases", "mcx_pack_reads_host", "mcx_pack_stream_dev", "mcx_graph_add_packed_dev",
    "mcx_ubench_stream", "mcx_ubench_random_rmw", "mcx_graph_insert_stats", "mcx_multi_exchange_bytes", "mcx_graph_hashtest", "mcx_hashtest_func", "mcx_debug_probe",
    "mcx_graph_infer_edges", "mcx_graph_infer_edges_dev", "mcx_graph_unitig_stats", "mcx_graph_clean",
    "mcx_graph_unitigs", "mcx_graph_unitigs_dev", "mcx_graph_pop_bubbles",
    "mcx_graph_subgraph_begin", "mcx_graph_subgraph_seed_reads", "mcx_graph_subgraph_seed_stream_dev", "mcx_graph_subgraph_finish",
    "mcx_graph_reads_touch", "mcx_graph_reads_touch_stream_dev",
    "mcx_graph_coverage", "mcx_graph_coverage_stream_dev", "mcx_graph_coverage_text",
    "mcx_graph_correct", "mcx_graph_correct_stream_dev", "mcx_graph_correct_walk_steps",
    "mcx_graph_thread", "mcx_graph_links_info", "mcx_graph_links_contig_hist", "mcx_graph_links_text", "mcx_graph_links_reset",
    "mcx_graph_links_load_text", "mcx_graph_contigs", "mcx_graph_bubbles", "mcx_graph_breakpoints",
    "mcx_join_create", "mcx_join_configure", "mcx_join_get_stats", "mcx_join_phases", "mcx_join_buffer", "mcx_join_add_records", "mcx_join_finish", "mcx_join_destroy",
    "mcx_links_create", "mcx_links_configure", "mcx_links_buffer", "mcx_links_add_text", "mcx_links_get_stats", "mcx_links_hist", "mcx_links_error",
    "mcx_links_phases", "mcx_links_destroy",
    "mcx_pjoin_create", "mcx_pjoin_configure", "mcx_pjoin_buffer", "mcx_pjoin_add_text", "mcx_pjoin_finish", "mcx_pjoin_get_stats", "mcx_pjoin_error",
    "mcx_pjoin_phases", "mcx_pjoin_destroy",
]


class McxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mcx error %d: %s" % (code, msg))
        self.code = code


class LoadStats(C.Structure):
    """mcx_load_stats (subset of the reference's SeqLoadingStats)."""
    _fields_ = [(n, C.c_uint64) for n in (
        "num_se_reads", "num_good_reads", "num_bad_reads", "total_bases_read",
        "total_bases_loaded", "contigs_parsed", "num_kmers_loaded", "num_kmers_novel",
        "num_pe_reads", "num_dup_se_reads", "num_dup_pe_pairs")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RecordStats(C.Structure):
    """mcx_records_stats"""
    _fields_ = [("nkmers_read", C.c_uint64), ("nkmers_loaded", C.c_uint64), ("nkmers_novel", C.c_uint64),
                ("first_oversized", C.c_int64), ("first_zero_covg", C.c_int64), ("first_edges_no_covg", C.c_int64)]

    def __init__(self):
        super().__init__(0, 0, 0, -1, -1, -1)

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class CleanStats(C.Structure):
    """mcx_clean_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("num_tips", "num_tip_kmers", "num_low_covg_unitigs", "num_low_covg_unitig_kmers",
                                          "num_tip_and_low_unitigs", "num_tip_and_low_unitig_kmers", "nkmers_before",
                                          "nkmers_removed")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PopStats(C.Structure):
    """mcx_pop_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("num_popped", "num_pairs", "nkmers_before", "nkmers_removed", "num_unitigs_removed")] + \
               [("rounds", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SubgraphStats(C.Structure):
    """mcx_subgraph_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("num_seed_kmers", "num_seed_found", "nkmers_before", "nkmers_kept", "nkmers_removed")] + \
               [("levels", C.c_uint32), ("narrow_launches", C.c_uint32), ("max_frontier", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TouchStats(C.Structure):
    """mcx_touch_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("num_reads", "num_reads_hit", "num_kmers", "num_kmers_found")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class CoverageStats(C.Structure):
    """mcx_coverage_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("num_reads", "num_kmers", "num_kmers_found")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class CorrectParams(C.Structure):
    """mcx_correct_params"""
    _fields_ = [("colour", C.c_uint32), ("flags", C.c_uint32), ("gap_variance", C.c_float), ("gap_wiggle", C.c_float), ("fq_zero", C.c_char)]


class CorrectStats(C.Structure):
    """mcx_correct_stats"""
    _fields_ = [(n, C.c_uint64) for n in (
        "num_reads", "num_kmers", "num_kmers_found", "num_perfect", "num_no_kmers", "gaps", "gaps_filled", "gaps_filled_backward",
        "gaps_too_short", "gaps_too_long_or_stopped", "stops_fork", "stops_colour", "stops_repeat", "missing_edges", "end_gaps",
        "end_gaps_extended", "bases_filled")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ThreadParams(C.Structure):
    """mcx_thread_params"""
    _fields_ = [("flags", C.c_uint32), ("gap_variance", C.c_float), ("gap_wiggle", C.c_float), ("max_juncs", C.c_uint32)]


class ThreadStats(C.Structure):
    """mcx_thread_stats"""
    _fields_ = [("aln", CorrectStats)] + [(n, C.c_uint64) for n in ("contigs", "contig_kmers", "juncs_fw", "juncs_rv", "links_added")]

    def as_dict(self):
        d = self.aln.as_dict()
        d.update({n: int(getattr(self, n)) for n, _ in self._fields_[1:]})
        return d


class LinksInfo(C.Structure):
    """mcx_links_info"""
    _fields_ = [(n, C.c_uint64) for n in ("num_kmers_with_paths", "num_paths", "path_bytes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ContigsParams(C.Structure):
    """mcx_contigs_params"""
    _fields_ = [("colour", C.c_uint32), ("flags", C.c_uint32), ("ncontigs", C.c_uint64), ("min_step_confid", C.c_double),
                ("min_cumul_confid", C.c_double), ("conf", C.c_void_p), ("nconf", C.c_uint64)]


class ContigsStats(C.Structure):
    """mcx_contigs_stats"""
    _fields_ = [("contigs", C.c_uint64), ("num_reseed_abort", C.c_uint64), ("seeds_not_found", C.c_uint64), ("stop_causes", C.c_uint64 * 9),
                ("wlk_steps", C.c_uint64 * 9), ("total_nodes", C.c_uint64), ("total_junc", C.c_uint64), ("corrupt_links", C.c_uint64),
                ("reruns", C.c_uint64)]

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n in ("stop_causes", "wlk_steps") else int(getattr(self, n))) for n, _ in self._fields_}


# mcx_contig_rec
CONTIG_REC = np.dtype([("seed_key", "<u8", 4), ("len_nodes", "<u8"), ("seq_off", "<u8"), ("num_junc", "<u4"), ("paths_held", "<u4", 2),
                       ("paths_cntr", "<u4", 2), ("max_step_gap", "<u8", 2), ("gap_conf", "<f8", 2), ("stop_causes", "u1", 2),
                       ("outdegree_rv", "u1"), ("outdegree_fw", "u1")], align=True)
CONTIGS_RESEED, CONTIGS_NO_MISSING_CHECK = 1, 2


class BubblesParams(C.Structure):
    """mcx_bubbles_params"""
    _fields_ = [("max_allele", C.c_uint32), ("max_flank", C.c_uint32), ("flags", C.c_uint32), ("nhaploid", C.c_uint32), ("haploid", C.c_void_p)]


class BubblesStats(C.Structure):
    """mcx_bubbles_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("forks", "paths", "steps", "stop_limit", "stop_nocovg", "stop_nocolcovg", "stop_nolinks", "stop_repeat",
                                          "candidates", "bubbles", "branches", "haploid_dropped", "serial_dropped")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# mcx_bubble_rec
BUBBLE_REC = np.dtype([("fork_key", "<u8", 4), ("text_off", "<u8"), ("text_len", "<u8"), ("fork_orient", "<u4"), ("num_branches", "<u4"),
                       ("flank5p_kmers", "<u4"), ("flank3p_kmers", "<u4")], align=True)
BUBBLES_KEEP_SERIAL = 1


class BreakpointsParams(C.Structure):
    """mcx_breakpoints_params"""
    _fields_ = [("min_ref", C.c_uint32), ("max_ref", C.c_uint32), ("flags", C.c_uint32)]


class BreakpointsStats(C.Structure):
    """mcx_breakpoints_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("occurrences", "ref_keys", "ref_added", "breaks", "flank_walks", "flanks", "flanks_norun", "allele_walks",
                                          "alleles", "alleles_norun", "calls", "steps", "runs_started", "runs_ended", "stop_runs", "stop_maxref",
                                          "stop_flank", "stop_nocovg", "stop_nocolcovg", "stop_nolinks", "stop_repeat", "stop_bound", "reruns")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# mcx_breakpoint_rec
BREAKPOINT_REC = np.dtype([("fork_key", "<u8", 4), ("text_off", "<u8"), ("text_len", "<u8"), ("fork_orient", "<u4"), ("succ_base", "<u4"),
                           ("num_cols", "<u4"), ("path_kmers", "<u4"), ("flank5p_kmers", "<u4"), ("flank3p_kmers", "<u4"), ("flank5p_runs", "<u4"),
                           ("flank3p_runs", "<u4")], align=True)
BREAKPOINTS_NO_REF_EDGES, BREAKPOINTS_REF_LOADED, BREAKPOINTS_LOAD_ONLY = 1, 2, 4


class UnitigsStats(C.Structure):
    """mcx_unitigs_stats"""
    _fields_ = [(n, C.c_uint64) for n in ("num_unitigs", "num_kmers", "num_bytes", "num_cycles")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class JoinStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("recs_read", "recs_kept", "isec_recs_read", "isec_recs_kept", "kmers_written",
                                          "kmers_intersection", "kmers_written_no_covg")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class LinksParams(C.Structure):
    """mcx_links_params"""
    _fields_ = [("flags", C.c_uint32), ("distsize", C.c_uint32), ("covgsize", C.c_uint32), ("reserved", C.c_uint32),
                ("cutoff", C.c_uint64), ("max_kmers", C.c_uint64)]


class LinksStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("kmers_read", "kmers_with_links", "links", "link_bytes", "tree_links", "links_in")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PjoinPieceStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("kmer_lines", "link_lines", "links_kept", "kmers_n_mismatch")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PjoinStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("kmer_lines", "link_lines", "links_kept", "kmers_n_mismatch", "kmers", "links", "path_bytes",
                                          "compactions", "store_bytes", "peak_store_bytes")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class UnitigsArrays(C.Structure):
    """mcx_unitigs_arrays (device pointers)"""
    _fields_ = [(n, C.c_void_p) for n in ("keys", "unitig", "rank", "orient", "first", "length")]


CLEAN_NBINS = 1000
UNITIGS_FORMATS = {"fasta": 0, "gfa": 1, "dot": 2}
UNITIGS_POINTS = 1
RECORDS_MUST_EXIST = 1
INFER_POP, INFER_PRESENCE_COVG = 1, 2
SUBGRAPH_UNITIGS, SUBGRAPH_INVERT = 1, 2
COVERAGE_EDGES, COVERAGE_DEGREES = 1, 2
CORRECT_TWO_WAY = 1
THREAD_TWO_WAY = 1
LINKS_SEQ = 1
SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)


def lib():
    """Load libmcxgpu.so; raises if the HIP extension has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same SONAME as
    # /opt/rocm's).  Importing torch first makes the loader bind this library to the runtime
    # torch uses, so torch tensors' device pointers are valid in our kernels.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("MCX_LIB") or _build.LIB  # MCX_LIB: tuning variants built by tools/
    if not os.path.exists(path):
        raise RuntimeError("HIP extension missing: %s (run __graft_entry__.build())" % path)
    L = C.CDLL(path)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    L.mcx_last_error.restype = C.c_char_p
    L.mcx_version.restype = C.c_char_p
    L.mcx_device_count.restype = C.c_int
    L.mcx_graph_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint64, C.c_int]
    L.mcx_graph_create_shard.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int]
    L.mcx_graph_create_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.c_int]
    L.mcx_graph_ndevices.argtypes = [vp]
    L.mcx_graph_shard_layout.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32), u64p, u64p]
    L.mcx_graph_shard_bins_dev.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64]
    L.mcx_graph_add_segments_dev.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64]
    L.mcx_graph_insert_tuple_segments_dev.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint32, C.c_uint64]
    L.mcx_graph_add_records.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, C.c_int, C.c_uint32, C.POINTER(RecordStats)]
    L.mcx_graph_kmer_covg.argtypes = [vp, u64p, u64p]
    L.mcx_graph_insert_stats.argtypes = [vp, vp]
    L.mcx_graph_covg_histogram.argtypes = [vp, u64p, C.c_uint32]
    L.mcx_sort_records.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, C.c_int]
    L.mcx_records_sorted.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.mcx_graph_intersect_finish.argtypes = [vp, u64p]
    L.mcx_join_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
    L.mcx_join_configure.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.mcx_join_add_records.argtypes = [vp, C.c_int, vp, C.c_uint64, C.c_int, vp, vp, C.c_int]
    L.mcx_join_finish.argtypes = [vp, SINK_FN, vp, C.POINTER(JoinStats)]
    L.mcx_join_get_stats.argtypes = [vp, C.POINTER(JoinStats)]
    L.mcx_join_buffer.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.mcx_join_phases.argtypes = [vp, C.POINTER(C.c_double)]
    L.mcx_join_destroy.argtypes = [vp]
    L.mcx_join_destroy.restype = None
    L.mcx_links_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    L.mcx_links_configure.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.mcx_links_buffer.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.mcx_links_add_text.argtypes = [vp, vp, C.c_uint64, C.POINTER(LinksParams), SINK_FN, vp, SINK_FN, vp]
    L.mcx_links_get_stats.argtypes = [vp, C.POINTER(LinksStats)]
    L.mcx_links_hist.argtypes = [vp, u64p]
    L.mcx_links_error.argtypes = [vp, C.POINTER(C.c_int), u64p]
    L.mcx_links_phases.argtypes = [vp, C.POINTER(C.c_double)]
    L.mcx_links_destroy.argtypes = [vp]
    L.mcx_links_destroy.restype = None
    L.mcx_pjoin_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int]
    L.mcx_pjoin_configure.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.mcx_pjoin_buffer.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.mcx_pjoin_add_text.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, C.c_int, C.POINTER(PjoinPieceStats)]
    L.mcx_pjoin_finish.argtypes = [vp, SINK_FN, vp, C.POINTER(PjoinStats)]
    L.mcx_pjoin_get_stats.argtypes = [vp, C.POINTER(PjoinStats)]
    L.mcx_pjoin_error.argtypes = [vp, C.POINTER(C.c_int), u64p]
    L.mcx_pjoin_phases.argtypes = [vp, C.POINTER(C.c_double)]
    L.mcx_pjoin_destroy.argtypes = [vp]
    L.mcx_pjoin_destroy.restype = None
    L.mcx_graph_unitig_stats.argtypes = [vp, vp]
    L.mcx_graph_clean.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(CleanStats), vp]
    L.mcx_graph_pop_bubbles.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PopStats)]
    L.mcx_graph_subgraph_begin.argtypes = [vp, C.c_uint32]
    L.mcx_graph_subgraph_seed_reads.argtypes = [vp, vp, vp, C.c_uint64]
    L.mcx_graph_subgraph_seed_stream_dev.argtypes = [vp, vp, C.c_uint64]
    L.mcx_graph_subgraph_finish.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(SubgraphStats)]
    L.mcx_graph_reads_touch.argtypes = [vp, vp, vp, C.c_uint64, vp, C.POINTER(TouchStats)]
    L.mcx_graph_reads_touch_stream_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp]
    L.mcx_graph_coverage.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.POINTER(CoverageStats)]
    L.mcx_graph_coverage_stream_dev.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64]
    L.mcx_graph_coverage_text.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, SINK_FN, vp, vp, C.POINTER(CoverageStats)]
    L.mcx_graph_correct.argtypes = [vp, vp, vp, vp, C.c_uint64, C.POINTER(CorrectParams), SINK_FN, vp, vp, C.POINTER(CorrectStats)]
    L.mcx_graph_correct_stream_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(CorrectParams), vp, C.c_uint64, vp,
                                               C.POINTER(CorrectStats)]
    L.mcx_graph_correct_walk_steps.argtypes = [vp]
    L.mcx_graph_thread.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(ThreadParams), C.POINTER(ThreadStats)]
    L.mcx_graph_links_info.argtypes = [vp, C.POINTER(LinksInfo)]
    L.mcx_graph_links_contig_hist.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_graph_links_text.argtypes = [vp, C.c_uint32, SINK_FN, vp]
    L.mcx_graph_links_reset.argtypes = [vp]
    L.mcx_graph_links_load_text.argtypes = [vp, vp, C.c_uint64, u64p, u64p]
    L.mcx_graph_contigs.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(ContigsParams), SINK_FN, vp, SINK_FN, vp, C.POINTER(ContigsStats)]
    L.mcx_graph_bubbles.argtypes = [vp, C.POINTER(BubblesParams), SINK_FN, vp, SINK_FN, vp, C.POINTER(BubblesStats)]
    L.mcx_graph_breakpoints.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.POINTER(BreakpointsParams), SINK_FN, vp, SINK_FN, vp, C.POINTER(BreakpointsStats)]
    L.mcx_graph_correct_walk_steps.restype = C.c_uint64
    L.mcx_graph_unitigs.argtypes = [vp, C.c_int, C.c_uint32, SINK_FN, vp, C.POINTER(UnitigsStats)]
    L.mcx_graph_unitigs_dev.argtypes = [vp, C.POINTER(UnitigsArrays), C.POINTER(UnitigsStats)]
    L.mcx_graph_infer_edges.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint32, u64p]
    L.mcx_graph_infer_edges_dev.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint32, u64p]
    L.mcx_superk_supported.argtypes = [C.c_int]
    L.mcx_superk_record_bytes.argtypes = [C.c_int]
    L.mcx_superk_owner.restype = C.c_uint32
    L.mcx_superk_owner.argtypes = [u64p, C.c_int, C.c_int]
    L.mcx_graph_superk_layout.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(C.c_uint32), u64p]
    L.mcx_graph_superk_bins_dev.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, C.c_uint64]
    L.mcx_graph_add_superk_dev.argtypes = [vp, C.c_int, vp, vp, C.c_uint32, C.c_uint64, C.c_uint64]
    L.mcx_graph_checksum.argtypes = [vp, u64p, u64p]
    L.mcx_records_checksum.restype = C.c_uint64
    L.mcx_records_checksum.argtypes = [vp, C.c_uint64, C.c_int, C.c_int]
    L.mcx_ubench_stream.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mcx_ubench_random_rmw.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mcx_graph_key_owner.restype = C.c_uint32
    L.mcx_graph_key_owner.argtypes = [vp, u64p]
    L.mcx_graph_destroy.argtypes = [vp]
    L.mcx_graph_destroy.restype = None
    L.mcx_graph_reset.argtypes = [vp]
    L.mcx_graph_capacity.argtypes = [vp, u64p, u64p]
    L.mcx_graph_configure.argtypes = [vp, C.c_char_p, C.c_uint64]
    L.mcx_graph_profile.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.mcx_graph_add_reads.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint64, C.c_uint8, C.c_uint8,
                                      C.POINTER(LoadStats)]
    L.mcx_graph_add_reads_pcr.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint64, C.c_uint8, C.c_uint8, C.c_uint8,
                                          C.c_int, C.c_int, C.POINTER(LoadStats)]
    L.mcx_graph_pcr_reset.argtypes = [vp]
    L.mcx_graph_add_stream_dev.argtypes = [vp, C.c_int, vp, C.c_uint64]
    L.mcx_pack_stream_dev.argtypes = [vp, C.c_uint64, vp, vp, vp]
    L.mcx_graph_add_packed_dev.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
    L.mcx_graph_partition_stream_dev.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint64, vp, vp, vp]
    L.mcx_graph_insert_tuples_dev.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
    L.mcx_graph_hashtest.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.mcx_hashtest_func.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.mcx_key_owner.restype = C.c_uint32
    L.mcx_key_owner.argtypes = [u64p, C.c_int, C.c_int]
    L.mcx_graph_sync.argtypes = [vp]
    L.mcx_graph_nkmers.argtypes = [vp, u64p]
    L.mcx_graph_device_stats.argtypes = [vp, C.POINTER(LoadStats)]
    L.mcx_graph_stream.restype = vp
    L.mcx_graph_stream.argtypes = [vp]
    L.mcx_graph_export.argtypes = [vp, C.c_int, SINK_FN, vp]
    L.mcx_kmer_from_str.restype = None
    L.mcx_kmer_from_str.argtypes = [C.c_char_p, C.c_int, u64p]
    L.mcx_kmer_canonical.restype = None
    L.mcx_kmer_canonical.argtypes = [u64p, C.c_int, u64p, C.POINTER(C.c_int)]
    L.mcx_kmer_hash.restype = C.c_uint32
    L.mcx_kmer_hash.argtypes = [u64p, C.c_int, C.c_uint32]
    _LIB = L
    return L


def _check(rc):
    if rc != MCX_OK:
        raise McxError(rc, lib().mcx_last_error().decode())


def device_count():
    return lib().mcx_device_count()


def _words(k):
    return (2 * k + 63) // 64


def kmer_from_str(s, k):
    out = (C.c_uint64 * 4)()
    lib().mcx_kmer_from_str(s.encode() if isinstance(s, str) else s, k, out)
    return [int(out[i]) for i in range(_words(k))]


def kmer_canonical(words, k):
    a = (C.c_uint64 * 4)(*words)
    out = (C.c_uint64 * 4)()
    o = C.c_int()
    lib().mcx_kmer_canonical(a, k, out, C.byref(o))
    return [int(out[i]) for i in range(_words(k))], int(o.value)


def kmer_hash(words, k, initval=0):
    a = (C.c_uint64 * 4)(*words)
    return int(lib().mcx_kmer_hash(a, k, initval))


def key_owner(words, k, nparts):
    a = (C.c_uint64 * 2)(*words)
    return int(lib().mcx_key_owner(a, k, nparts))


def stream_from_reads(reads):
    """Host helper: reads -> the separator-delimited byte stream the device entry takes."""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    return np.frombuffer(b"".join(b + b"\n" for b in bs), dtype=np.uint8).copy()


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p)
    if hasattr(x, "data_ptr"):  # torch tensor (device or host)
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


class Graph:
    """One coloured de Bruijn graph resident in the HBM of one GPU."""

    def __init__(self, kmer_size, ncols=1, capacity=1 << 20, device=0, nparts=1, part=0, devices=None):
        """devices: list of device ordinals -> one table split over them (mcx_graph_create_multi);
        the same ordinal may repeat (several shards on one GPU: how the path is tested on one)."""
        self.L = lib()
        self.k, self.ncols, self.W = kmer_size, ncols, _words(kmer_size)
        self.nparts, self.part = nparts, part
        self.device = device if devices is None else devices[0]
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            _check(self.L.mcx_graph_create_multi(C.byref(h), kmer_size, ncols, capacity, arr, len(devices)))
        else:
            _check(self.L.mcx_graph_create_shard(C.byref(h), kmer_size, ncols, capacity, device, nparts, part))
        self.h = h

    @property
    def ndevices(self):
        return int(self.L.mcx_graph_ndevices(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.mcx_graph_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _check(self.L.mcx_graph_reset(self.h))

    def configure(self, key, value):
        _check(self.L.mcx_graph_configure(self.h, key.encode(), int(value)))

    def profile(self):
        """{kernel: (calls, total_ms)} for launches recorded since configure('profile', 1)."""
        buf = C.create_string_buffer(16384)   # (a multi-GPU handle reports every shard's kernels: name@shard)
        _check(self.L.mcx_graph_profile(self.h, buf, 16384))
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.split()
            out[name] = (int(calls), float(ms))
        return out

    def capacity(self):
        s, b = C.c_uint64(), C.c_uint64()
        _check(self.L.mcx_graph_capacity(self.h, C.byref(s), C.byref(b)))
        return int(s.value), int(b.value)

    def add_reads(self, colour, bases, offsets, quals=None, fq_cutoff=0, hp_cutoff=0, stats=None):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        st = stats if stats is not None else LoadStats()
        _check(self.L.mcx_graph_add_reads(self.h, colour, _ptr(bases), _ptr(quals), _ptr(offsets),
                                          len(offsets) - 1, fq_cutoff, hp_cutoff, C.byref(st)))
        return st

    MATEDIR = {"FF": 0, "FR": 1, "RF": 2, "RR": 3}

    def add_reads_pcr(self, colour, bases, offsets, quals=None, fq_cutoff=0, fq_cutoff2=None, hp_cutoff=0,
                      paired=False, matedir="FR", stats=None):
        """`build --remove-pcr` over one batch (reads 2i, 2i + 1 are mates when `paired`)"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        st = stats if stats is not None else LoadStats()
        _check(self.L.mcx_graph_add_reads_pcr(self.h, colour, _ptr(bases), _ptr(quals), _ptr(offsets), len(offsets) - 1,
                                              fq_cutoff, fq_cutoff if fq_cutoff2 is None else fq_cutoff2, hp_cutoff,
                                              1 if paired else 0, self.MATEDIR.get(matedir, matedir), C.byref(st)))
        return st

    def pcr_reset(self):
        _check(self.L.mcx_graph_pcr_reset(self.h))

    def superk_layout(self, nparts, positions_per_call):
        segs, cap = C.c_uint32(), C.c_uint64()
        _check(self.L.mcx_graph_superk_layout(self.h, nparts, int(positions_per_call), C.byref(segs), C.byref(cap)))
        return int(segs.value), int(cap.value)

    def superk_bins_dev(self, d_stream, nbytes, nparts, d_recs, d_counts, seg_cap):
        _check(self.L.mcx_graph_superk_bins_dev(self.h, _ptr(d_stream), nbytes, nparts, _ptr(d_recs), _ptr(d_counts), seg_cap))

    def add_superk_dev(self, colour, d_recs, d_counts, nseg, seg_cap, kmers_upper_bound):
        _check(self.L.mcx_graph_add_superk_dev(self.h, colour, _ptr(d_recs), _ptr(d_counts), nseg, seg_cap, int(kmers_upper_bound)))

    def checksum(self):
        """(order-independent checksum of the exported records, number of k-mers)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self.L.mcx_graph_checksum(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def intersect_finish(self):
        n = C.c_uint64(0)
        _check(self.L.mcx_graph_intersect_finish(self.h, C.byref(n)))
        return int(n.value)

    def add_records(self, recs, file_ncols, colour_filter, must_exist=False, stats=None, mask_edges=False):
        """recs: .ctx body bytes (W x u64 key, file_ncols x u32 coverage, file_ncols x u8 edges per
        record); colour_filter: [(from file colour, into graph colour)]"""
        recs = np.frombuffer(recs, dtype=np.uint8) if isinstance(recs, (bytes, bytearray, memoryview)) else np.ascontiguousarray(recs, dtype=np.uint8)
        rs = 8 * self.W + 5 * file_ncols
        assert recs.size % rs == 0
        frm = np.array([f for f, _ in colour_filter], dtype=np.int32)
        into = np.array([t for _, t in colour_filter], dtype=np.int32)
        st = stats if stats is not None else RecordStats()
        _check(self.L.mcx_graph_add_records(self.h, _ptr(recs), recs.size // rs, file_ncols, _ptr(frm), _ptr(into),
                                            len(frm), (RECORDS_MUST_EXIST if must_exist else 0) | (2 if mask_edges else 0), C.byref(st)))
        return st

    def _infer_flags(self, pop, presence):
        if presence not in ("any", "covg"):
            raise ValueError("presence must be 'any' (a file: coverage or edges) or 'covg' (a stream)")
        return (INFER_POP if pop else 0) | (INFER_PRESENCE_COVG if presence == "covg" else 0)

    def infer_edges(self, recs, pop=False, presence="any"):
        """`inferedges` over .ctx body bytes (self.ncols colours) against the loaded graph:
        returns (the records with the inferred edges added, number of records modified)"""
        a = np.frombuffer(bytes(recs), dtype=np.uint8).copy()
        rs = 8 * self.W + 5 * self.ncols
        assert a.size % rs == 0
        n = C.c_uint64(0)
        _check(self.L.mcx_graph_infer_edges(self.h, _ptr(a), a.size // rs, self.ncols, self._infer_flags(pop, presence),
                                            C.byref(n)))
        return a.tobytes(), int(n.value)

    def infer_edges_dev(self, d_recs, nrecs, pop=False, presence="any"):
        """the same over records already in HBM (a device pointer or tensor), updated in place; returns records modified"""
        n = C.c_uint64(0)
        _check(self.L.mcx_graph_infer_edges_dev(self.h, _ptr(d_recs), int(nrecs), self.ncols, self._infer_flags(pop, presence),
                                                C.byref(n)))
        return int(n.value)

    @staticmethod
    def _clean_hists(a):
        return {"kmer_covg": a[:CLEAN_NBINS], "unitig_covg": a[CLEAN_NBINS:2 * CLEAN_NBINS], "unitig_len": a[2 * CLEAN_NBINS:]}

    def unitig_stats(self):
        """`clean`'s first pass: split the graph into unitigs on the device and return the "before" histograms
        {kmer_covg, unitig_covg (median), unitig_len}, 1000 bins each; the decomposition is kept for clean()"""
        a = np.zeros(3 * CLEAN_NBINS, dtype=np.uint64)
        _check(self.L.mcx_graph_unitig_stats(self.h, _ptr(a)))
        return self._clean_hists(a)

    def clean(self, threshold, tips):
        """remove unitigs with median coverage < threshold and tips shorter than `tips` k-mers (0 = off):
        returns (stats dict, "after" histograms of the kept unitigs)"""
        a = np.zeros(3 * CLEAN_NBINS, dtype=np.uint64)
        st = CleanStats()
        _check(self.L.mcx_graph_clean(self.h, int(threshold), int(tips), C.byref(st), _ptr(a)))
        return st.as_dict(), self._clean_hists(a)

    def kmer_covg(self):
        """per colour: (k-mers with coverage, summed coverage) -- db_graph_get_kmer_covg"""
        nk = np.zeros(self.ncols, dtype=np.uint64)
        sc = np.zeros(self.ncols, dtype=np.uint64)
        _check(self.L.mcx_graph_kmer_covg(self.h, nk.ctypes.data_as(C.POINTER(C.c_uint64)), sc.ctypes.data_as(C.POINTER(C.c_uint64))))
        return nk, sc

    def covg_histogram(self, nbins):
        h = np.zeros(nbins, dtype=np.uint64)
        _check(self.L.mcx_graph_covg_histogram(self.h, h.ctypes.data_as(C.POINTER(C.c_uint64)), nbins))
        return h

    def add_packed_dev(self, colour, d_code, d_inv, npos):
        """a device-resident stream in packed form (pack_stream_dev): 3 bits per position"""
        _check(self.L.mcx_graph_add_packed_dev(self.h, colour, _ptr(d_code), _ptr(d_inv), int(npos)))

    def add_stream_dev(self, colour, d_stream, nbytes):
        _check(self.L.mcx_graph_add_stream_dev(self.h, colour, _ptr(d_stream), nbytes))

    def partition_stream_dev(self, d_stream, nbytes, nparts, bin_capacity, d_keys, d_edges, d_counts):
        _check(self.L.mcx_graph_partition_stream_dev(self.h, _ptr(d_stream), nbytes, nparts, bin_capacity,
                                                     _ptr(d_keys), _ptr(d_edges), _ptr(d_counts)))

    def hashtest(self, first, n):
        """The reference's `hashtest`: find-or-insert of the keys whose top word is first .. first + n - 1."""
        _check(self.L.mcx_graph_hashtest(self.h, first, n))

    def insert_tuples_dev(self, colour, d_keys, d_edges, n):
        _check(self.L.mcx_graph_insert_tuples_dev(self.h, colour, _ptr(d_keys), _ptr(d_edges), n))

    def shard_layout(self, tuples_per_call):
        """(segments per owner, tuples per segment, overflow capacity per owner)"""
        segs, cap, ov = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(self.L.mcx_graph_shard_layout(self.h, int(tuples_per_call), C.byref(segs), C.byref(cap), C.byref(ov)))
        return int(segs.value), int(cap.value), int(ov.value)

    def shard_bins_dev(self, d_stream, nbytes, d_keys, d_counts, seg_cap, d_ov_keys, d_ov_edges, d_ov_counts, ov_cap):
        _check(self.L.mcx_graph_shard_bins_dev(self.h, _ptr(d_stream), nbytes, _ptr(d_keys), _ptr(d_counts), seg_cap,
                                               _ptr(d_ov_keys), _ptr(d_ov_edges), _ptr(d_ov_counts), ov_cap))

    def add_segments_dev(self, colour, d_keys, d_counts, nseg, seg_cap, ntuples):
        _check(self.L.mcx_graph_add_segments_dev(self.h, colour, _ptr(d_keys), _ptr(d_counts), nseg, seg_cap, int(ntuples)))

    def insert_tuple_segments_dev(self, colour, d_keys, d_edges, d_counts, nseg, seg_cap):
        _check(self.L.mcx_graph_insert_tuple_segments_dev(self.h, colour, _ptr(d_keys), _ptr(d_edges), _ptr(d_counts),
                                                          nseg, seg_cap))

    def key_owner(self, words):
        a = (C.c_uint64 * 2)(*words)
        return int(self.L.mcx_graph_key_owner(self.h, a))

    def sync(self):
        _check(self.L.mcx_graph_sync(self.h))

    @property
    def nkmers(self):
        n = C.c_uint64()
        _check(self.L.mcx_graph_nkmers(self.h, C.byref(n)))
        return int(n.value)

    def device_stats(self):
        st = LoadStats()
        _check(self.L.mcx_graph_device_stats(self.h, C.byref(st)))
        return st

    def insert_stats(self):
        """mcx_insert_stats as a dict: fallback_inserts, foreign_inserts, spilled, flushes (implies a sync)"""
        st = (C.c_uint64 * 4)()
        _check(self.L.mcx_graph_insert_stats(self.h, st))
        return dict(zip(("fallback_inserts", "foreign_inserts", "spilled", "flushes"), (int(x) for x in st)))

    @property
    def stream(self):
        return self.L.mcx_graph_stream(self.h)

    def pop_bubbles(self, max_covg=-1, max_klen=-1, max_kdiff=-1):
        """`popbubbles` (ctx_pop_bubbles.c): of two parallel unitigs the one with the lower mean coverage goes, if its mean
        is <= max_covg and its length <= max_klen (<= 0: ignored) and the lengths differ by <= max_kdiff (< 0: ignored).
        Returns the stats dict (num_popped, num_pairs, nkmers_before, nkmers_removed, num_unitigs_removed, rounds)"""
        st = PopStats()
        _check(self.L.mcx_graph_pop_bubbles(self.h, int(max_covg), int(max_klen), int(max_kdiff), C.byref(st)))
        return st.as_dict()

    def subgraph_begin(self, unitigs=False):
        """`subgraph`, first step: set up the marks and the queue on the device (unitigs: seeds mark whole unitigs)"""
        _check(self.L.mcx_graph_subgraph_begin(self.h, SUBGRAPH_UNITIGS if unitigs else 0))

    def subgraph_seed(self, bases, offsets):
        """mark the k-mers of the seed reads (the layout of add_reads) that are in the graph; may be repeated"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        _check(self.L.mcx_graph_subgraph_seed_reads(self.h, _ptr(bases), _ptr(offsets), len(offsets) - 1))

    def subgraph_seed_stream_dev(self, d_stream, nbytes):
        """the same for an ASCII stream in HBM (the layout of add_stream_dev)"""
        _check(self.L.mcx_graph_subgraph_seed_stream_dev(self.h, _ptr(d_stream), int(nbytes)))

    def subgraph_finish(self, dist=0, invert=False, unitigs=False):
        """extend the marked set by `dist` edges, complement it with `invert`, prune the rest; returns the stats dict"""
        st = SubgraphStats()
        _check(self.L.mcx_graph_subgraph_finish(self.h, int(dist), (SUBGRAPH_UNITIGS if unitigs else 0) | (SUBGRAPH_INVERT if invert else 0),
                                                C.byref(st)))
        return st.as_dict()

    def reads_touch(self, bases, offsets, stats=None):
        """`reads` (ctx_reads.c, read_touches_graph): (np.uint8[nreads] of 0 / 1, TouchStats) -- hit[r] = 1 iff read r
        (bases[offsets[r]:offsets[r + 1]]) has a k-mer in the graph.  `stats`, if given, is added to."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nreads = max(len(offsets) - 1, 0)
        hit = np.zeros(nreads, dtype=np.uint8)
        st = stats if stats is not None else TouchStats()
        _check(self.L.mcx_graph_reads_touch(self.h, _ptr(bases), _ptr(offsets), nreads, _ptr(hit), C.byref(st)))
        return hit, st

    def reads_touch_stream_dev(self, d_stream, nbytes, d_stream_off, nreads, d_hit):
        """the same over a stream in HBM (torch tensors or addresses); asynchronous on the graph's stream"""
        _check(self.L.mcx_graph_reads_touch_stream_dev(self.h, _ptr(d_stream), int(nbytes), _ptr(d_stream_off), int(nreads), _ptr(d_hit)))

    def coverage(self, bases, offsets, edges=False, stats=None):
        """`coverage` (ctx_coverage.c, print_read_covg): (np.uint32[ncols, nbases], np.uint8[ncols, nbases] or None,
        CoverageStats) with nbases = offsets[-1] -- index p of a colour holds the coverage (and the edges, turned to the
        read's strand) of the k-mer that starts at bases[p], 0 where none does or it is not in the graph.  `stats`, if
        given, is added to."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nreads = max(len(offsets) - 1, 0)
        nbases = int(offsets[-1]) if len(offsets) else 0
        covg = np.zeros((self.ncols, nbases), dtype=np.uint32)
        edg = np.zeros((self.ncols, nbases), dtype=np.uint8) if edges else None
        st = stats if stats is not None else CoverageStats()
        _check(self.L.mcx_graph_coverage(self.h, _ptr(bases), _ptr(offsets), nreads, _ptr(covg), _ptr(edg) if edges else None, C.byref(st)))
        return covg, edg, st

    def coverage_stream_dev(self, d_stream, nbytes, d_covg, d_edges, pitch):
        """the same over a stream in HBM (torch tensors or addresses) into d_covg[ncols, pitch] (32-bit) and, unless
        None, d_edges[ncols, pitch] (bytes), indexed by stream position; asynchronous on the graph's stream"""
        _check(self.L.mcx_graph_coverage_stream_dev(self.h, _ptr(d_stream), int(nbytes), _ptr(d_covg),
                                                    _ptr(d_edges) if d_edges is not None else None, int(pitch)))

    def coverage_text(self, bases, offsets, edges=False, degrees=False, stats=None):
        """the value lines of `coverage`, written on the device: (bytes, np.uint64 line_off, CoverageStats).  Per read and
        colour the edges line (if `edges`), the degree line (if `degrees`) and the coverage line; line i is
        text[line_off[i]:line_off[i + 1]]"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nreads = max(len(offsets) - 1, 0)
        flags = (COVERAGE_EDGES if edges else 0) | (COVERAGE_DEGREES if degrees else 0)
        line_off = np.zeros(nreads * self.ncols * (1 + bool(edges) + bool(degrees)) + 1, dtype=np.uint64)
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n))
            return 0

        st = stats if stats is not None else CoverageStats()
        _check(self.L.mcx_graph_coverage_text(self.h, _ptr(bases), _ptr(offsets), nreads, flags, SINK_FN(sink), None, _ptr(line_off),
                                              C.byref(st)))
        return b"".join(parts), line_off, st

    @staticmethod
    def _correct_params(colour, two_way, gap_variance, gap_wiggle, fq_zero):
        z = fq_zero.encode() if isinstance(fq_zero, str) else bytes(fq_zero)
        return CorrectParams(int(colour), CORRECT_TWO_WAY if two_way else 0, float(gap_variance), float(gap_wiggle), z[:1] or b"\0")

    def correct(self, bases, offsets, quals=None, colour=0, two_way=False, gap_variance=0.1, gap_wiggle=5.0, fq_zero=".", stats=None):
        """`correct` (ctx_correct.c without link files): (bytes, np.uint64 out_off, CorrectStats).  Record r is
        out[out_off[r]:out_off[r + 1]]: the corrected sequence of read r and, when `quals` (a byte per base) is given, as
        many quality bytes behind it, `fq_zero` for every base a walk supplied.  `stats`, if given, is added to."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            if len(quals) < (int(offsets[-1]) if len(offsets) else 0):
                raise ValueError("quals must hold a byte per base")
        nreads = max(len(offsets) - 1, 0)
        out_off = np.zeros(nreads + 1, dtype=np.uint64)
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n))
            return 0

        st = stats if stats is not None else CorrectStats()
        prm = self._correct_params(colour, two_way, gap_variance, gap_wiggle, fq_zero)
        _check(self.L.mcx_graph_correct(self.h, _ptr(bases), _ptr(quals) if quals is not None else None, _ptr(offsets), nreads, C.byref(prm),
                                        SINK_FN(sink), None, _ptr(out_off), C.byref(st)))
        return b"".join(parts), out_off, st

    def correct_stream_dev(self, d_stream, nbytes, d_stream_off, nreads, d_node, pitch, d_len, colour=0, two_way=False, gap_variance=0.1,
                           gap_wiggle=5.0, stats=None):
        """the probe, the tasks and the walks of `correct` over a stream in HBM (torch tensors or addresses): d_node is
        scratch of `pitch` 64-bit words, d_len receives the record lengths; returns the CorrectStats"""
        st = stats if stats is not None else CorrectStats()
        prm = self._correct_params(colour, two_way, gap_variance, gap_wiggle, ".")
        _check(self.L.mcx_graph_correct_stream_dev(self.h, _ptr(d_stream), int(nbytes), _ptr(d_stream_off), int(nreads), C.byref(prm),
                                                   _ptr(d_node), int(pitch), _ptr(d_len), C.byref(st)))
        return st

    def correct_walk_steps(self):
        """walker steps of the last correct / correct_stream_dev call"""
        return int(self.L.mcx_graph_correct_walk_steps(self.h))

    def thread(self, bases, offsets, two_way=False, gap_variance=0.1, gap_wiggle=5.0, max_juncs=0, stats=None):
        """`thread` (ctx_thread.c without -p and -u) over a graph of one colour: the links of the reads' contigs are
        generated and added to those the handle keeps.  Returns the ThreadStats (`stats`, if given, is added to)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nreads = max(len(offsets) - 1, 0)
        st = stats if stats is not None else ThreadStats()
        prm = ThreadParams(THREAD_TWO_WAY if two_way else 0, float(gap_variance), float(gap_wiggle), int(max_juncs))
        _check(self.L.mcx_graph_thread(self.h, _ptr(bases), _ptr(offsets), nreads, C.byref(prm), C.byref(st)))
        return st

    def links_info(self):
        """{num_kmers_with_paths, num_paths, path_bytes} of the links kept"""
        out = LinksInfo()
        _check(self.L.mcx_graph_links_info(self.h, C.byref(out)))
        return out.as_dict()

    def links_contig_hist(self):
        """[(contig length in bases, contigs)] in ascending length"""
        n = C.c_uint64(0)
        _check(self.L.mcx_graph_links_contig_hist(self.h, None, None, 0, C.byref(n)))
        lengths, counts = np.zeros(n.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64)
        _check(self.L.mcx_graph_links_contig_hist(self.h, _ptr(lengths), _ptr(counts), n.value, C.byref(n)))
        return list(zip(lengths.tolist(), counts.tolist()))

    def links_text(self, seq=True):
        """the body of the .ctp file (bytes): per k-mer in key order `<kmer> <nlinks>`, then its links; with `seq` every
        link carries seq= and juncpos="""
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n))
            return 0

        _check(self.L.mcx_graph_links_text(self.h, LINKS_SEQ if seq else 0, SINK_FN(sink), None))
        return b"".join(parts)

    def links_reset(self):
        """forget the links and the contig histogram"""
        _check(self.L.mcx_graph_links_reset(self.h))

    def links_load_text(self, text):
        """the links of whole k-mer blocks of a version-4, one-colour .ctp body onto the handle, merged with those it keeps.
        Returns (link lines stored, k-mers missing); raises McxError (with .nmissing set) when a k-mer is not in the graph."""
        text = bytes(text)
        nl, nm = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.mcx_graph_links_load_text(self.h, text, len(text), C.byref(nl), C.byref(nm))
        if rc != MCX_OK:
            err = McxError(rc, self.L.mcx_last_error().decode())
            err.nmissing = int(nm.value)
            raise err
        return int(nl.value), int(nm.value)

    def contigs(self, conf=(), colour=0, seeds=None, reseed=False, missing_check=True, ncontigs=0, min_step_confid=-1.0,
                min_cumul_confid=-1.0, stats=None, want_seq=True):
        """`contigs` (ctx_contigs.c): every seed walked both ways with the links on the handle.  seeds: None = every key of
        the sample in key order, else a list of k-base strings.  conf: the confidence table indexed by gap length.
        Returns (records as a CONTIG_REC array, the sequences as bytes `<bases>\n` per contig, ContigsStats)."""
        conf = np.ascontiguousarray(conf, dtype=np.float64)
        bases = offsets = None
        nseeds = 0
        if seeds is not None:
            bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seeds]
            nseeds = len(bs)
            bases = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy()
            offsets = np.cumsum([0] + [len(b) for b in bs]).astype(np.uint64)
        recs, seq = [], []

        def rec_sink(_ctx, ptr, n):
            recs.append(C.string_at(ptr, n))
            return 0

        def seq_sink(_ctx, ptr, n):
            seq.append(C.string_at(ptr, n))
            return 0

        st = stats if stats is not None else ContigsStats()
        flags = (CONTIGS_RESEED if reseed else 0) | (0 if missing_check else CONTIGS_NO_MISSING_CHECK)
        prm = ContigsParams(int(colour), flags, int(ncontigs), float(min_step_confid), float(min_cumul_confid),
                            conf.ctypes.data_as(C.c_void_p) if len(conf) else None, len(conf))
        a, b = SINK_FN(rec_sink), SINK_FN(seq_sink)
        _check(self.L.mcx_graph_contigs(self.h, _ptr(bases), _ptr(offsets), nseeds, C.byref(prm), a, None, b if want_seq else C.cast(None, SINK_FN), None,
                                        C.byref(st)))
        return np.frombuffer(b"".join(recs), dtype=CONTIG_REC), b"".join(seq), st

    def bubbles(self, max_allele=2000, max_flank=500, haploid=(), keep_serial=False, stats=None):
        """`bubbles` (ctx_bubbles.c without link files): the calls of every fork of the multi-colour graph, forks in ascending
        key order.  haploid: colours that hold one allele only; keep_serial: skip the serial-bubble filter (-S).  stats: a
        BubblesStats that the call adds to.  Returns (records as a BUBBLE_REC array, the text of the calls as bytes)."""
        hap = np.ascontiguousarray(list(haploid), dtype=np.uint32)
        recs, text = [], []

        def rec_sink(_ctx, ptr, n):
            recs.append(C.string_at(ptr, n))
            return 0

        def text_sink(_ctx, ptr, n):
            text.append(C.string_at(ptr, n))
            return 0

        st = stats if stats is not None else BubblesStats()
        prm = BubblesParams(int(max_allele), int(max_flank), BUBBLES_KEEP_SERIAL if keep_serial else 0, len(hap),
                            hap.ctypes.data_as(C.c_void_p) if len(hap) else None)
        a, b = SINK_FN(rec_sink), SINK_FN(text_sink)
        _check(self.L.mcx_graph_bubbles(self.h, C.byref(prm), a, None, b, None, C.byref(st)))
        return np.frombuffer(b"".join(recs), dtype=BUBBLE_REC), b"".join(text)

    def breakpoints(self, ref_seqs, names, min_ref=5, max_ref=1000, ref_edges=True, ref_loaded=False, stats=None, load_only=False):
        """`breakpoints` (ctx_breakpoints.c without link files): where the samples differ from the reference genome `ref_seqs`
        (a list of str or bytes; `names` as they print, already cleaned), which goes into the graph's last colour.  ref_edges
        False: the genome's k-mers enter without edges (-E); ref_loaded: the genome is in the graph already (a second call
        with other limits); load_only: the genome goes in and nothing else happens.  stats: a BreakpointsStats that the call adds to.  Returns (records as a BREAKPOINT_REC array,
        the text of the calls as bytes)."""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in ref_seqs]
        nms = [s.encode() if isinstance(s, str) else bytes(s) for s in names]
        if len(seqs) != len(nms):
            raise ValueError("a name per reference sequence")
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        noff = np.zeros(len(nms) + 1, dtype=np.uint64)
        noff[1:] = np.cumsum([len(s) for s in nms])
        bases = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
        nbuf = np.frombuffer(b"".join(nms) + b"\0", dtype=np.uint8)
        recs, text = [], []

        def rec_sink(_ctx, ptr, n):
            recs.append(C.string_at(ptr, n))
            return 0

        def text_sink(_ctx, ptr, n):
            text.append(C.string_at(ptr, n))
            return 0

        st = stats if stats is not None else BreakpointsStats()
        prm = BreakpointsParams(int(min_ref), int(max_ref), (0 if ref_edges else BREAKPOINTS_NO_REF_EDGES) | (BREAKPOINTS_REF_LOADED if ref_loaded else 0)
                                | (BREAKPOINTS_LOAD_ONLY if load_only else 0))
        a, b = SINK_FN(rec_sink), SINK_FN(text_sink)
        _check(self.L.mcx_graph_breakpoints(self.h, _ptr(bases), _ptr(offs), len(seqs), _ptr(nbuf), _ptr(noff), C.byref(prm), a, None, b, None, C.byref(st)))
        return np.frombuffer(b"".join(recs), dtype=BREAKPOINT_REC), b"".join(text)

    def subgraph(self, seeds, dist=0, invert=False, unitigs=False):
        """`subgraph` (ctx_subgraph.c): keep the k-mers within `dist` edges of the k-mers of `seeds` (a list of str or
        bytes); with `unitigs` the seeds' whole unitigs count as seeds, with `invert` the complement is kept.
        Returns the stats dict (num_seed_kmers, num_seed_found, nkmers_before, nkmers_kept, nkmers_removed, levels,
        narrow_launches, max_frontier)"""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seeds]
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        self.subgraph_begin(unitigs)
        if seqs:
            self.subgraph_seed(np.frombuffer(b"".join(seqs) or b"\n", dtype=np.uint8), offs)
        return self.subgraph_finish(dist, invert, unitigs)

    def unitigs_chunks(self, format="fasta", points=False, stats=None):
        """`unitigs`: yields the text in consecutive chunks (the whole text is produced on the first step; `stats`,
        a dict, receives num_unitigs, num_kmers, num_bytes, num_cycles)"""
        if format not in UNITIGS_FORMATS:
            raise ValueError("unitigs format: one of %s" % ", ".join(sorted(UNITIGS_FORMATS)))
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n))
            return 0

        st = UnitigsStats()
        _check(self.L.mcx_graph_unitigs(self.h, UNITIGS_FORMATS[format], UNITIGS_POINTS if points else 0, SINK_FN(sink), None,
                                        C.byref(st)))
        if stats is not None:
            stats.update(st.as_dict())
        yield from parts

    def unitigs(self, format="fasta", points=False, stats=None):
        """`unitigs` (ctx_unitigs.c): every unitig of the graph as FASTA, GFA or DOT text, written on the device;
        normalised, numbered by the key of the first k-mer (include/mcx_gpu.h states the contract)"""
        return b"".join(self.unitigs_chunks(format, points, stats))

    def unitigs_dev(self):
        """mcx_graph_unitigs_dev into torch tensors on the graph's device: (dict of keys[n,W] (int64 bit patterns),
        unitig[n], rank[n], orient[n], first[u], length[u], stats dict)"""
        import torch
        n = max(self.nkmers, 1)
        dev = "cuda:%d" % self.device
        t = {"keys": torch.zeros((n, self.W), dtype=torch.int64, device=dev), "unitig": torch.zeros(n, dtype=torch.int32, device=dev),
             "rank": torch.zeros(n, dtype=torch.int32, device=dev), "orient": torch.zeros(n, dtype=torch.uint8, device=dev),
             "first": torch.zeros(n, dtype=torch.int32, device=dev), "length": torch.zeros(n, dtype=torch.int32, device=dev)}
        arr = UnitigsArrays(*[t[name].data_ptr() for name, _ in UnitigsArrays._fields_])
        st = UnitigsStats()
        torch.cuda.synchronize(self.device)
        _check(self.L.mcx_graph_unitigs_dev(self.h, C.byref(arr), C.byref(st)))
        nk, nu = int(st.num_kmers), int(st.num_unitigs)
        out = {name: (v[:nu] if name in ("first", "length") else v[:nk]) for name, v in t.items()}
        return out, st.as_dict()

    def export(self, sorted_=True):
        """Records in .ctx body layout as one bytes object."""
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n))
            return 0

        cb = SINK_FN(sink)
        _check(self.L.mcx_graph_export(self.h, 1 if sorted_ else 0, cb, None))
        return b"".join(parts)

    def records(self, sorted_=True):
        """(keys[n,W] u64, covg[n,ncols] u32, edges[n,ncols] u8)."""
        body = self.export(sorted_)
        rs = 8 * self.W + 5 * self.ncols
        rec = np.frombuffer(body, dtype=np.uint8).reshape(-1, rs)
        keys = rec[:, :8 * self.W].copy().view(np.uint64).reshape(-1, self.W)
        cov = rec[:, 8 * self.W:8 * self.W + 4 * self.ncols].copy().view(np.uint32).reshape(-1, self.ncols)
        edg = rec[:, 8 * self.W + 4 * self.ncols:].copy()
        return keys, cov, edg


def sort_records(recs, kmer_size, ncols, device=0):
    """sort .ctx body bytes by k-mer on the device; returns the sorted bytes"""
    a = np.frombuffer(bytes(recs), dtype=np.uint8).copy()
    rs = 8 * _words(kmer_size) + 5 * ncols
    assert a.size % rs == 0
    _check(lib().mcx_sort_records(_ptr(a), a.size // rs, kmer_size, ncols, device))
    return a.tobytes()


JOIN_KEEP_EMPTY = 1


class Join:
    """`join` on the device: .ctx records of several files merged by a sort and a segmented reduce (no table)."""

    def __init__(self, kmer_size, out_ncols, n_isec=0, keep_empty=False, device=0):
        self.L = lib()
        self.h = None
        self.k, self.W, self.ncols = kmer_size, _words(kmer_size), out_ncols
        h = C.c_void_p()
        _check(self.L.mcx_join_create(C.byref(h), kmer_size, out_ncols, n_isec, JOIN_KEEP_EMPTY if keep_empty else 0, device))
        self.h = h

    def close(self):
        if self.h:
            self.L.mcx_join_destroy(self.h)
            self.h = None

    __del__ = close

    def configure(self, key, value):
        _check(self.L.mcx_join_configure(self.h, key.encode(), int(value)))

    def add(self, recs, file_ncols, colour_filter, source=-1):
        """recs: .ctx body bytes of a file with file_ncols colours; colour_filter: [(from, into)]; source -1 = an
        input graph, r >= 0 = the intersection graph of rank r (only the `from` side of its filter counts)"""
        recs = np.frombuffer(recs, dtype=np.uint8) if isinstance(recs, (bytes, bytearray, memoryview)) else np.ascontiguousarray(recs, dtype=np.uint8)
        rs = 8 * self.W + 5 * file_ncols
        assert recs.size % rs == 0
        frm = np.array([f for f, _ in colour_filter], dtype=np.int32)
        into = np.array([t for _, t in colour_filter], dtype=np.int32)
        _check(self.L.mcx_join_add_records(self.h, source, _ptr(recs), recs.size // rs, file_ncols, _ptr(frm), _ptr(into), len(frm)))

    def phases(self):
        """host-clock ms so far: upload + key extraction, sort, runs + intersection, reduce + write-out"""
        ms = (C.c_double * 4)()
        _check(self.L.mcx_join_phases(self.h, ms))
        return dict(zip(("upload_extract_ms", "sort_ms", "runs_isec_ms", "reduce_write_ms"), [float(x) for x in ms]))

    def finish(self, keep=True):
        """-> (body bytes in ascending key order, stats dict); keep=False drops the bytes (benchmarks)"""
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n) if keep else n)
            return 0

        st = JoinStats()
        _check(self.L.mcx_join_finish(self.h, SINK_FN(sink), None, C.byref(st)))
        self.chunks = [len(p) if keep else p for p in parts]
        return (b"".join(parts) if keep else b""), st.as_dict()


LINKS_CLEAN, LINKS_HIST = 1, 2
LINKS_REFUSALS = {1: "bad_kmer_line", 2: "bad_orient", 3: "bad_number", 4: "multi_colour", 5: "bad_junction", 6: "njuncs_range",
                  7: "njuncs_length", 8: "no_seq", 9: "no_juncpos", 10: "juncpos_count", 11: "seq_length", 12: "seq_base",
                  13: "link_before_kmer", 14: "count_columns"}


class Links:
    """`links` on the device: the body of a version-4 .ctp file cleaned, listed and counted (no graph, no table)."""

    def __init__(self, kmer_size, device=0):
        self.L = lib()
        self.h = None
        self.k = kmer_size
        self.hist_shape = None
        h = C.c_void_p()
        _check(self.L.mcx_links_create(C.byref(h), kmer_size, device))
        self.h = h

    def close(self):
        if self.h:
            self.L.mcx_links_destroy(self.h)
            self.h = None

    __del__ = close

    def configure(self, key, value):
        _check(self.L.mcx_links_configure(self.h, key.encode(), int(value)))

    def add(self, text, clean=None, hist=None, max_kmers=0, ctp=True, rows=True):
        """text: whole k-mer blocks of a .ctp body; clean: the cut-off or None; hist: (distsize, covgsize) or None;
        -> (.ctp bytes, list bytes).  ctp / rows = False: that text is not made (benchmarks)"""
        text = bytes(text)
        p = LinksParams()
        p.flags = (LINKS_CLEAN if clean is not None else 0) | (LINKS_HIST if hist is not None else 0)
        p.cutoff = int(clean) if clean is not None else 0
        if hist is not None:
            p.distsize, p.covgsize = int(hist[0]), int(hist[1])
        p.max_kmers = int(max_kmers)
        out, lst = [], []

        def sink_to(parts):
            def sink(_ctx, ptr, n):
                parts.append(C.string_at(ptr, n))
                return 0
            return SINK_FN(sink)

        none = C.cast(None, SINK_FN)
        a, b = sink_to(out), sink_to(lst)
        _check(self.L.mcx_links_add_text(self.h, text, len(text), C.byref(p), a if ctp else none, None, b if rows else none, None))
        if hist is not None:
            self.hist_shape = (int(hist[0]), int(hist[1]))
        self.chunks = [len(x) for x in out], [len(x) for x in lst]
        return b"".join(out), b"".join(lst)

    def stats(self):
        st = LinksStats()
        _check(self.L.mcx_links_get_stats(self.h, C.byref(st)))
        return st.as_dict()

    def hist(self):
        """the distsize x covgsize counters so far"""
        a = np.zeros(self.hist_shape, dtype=np.uint64)
        _check(self.L.mcx_links_hist(self.h, a.ctypes.data_as(C.POINTER(C.c_uint64))))
        return a

    def error(self):
        """after an McxError of code MCX_ERR_INVAL: (refusal name, byte offset of the first bad line in the text)"""
        code, off = C.c_int(0), C.c_uint64(0)
        _check(self.L.mcx_links_error(self.h, C.byref(code), C.byref(off)))
        return LINKS_REFUSALS.get(code.value, code.value), int(off.value)

    def phases(self):
        ms = (C.c_double * 8)()
        _check(self.L.mcx_links_phases(self.h, ms))
        return dict(zip(("upload_ms", "lines_ms", "parse_ms", "sort_ms", "reduce_lcp_ms", "tree_ms", "written_ms", "text_ms"), [float(x) for x in ms]))


class Pjoin:
    """`pjoin` on the device: the bodies of version-4 .ctp files merged by a sort and a segmented reduce of per-colour
    counts (no graph, no table)."""

    def __init__(self, kmer_size, out_ncols, device=0):
        self.L = lib()
        self.h = None
        self.k, self.ncols = kmer_size, out_ncols
        h = C.c_void_p()
        _check(self.L.mcx_pjoin_create(C.byref(h), kmer_size, out_ncols, device))
        self.h = h

    def close(self):
        if self.h:
            self.L.mcx_pjoin_destroy(self.h)
            self.h = None

    __del__ = close

    def configure(self, key, value):
        _check(self.L.mcx_pjoin_configure(self.h, key.encode(), int(value)))

    def add(self, text, src_ncols=1, filter=None):
        """text: lines of the body of a file with src_ncols colours; filter: [(from, into)], None = colour c into
        colour c; -> the piece's line counts as a dict"""
        text = bytes(text)
        pairs = [(c, c) for c in range(src_ncols)] if filter is None else list(filter)
        flt = np.array(pairs, dtype=np.int32).reshape(-1, 2)
        ps = PjoinPieceStats()
        _check(self.L.mcx_pjoin_add_text(self.h, text, len(text), src_ncols, _ptr(flt) if len(flt) else None, len(flt), C.byref(ps)))
        return ps.as_dict()

    def finish(self, keep=True):
        """-> the merged body as bytes (k-mers in ascending text order); keep=False drops the bytes (benchmarks)"""
        parts = []

        def sink(_ctx, ptr, n):
            parts.append(C.string_at(ptr, n) if keep else n)
            return 0

        st = PjoinStats()
        _check(self.L.mcx_pjoin_finish(self.h, SINK_FN(sink), None, C.byref(st)))
        self.chunks = [len(p) if keep else p for p in parts]
        return b"".join(parts) if keep else b""

    def stats(self):
        st = PjoinStats()
        _check(self.L.mcx_pjoin_get_stats(self.h, C.byref(st)))
        return st.as_dict()

    def error(self):
        """after an McxError of code MCX_ERR_INVAL: (refusal name, byte offset of the first bad line in the text)"""
        code, off = C.c_int(0), C.c_uint64(0)
        _check(self.L.mcx_pjoin_error(self.h, C.byref(code), C.byref(off)))
        return LINKS_REFUSALS.get(code.value, code.value), int(off.value)

    def phases(self):
        ms = (C.c_double * 6)()
        _check(self.L.mcx_pjoin_phases(self.h, ms))
        return dict(zip(("upload_ms", "lines_ms", "parse_store_ms", "sort_ms", "reduce_ms", "text_ms"), [float(x) for x in ms]))


def records_sorted(recs, kmer_size, ncols, device=0):
    """index of the first record that is not greater than its predecessor, or -1"""
    a = np.frombuffer(bytes(recs), dtype=np.uint8)
    rs = 8 * _words(kmer_size) + 5 * ncols
    bad = C.c_int64(-1)
    _check(lib().mcx_records_sorted(_ptr(a), a.size // rs, kmer_size, ncols, device, C.byref(bad)))
    return int(bad.value)


def superk_supported(kmer_size):
    return bool(lib().mcx_superk_supported(kmer_size))


def multi_exchange_bytes(kmer_size, ndevices, capacity_kmers):
    """HBM per device that the exchange buffers of an N-device table take (mcx_multi_exchange_bytes; no GPU needed)"""
    out = C.c_uint64(0)
    L = lib()
    L.mcx_multi_exchange_bytes.argtypes = [C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
    rc = L.mcx_multi_exchange_bytes(kmer_size, ndevices, capacity_kmers, C.byref(out))
    if rc != 0:
        raise McxError(rc, L.mcx_last_error().decode())
    return int(out.value)


def superk_record_words(kmer_size):
    """64-bit words per super-k-mer record (2 for one-word keys, 4 for two-word keys)"""
    return int(lib().mcx_superk_record_bytes(kmer_size)) // 8


def superk_owner(words, kmer_size, nparts):
    a = (C.c_uint64 * 2)(*(list(words) + [0])[:2])
    return int(lib().mcx_superk_owner(a, kmer_size, nparts))


def pack_stream_dev(d_stream, nbytes, d_code, d_inv, hip_stream=None):
    """ASCII stream in HBM -> packed form (d_code: int32 [(nbytes + 15) // 16], d_inv: int16 likewise)"""
    _check(lib().mcx_pack_stream_dev(_ptr(d_stream), int(nbytes), _ptr(d_code), _ptr(d_inv), C.c_void_p(hip_stream) if hip_stream else None))


def ubench_stream(nbytes=8 << 30, device=0):
    """measured streaming ceilings of the device in GB/s: {"copy", "read", "write"} (mcx_ubench_stream)"""
    c, r, w = C.c_double(0), C.c_double(0), C.c_double(0)
    _check(lib().mcx_ubench_stream(device, C.c_uint64(nbytes), C.byref(c), C.byref(r), C.byref(w)))
    return {"copy": c.value, "read": r.value, "write": w.value}


def ubench_random_rmw(table_bytes=16 << 30, nupdates=1 << 29, device=0):
    """measured random 64-byte-sector rates per second over a working set of `table_bytes`:
    {"rmw" (agent-scope atomic), "load16", "load_rmw"} (mcx_ubench_random_rmw)"""
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    _check(lib().mcx_ubench_random_rmw(device, C.c_uint64(table_bytes), C.c_uint64(nupdates), C.byref(a), C.byref(b), C.byref(c)))
    return {"rmw": a.value, "load16": b.value, "load_rmw": c.value}


def records_checksum(recs, kmer_size, ncols):
    if isinstance(recs, np.ndarray) and recs.dtype == np.uint8 and recs.flags.c_contiguous:
        a = recs  # (no copy: bodies of hundreds of millions of records)
    else:
        a = np.frombuffer(bytes(recs), dtype=np.uint8)
    rs = 8 * _words(kmer_size) + 5 * ncols
    assert a.size % rs == 0
    return int(lib().mcx_records_checksum(_ptr(a), a.size // rs, kmer_size, ncols))
