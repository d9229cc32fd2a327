"""ctypes binding of the C ABI in include/whatshap_amd.h.

This is the *only* place the shared library is loaded.  There is no CPU fallback: if
``libwhatshap_amd.so`` has not been built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C whatshap_amd/csrc``) importing this module raises, and creating a table on a machine
without a HIP device raises ``RuntimeError`` from the library's own message.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwhatshap_amd.so")
DEBUG_LIB_PATH = os.path.join(_HERE, "libwhatshap_amd_debug.so")   # test infrastructure (debug_lib)
ABI_VERSION = 4   # WHAMD_ABI_VERSION of include/whatshap_amd.h this file mirrors (struct layouts below)

WHAMD_OK = 0
WHAMD_ERR_INVALID = 1
WHAMD_ERR_MENDELIAN_CONFLICT = 2
WHAMD_ERR_UNSORTED = 3
WHAMD_ERR_UNSUPPORTED = 4
WHAMD_ERR_DEVICE = 5
WHAMD_ERR_OVERFLOW = 6
WHAMD_ERR_HOST = 7
GT_OTHER = 255


class Record(C.Structure):
    """A struct the library fills (statistics, a plan's summary), readable as a dict."""

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class ReadSetView(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint32),
        ("read_ptr", C.POINTER(C.c_uint64)),
        ("var_position", C.POINTER(C.c_int32)),
        ("var_allele", C.POINTER(C.c_uint8)),
        ("var_quality", C.POINTER(C.c_uint32)),
        ("read_sample_id", C.POINTER(C.c_int32)),
    ]


class PedigreeView(C.Structure):
    _fields_ = [
        ("n_individuals", C.c_uint32),
        ("individual_id", C.POINTER(C.c_uint32)),
        ("n_triples", C.c_uint32),
        ("triple_ids", C.POINTER(C.c_uint32)),
        ("n_variants", C.c_uint32),
        ("genotype", C.POINTER(C.c_uint8)),
        ("genotype_likelihoods", C.POINTER(C.c_double)),
        ("gl_present", C.POINTER(C.c_uint8)),
    ]


class PlanSummary(Record):
    _fields_ = [(name, C.c_uint64) for name in (
        "n_columns", "n_steps", "n_runs", "n_resident_columns", "n_folded_columns", "n_vectorised_columns",
        "max_run_columns", "max_workgroups", "max_lds_bytes", "backtrace_bytes", "n_components", "n_halved_runs")] + [
        ("max_coverage", C.c_uint32), ("invariants_ok", C.c_uint32), ("n_yform_runs", C.c_uint64), ("n_fact_runs", C.c_uint64)]


class SolveStats(Record):
    _fields_ = [
        ("n_columns", C.c_uint64),
        ("n_cells", C.c_uint64),
        ("n_costs", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64),
        ("forward_launches", C.c_uint64),
        ("forward_ms", C.c_double),
        ("backtrace_ms", C.c_double),
        ("total_ms", C.c_double),
        ("host_prepare_ms", C.c_double),
        ("host_finish_ms", C.c_double),
        ("max_coverage", C.c_uint32),
        ("transmissions", C.c_uint32),
        ("bt_chunks", C.c_uint32),
        ("bt_missed", C.c_uint32),
        ("bt_rewalked", C.c_uint32),
        ("group_tables", C.c_uint32),
        ("host_flatten_ms", C.c_double),
    ]


class GenotypeStats(Record):
    _fields_ = [
        ("n_columns", C.c_uint64),
        ("n_cells", C.c_uint64),
        ("launches", C.c_uint64),
        ("backward_ms", C.c_double),
        ("forward_ms", C.c_double),
        ("total_ms", C.c_double),
        ("host_prepare_ms", C.c_double),
        ("window", C.c_uint32),
        ("max_coverage", C.c_uint32),
        ("transmissions", C.c_uint32),
        ("slot_runs", C.c_uint32),
    ]


class HeuristicStats(Record):
    _fields_ = [
        ("n_columns", C.c_uint64),
        ("n_reads", C.c_uint64),
        ("max_solutions", C.c_uint64),
        ("total_solutions", C.c_uint64),
        ("device_ms", C.c_double),
        ("host_prepare_ms", C.c_double),
        ("host_finish_ms", C.c_double),
        ("n_samples", C.c_uint32),
        ("row_limit", C.c_uint32),
    ]


class HeuristicJob(C.Structure):
    _fields_ = [("readset", C.POINTER(ReadSetView)), ("recombcost", C.POINTER(C.c_uint32)), ("n_recombcost", C.c_size_t),
                ("pedigree", C.POINTER(PedigreeView)), ("distrust_genotypes", C.c_int), ("positions", C.POINTER(C.c_uint32)),
                ("n_positions", C.c_size_t), ("row_limit", C.c_uint32), ("allow_mutations", C.c_int)]


class RealignAlignmentsView(C.Structure):
    _fields_ = [("n_alignments", C.c_uint64), ("reference_start", C.POINTER(C.c_int64)), ("first_variant", C.POINTER(C.c_uint64)),
                ("cigar_ptr", C.POINTER(C.c_uint64)), ("cigar_op", C.POINTER(C.c_uint32)), ("cigar_len", C.POINTER(C.c_uint32)),
                ("seq_ptr", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint8)), ("seq_present", C.POINTER(C.c_uint8))]


class RealignVariantsView(C.Structure):
    _fields_ = [("n_variants", C.c_uint64), ("position", C.POINTER(C.c_int64)), ("ref_ptr", C.POINTER(C.c_uint64)), ("ref_bytes", C.POINTER(C.c_uint8)),
                ("alt_ptr", C.POINTER(C.c_uint64)), ("alt_byte_ptr", C.POINTER(C.c_uint64)), ("alt_bytes", C.POINTER(C.c_uint8)),
                ("restrict_ptr", C.POINTER(C.c_uint64)), ("restrict_alleles", C.POINTER(C.c_int64)), ("restrict_present", C.POINTER(C.c_uint8))]


class RealignReferenceView(C.Structure):
    _fields_ = [("bytes", C.POINTER(C.c_uint8)), ("offset", C.c_uint64), ("length", C.c_uint64), ("chromosome_length", C.c_uint64)]


class RealignParams(C.Structure):
    _fields_ = [("overhang", C.c_int64), ("use_affine", C.c_int32), ("gap_start", C.c_int32), ("gap_extend", C.c_int32), ("default_mismatch", C.c_float),
                ("affine_unset", C.c_int32)]


class RealignStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_alignments", "n_jobs", "n_pairs", "n_results")] + [
        (name, C.c_double) for name in ("host_walk_ms", "upload_ms", "kernel_ms", "download_ms", "host_finish_ms", "total_ms")]


class DebugRealignShape(Record):
    """whamd_debug_realign_shape (include/whatshap_amd_debug.h): the launch of realign's long jobs."""
    _fields_ = [("blocks", C.c_uint32), ("block", C.c_uint32), ("lds_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64), ("carry_words", C.c_uint32),
                ("row_floats", C.c_uint32), ("global_rows", C.c_int32), ("reserved", C.c_int32)]


class PolyMatrixView(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("read_ptr", C.POINTER(C.c_uint64)), ("position", C.POINTER(C.c_int64)), ("allele", C.POINTER(C.c_int8))]


class PolyScoreStats(Record):
    _fields_ = [("err", C.c_double)] + [(name, C.c_uint64) for name in ("n_reads", "n_positions", "n_candidates", "n_overlapping", "n_entries", "n_nan", "n_pair_positions")] + [
        ("launches", C.c_uint32)] + [(name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class ProgenyView(C.Structure):
    _fields_ = [("gl", C.POINTER(C.c_float)), ("n_positions", C.c_uint64), ("n_samples", C.c_uint32), ("ploidy", C.c_uint32), ("n_nodes", C.c_uint64),
                ("node_variant", C.POINTER(C.c_uint32)), ("n_variants", C.c_uint64), ("alt_count", C.POINTER(C.c_uint32)),
                ("co_alt_count", C.POINTER(C.c_uint32)), ("scoring_window", C.c_uint32)]


class ProgenyDepthsView(C.Structure):
    _fields_ = [("ref_depth", C.POINTER(C.c_uint32)), ("alt_depth", C.POINTER(C.c_uint32)), ("n_rows", C.c_uint64), ("n_samples", C.c_uint32),
                ("ploidy", C.c_uint32), ("error_rate", C.c_double), ("row_alt_count", C.POINTER(C.c_uint32)), ("row_co_alt_count", C.POINTER(C.c_uint32)),
                ("n_nodes", C.c_uint64), ("node_row", C.POINTER(C.c_uint32)), ("priors", C.POINTER(C.c_double)), ("scoring_window", C.c_uint32),
                ("node_variant", C.POINTER(C.c_uint32)), ("n_variants", C.c_uint64), ("alt_count", C.POINTER(C.c_uint32)),
                ("co_alt_count", C.POINTER(C.c_uint32))]


class ProgenyScoreStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_nodes", "n_entries", "n_inf", "n_reused", "n_sample_terms")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class HaplotagView(C.Structure):
    _fields_ = [("ploidy", C.c_uint32), ("linked_reads", C.c_uint32), ("linked_read_cutoff", C.c_int64), ("n_variants", C.c_uint64),
                ("variant_position", C.POINTER(C.c_int64)), ("variant_phaseset", C.POINTER(C.c_int64)), ("variant_phasing", C.POINTER(C.c_int8)),
                ("n_reads", C.c_uint64), ("read_ptr", C.POINTER(C.c_uint64)), ("entry_position", C.POINTER(C.c_int64)), ("entry_allele", C.POINTER(C.c_int8)),
                ("entry_quality", C.POINTER(C.c_int32)), ("read_start", C.POINTER(C.c_int64)), ("read_repr", C.POINTER(C.c_uint32)),
                ("read_bx", C.POINTER(C.c_uint32))]


class HaplotagStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_groups", "n_assigned", "n_multiple_phase_sets", "n_entries", "groups_class_a", "groups_class_b",
                                                "groups_class_c", "groups_many_phase_sets")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class TagphaseView(C.Structure):
    _fields_ = [("n_variants", C.c_uint64), ("variant_flags", C.POINTER(C.c_uint8)), ("n_reads", C.c_uint64), ("read_ptr", C.POINTER(C.c_uint64)),
                ("entry_variant", C.POINTER(C.c_uint32)), ("entry_id", C.POINTER(C.c_uint8)), ("entry_quality", C.POINTER(C.c_int32)),
                ("read_ps", C.POINTER(C.c_int64)), ("read_hp", C.POINTER(C.c_int32)), ("gap_threshold", C.c_double), ("only_indels", C.c_uint32),
                ("want_table", C.c_uint32)]


class TagphaseStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_variants", "n_entries", "n_voting", "n_skipped", "n_voted", "n_kept", "n_zero_total",
                                                "variants_class_a", "variants_class_b", "variants_class_c", "variants_many_phase_sets", "table_rows")] + [
        ("launches", C.c_uint32)] + [(name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class PriorGenotypesView(C.Structure):
    _fields_ = [("n_positions", C.c_uint64), ("positions", C.POINTER(C.c_uint32)), ("n_reads", C.c_uint64), ("read_ptr", C.POINTER(C.c_uint64)),
                ("entry_position", C.POINTER(C.c_uint32)), ("entry_allele", C.POINTER(C.c_uint8)), ("entry_quality", C.POINTER(C.c_uint32)),
                ("constant", C.c_double), ("gt_prob", C.c_double), ("want_regularized", C.c_uint32), ("reserved", C.c_uint32)]


class PriorGenotypesStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_positions", "n_entries", "n_counted", "n_covered", "n_genotyped", "columns_class_a",
                                                "columns_class_b", "columns_class_c", "longest_run")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("map_ms", "host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


PRIOR_GENOTYPES_LAUNCHES = 8   # WHAMD_PRIOR_GENOTYPES_LAUNCHES of include/whatshap_amd.h


class PolyReorderView(C.Structure):
    _fields_ = [("matrix", PolyMatrixView), ("ploidy", C.c_uint32), ("reserved", C.c_uint32), ("n_pos", C.c_uint64), ("haplotypes", C.POINTER(C.c_int8)),
                ("threads", C.POINTER(C.c_int32)), ("n_clusters", C.c_uint64), ("cluster_ptr", C.POINTER(C.c_uint64)), ("cluster_reads", C.POINTER(C.c_uint32)),
                ("n_breakpoints", C.c_uint64), ("bp_position", C.POINTER(C.c_uint64)), ("bp_affected_ptr", C.POINTER(C.c_uint64)),
                ("bp_affected", C.POINTER(C.c_uint32)), ("bp_cluster_ptr", C.POINTER(C.c_uint64)), ("bp_clusters", C.POINTER(C.c_uint32))]


class PolyReorderStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_breakpoints", "n_reads_visited", "n_permutations", "n_window_positions")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class PolyCompareView(C.Structure):
    _fields_ = [("ploidy", C.c_uint32), ("matched_only", C.c_uint32), ("n_pos", C.c_uint64), ("phasing0", C.POINTER(C.c_uint8)),
                ("phasing1", C.POINTER(C.c_uint8)), ("switch_cost", C.c_double), ("flip_cost", C.c_double), ("want_path", C.c_uint32), ("reserved", C.c_uint32)]


class PolyCompareJobResult(C.Structure):
    _fields_ = [("total", C.c_double), ("n_matched", C.c_uint64), ("n_visited", C.c_uint64), ("min_hamming_sum", C.c_uint64), ("switches", C.c_uint32),
                ("flips", C.c_uint32)]


class PolyCompareStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_jobs", "n_positions", "n_visited", "path_bytes")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class PolyThreadView(C.Structure):
    _fields_ = [("matrix", PolyMatrixView), ("n_clusters", C.c_uint64), ("cluster_ptr", C.POINTER(C.c_uint64)), ("cluster_reads", C.POINTER(C.c_uint32)),
                ("ploidy", C.c_uint32), ("max_cluster_gap", C.c_uint32), ("n_alleles", C.c_uint32), ("flags", C.c_uint32)]


class PolyThreadStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_positions", "n_entries", "n_counted", "n_rows", "n_selected", "n_readded", "n_emptied",
                                                "positions_class_a", "positions_class_b", "positions_class_c")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "fill_ms", "total_ms")]


class PolyThreaderView(C.Structure):
    _fields_ = [("n_positions", C.c_uint64), ("cov_ptr", C.POINTER(C.c_uint64)), ("cov_cluster", C.POINTER(C.c_uint32)), ("pc_ptr", C.POINTER(C.c_uint64)),
                ("pc_cluster", C.POINTER(C.c_uint32)), ("pc_total", C.POINTER(C.c_uint32)), ("n_block_starts", C.c_uint64), ("block_starts", C.POINTER(C.c_uint64)),
                ("switch_cost", C.c_double), ("affine_switch_cost", C.c_double), ("ploidy", C.c_uint32), ("max_cluster_gap", C.c_uint32),
                ("row_limit", C.c_uint32), ("flags", C.c_uint32)]


class PolyThreaderStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_positions", "n_sections", "n_tuples", "n_entries")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "download_ms", "total_ms")]


class ReadmergeView(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("read_ptr", C.POINTER(C.c_uint64)), ("entry_position", C.POINTER(C.c_int64)), ("entry_allele", C.POINTER(C.c_uint8)),
                ("entry_quality", C.POINTER(C.c_int64)), ("representative", C.POINTER(C.c_uint32)), ("thr_diff", C.c_int64), ("thr_neg_diff", C.c_int64),
                ("max_error_rate", C.c_double), ("want_edges", C.c_uint32), ("reserved", C.c_uint32)]


class ReadmergeStats(Record):
    _fields_ = [(name, C.c_uint64) for name in ("n_reads", "n_entries", "n_pairs", "n_blue", "n_not_blue", "n_merged_components", "n_merged_entries",
                                                "n_super_entries")] + [("launches", C.c_uint32)] + [
        (name, C.c_double) for name in ("host_ms", "upload_ms", "kernel_ms", "pair_kernel_ms", "download_ms", "components_ms", "total_ms")]


READMERGE_LAUNCHES = 9          # WHAMD_READMERGE_LAUNCHES of include/whatshap_amd.h
POLY_THREAD_LAUNCHES = 13       # WHAMD_POLY_THREAD_LAUNCHES of include/whatshap_amd.h
POLY_THREAD_MAX_PLOIDY = 16     # WHAMD_POLY_THREAD_MAX_PLOIDY
POLY_THREAD_MAX_ALLELES = 16    # WHAMD_POLY_THREAD_MAX_ALLELES
POLY_THREAD_DEPTHS_ONLY = 1     # WHAMD_POLY_THREAD_DEPTHS_ONLY
POLY_THREADER_LAUNCHES = 5      # WHAMD_POLY_THREADER_LAUNCHES
POLY_THREADER_MIN_PLOIDY = 2    # WHAMD_POLY_THREADER_MIN_PLOIDY
POLY_THREADER_MAX_PLOIDY = 6    # WHAMD_POLY_THREADER_MAX_PLOIDY
POLY_THREADER_MAX_CLUSTERS = 8  # WHAMD_POLY_THREADER_MAX_CLUSTERS
POLY_THREADER_WANT_COSTS = 1    # WHAMD_POLY_THREADER_WANT_COSTS


def _ptr(arr: Optional[np.ndarray], ctype):
    if arr is None:
        return C.cast(None, C.POINTER(ctype))
    return arr.ctypes.data_as(C.POINTER(ctype))


class ProblemArrays:
    """Owns the numpy arrays behind a (readset view, pedigree view, recombcost, positions) tuple.

    The same object feeds the product library, the oracle restatement and the compiled reference
    driver, so all three see byte-identical inputs.
    """

    def __init__(
        self,
        read_ptr,
        var_position,
        var_allele,
        var_quality,
        read_sample_id,
        individual_id,
        triple_ids,
        genotype,
        genotype_likelihoods,
        recombcost,
        positions,
        distrust_genotypes: bool,
        n_variants: Optional[int] = None,
    ):
        self.read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
        if self.read_ptr.size == 0:
            self.read_ptr = np.zeros(1, dtype=np.uint64)
        self.var_position = np.ascontiguousarray(var_position, dtype=np.int32)
        self.var_allele = np.ascontiguousarray(var_allele, dtype=np.uint8)
        self.var_quality = np.ascontiguousarray(var_quality, dtype=np.uint32)
        self.read_sample_id = np.ascontiguousarray(read_sample_id, dtype=np.int32)
        self.individual_id = np.ascontiguousarray(individual_id, dtype=np.uint32)
        self.triple_ids = np.ascontiguousarray(triple_ids, dtype=np.uint32).reshape(-1)
        n_ind = self.individual_id.size
        genotype = np.ascontiguousarray(genotype, dtype=np.uint8)
        if n_variants is None:
            n_variants = genotype.size // n_ind if n_ind else 0
        self.n_variants = int(n_variants)
        self.genotype = genotype.reshape(-1)
        assert self.genotype.size == n_ind * self.n_variants
        if genotype_likelihoods is None:
            self.genotype_likelihoods = None
        else:
            self.genotype_likelihoods = np.ascontiguousarray(genotype_likelihoods, dtype=np.float64).reshape(-1)
            assert self.genotype_likelihoods.size == n_ind * self.n_variants * 3
        self.recombcost = np.ascontiguousarray(recombcost, dtype=np.uint32)
        self.positions = None if positions is None else np.ascontiguousarray(positions, dtype=np.uint32)
        self.distrust_genotypes = bool(distrust_genotypes)
        self.n_reads = self.read_sample_id.size
        assert self.read_ptr.size == self.n_reads + 1

        self.readset_view = ReadSetView(
            self.n_reads,
            _ptr(self.read_ptr, C.c_uint64),
            _ptr(self.var_position, C.c_int32),
            _ptr(self.var_allele, C.c_uint8),
            _ptr(self.var_quality, C.c_uint32),
            _ptr(self.read_sample_id, C.c_int32),
        )
        self.pedigree_view = PedigreeView(
            n_ind,
            _ptr(self.individual_id, C.c_uint32),
            self.triple_ids.size // 3,
            _ptr(self.triple_ids, C.c_uint32),
            self.n_variants,
            _ptr(self.genotype, C.c_uint8),
            _ptr(self.genotype_likelihoods, C.c_double),
            _ptr(None, C.c_uint8),
        )

    @property
    def n_individuals(self) -> int:
        return int(self.individual_id.size)

    def call_args(self):
        """(readset*, recombcost*, n_recomb, pedigree*, distrust, positions*, n_positions)"""
        return (
            C.byref(self.readset_view),
            _ptr(self.recombcost, C.c_uint32),
            C.c_size_t(self.recombcost.size),
            C.byref(self.pedigree_view),
            C.c_int(1 if self.distrust_genotypes else 0),
            _ptr(self.positions, C.c_uint32),
            C.c_size_t(0 if self.positions is None else self.positions.size),
        )


_lib = None
_debug_lib = None
_load_lock = threading.Lock()   # (the first call may come from several threads at once -- blocks.solve_blocks' create workers: ONE CDLL object per library)


def lib() -> C.CDLL:
    """Loads libwhatshap_amd.so (once).  Raises if it is missing -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C whatshap_amd/csrc). "
                "whatshap_amd has no CPU fallback."
            )
        _lib = _bind(C.CDLL(LIB_PATH), LIB_PATH)
    return _lib


def debug_lib() -> C.CDLL:
    """TEST INFRASTRUCTURE: libwhatshap_amd_debug.so -- the same sources compiled with -DWHAMD_DEBUG_BUILD: the CPU plan emulators, the
    host instantiation of the heuristic (include/whatshap_amd_debug.h), the kernel instantiations with cycle stamps and the timing switches
    (WHAMD_SLOT_STAMPS, WHAMD_SLOT_SKIP: results invalid).  None of that is in the product library.  A handle made by one library is only
    ever passed to functions of the same library."""
    global _debug_lib
    if _debug_lib is not None:
        return _debug_lib
    if not os.path.exists(DEBUG_LIB_PATH):
        raise ImportError(f"{DEBUG_LIB_PATH} is missing: make -C whatshap_amd/csrc debug (tests and timing scripts only)")
    L = _bind(C.CDLL(DEBUG_LIB_PATH), DEBUG_LIB_PATH)
    L.whamd_debug_emulate_slot_plan.restype = C.c_int
    L.whamd_debug_emulate_slot_plan.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
        C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
    ]
    L.whamd_debug_emulate_pedslot_plan.restype = C.c_int
    L.whamd_debug_emulate_pedslot_plan.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
        C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
    ]
    L.whamd_debug_pedmec_heuristic_create_host.restype = C.c_int
    L.whamd_debug_pedmec_heuristic_create_host.argtypes = [C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
                                                           C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_debug_realign_detect_host.restype = C.c_int
    L.whamd_debug_realign_detect_host.argtypes = [C.POINTER(RealignAlignmentsView), C.POINTER(RealignVariantsView), C.POINTER(RealignReferenceView),
                                                  C.POINTER(RealignParams), C.POINTER(C.c_void_p)]
    L.whamd_debug_edit_distance_host.restype = C.c_int
    L.whamd_debug_edit_distance_host.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
                                                 C.c_int, C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    L.whamd_debug_realign_long_shape.restype = C.c_int
    L.whamd_debug_realign_long_shape.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(DebugRealignShape)]
    L.whamd_debug_realign_walk_counts.restype = C.c_int
    L.whamd_debug_realign_walk_counts.argtypes = [C.POINTER(RealignAlignmentsView), C.POINTER(RealignVariantsView), C.POINTER(RealignReferenceView),
                                                  C.POINTER(RealignParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.whamd_debug_edit_distance_long_counts.restype = C.c_int
    L.whamd_debug_edit_distance_long_counts.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.whamd_debug_poly_score_host.restype = C.c_int
    L.whamd_debug_poly_score_host.argtypes = [C.POINTER(PolyMatrixView), C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(C.c_void_p)]
    L.whamd_debug_progeny_score_host.restype = C.c_int
    L.whamd_debug_progeny_score_host.argtypes = [C.POINTER(ProgenyView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_progeny_score_entries_host.restype = C.c_int
    L.whamd_debug_progeny_score_entries_host.argtypes = [C.POINTER(ProgenyView), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                         C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
    L.whamd_debug_progeny_pair_score_host.restype = C.c_int
    L.whamd_debug_progeny_pair_score_host.argtypes = [C.POINTER(C.c_float), C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                                      C.POINTER(C.c_double)]
    L.whamd_debug_progeny_variant_types_host.restype = C.c_int
    L.whamd_debug_progeny_variant_types_host.argtypes = [C.POINTER(C.c_float), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                                         C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.whamd_debug_progeny_gl_host.restype = C.c_int
    L.whamd_debug_progeny_gl_host.argtypes = [C.POINTER(ProgenyDepthsView), C.c_uint64, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_double))]
    L.whamd_debug_haplotag_host.restype = C.c_int
    L.whamd_debug_haplotag_host.argtypes = [C.POINTER(HaplotagView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_tagphase_host.restype = C.c_int
    L.whamd_debug_tagphase_host.argtypes = [C.POINTER(TagphaseView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_prior_genotypes_host.restype = C.c_int
    L.whamd_debug_prior_genotypes_host.argtypes = [C.POINTER(PriorGenotypesView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_poly_reorder_host.restype = C.c_int
    L.whamd_debug_poly_reorder_host.argtypes = [C.POINTER(PolyReorderView), C.c_uint64, C.c_double, C.c_double, C.POINTER(C.c_void_p)]
    L.whamd_debug_poly_compare_host.restype = C.c_int
    L.whamd_debug_poly_compare_host.argtypes = [C.POINTER(PolyCompareView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_poly_thread_inputs_host.restype = C.c_int
    L.whamd_debug_poly_thread_inputs_host.argtypes = [C.POINTER(PolyThreadView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_poly_select_clusters_host.restype = C.c_int
    L.whamd_debug_poly_select_clusters_host.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    L.whamd_debug_poly_haplotypes_host.restype = C.c_int
    L.whamd_debug_poly_haplotypes_host.argtypes = [C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int8),
                                                   C.POINTER(C.c_int8)]
    L.whamd_debug_poly_threader_host.restype = C.c_int
    L.whamd_debug_poly_threader_host.argtypes = [C.POINTER(PolyThreaderView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_readmerge_host.restype = C.c_int
    L.whamd_debug_readmerge_host.argtypes = [C.POINTER(ReadmergeView), C.c_uint64, C.POINTER(C.c_void_p)]
    L.whamd_debug_solve_kernels.restype = C.c_size_t
    L.whamd_debug_solve_kernels.argtypes = [C.POINTER(DebugKernel), C.c_size_t]
    L.whamd_debug_dptable_launches.restype = C.c_int
    L.whamd_debug_dptable_launches.argtypes = [C.c_void_p, C.POINTER(DebugLaunch), C.c_size_t, C.POINTER(C.c_size_t)]
    L.whamd_debug_dptable_preview.restype = C.c_int
    L.whamd_debug_dptable_preview.argtypes = [C.c_void_p, C.POINTER(DebugPreview)]
    _debug_lib = L
    return L


def use_debug_library() -> None:
    """Timing scripts (scripts/gpu_slot_stamps.py ...): every later call of this process goes through the debug build."""
    global _lib
    _lib = debug_lib()


def _bind(L: C.CDLL, path: str) -> C.CDLL:
    H = C.c_void_p
    L.whamd_abi_version.restype = C.c_int
    L.whamd_device_count.restype = C.c_int
    L.whamd_last_error.restype = C.c_char_p
    L.whamd_dptable_create.restype = C.c_int
    L.whamd_dptable_create.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
        C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.POINTER(H),
    ]
    L.whamd_dptable_create_with_options.restype = C.c_int
    L.whamd_dptable_create_with_options.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
        C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_size_t, C.c_int, C.POINTER(H),
    ]
    L.whamd_dptable_solve.restype = C.c_int
    L.whamd_dptable_solve.argtypes = [H]
    L.whamd_dptable_enqueue.restype = C.c_int
    L.whamd_dptable_enqueue.argtypes = [H]
    L.whamd_dptable_wait.restype = C.c_int
    L.whamd_dptable_wait.argtypes = [H]
    L.whamd_dptable_enqueue_many.restype = C.c_int
    L.whamd_dptable_enqueue_many.argtypes = [C.POINTER(H), C.c_size_t]
    L.whamd_dptable_wait_many.restype = C.c_int
    L.whamd_dptable_wait_many.argtypes = [C.POINTER(H), C.c_size_t]
    L.whamd_dptable_release_device.restype = C.c_int
    L.whamd_dptable_release_device.argtypes = [H]
    L.whamd_dptable_destroy.restype = None
    L.whamd_dptable_destroy.argtypes = [H]
    L.whamd_dptable_column_count.restype = C.c_uint64
    L.whamd_dptable_column_count.argtypes = [H]
    L.whamd_dptable_individual_count.restype = C.c_uint32
    L.whamd_dptable_individual_count.argtypes = [H]
    L.whamd_dptable_read_count.restype = C.c_uint32
    L.whamd_dptable_read_count.argtypes = [H]
    L.whamd_dptable_positions.restype = C.c_int
    L.whamd_dptable_positions.argtypes = [H, C.POINTER(C.c_uint32)]
    L.whamd_dptable_get_optimal_score.restype = C.c_int
    L.whamd_dptable_get_optimal_score.argtypes = [H, C.POINTER(C.c_uint32)]
    L.whamd_dptable_get_super_reads.restype = C.c_int
    L.whamd_dptable_get_super_reads.argtypes = [
        H, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
    ]
    L.whamd_dptable_get_optimal_partitioning.restype = C.c_int
    L.whamd_dptable_get_optimal_partitioning.argtypes = [H, C.POINTER(C.c_uint8)]
    L.whamd_dptable_get_index_path.restype = C.c_int
    L.whamd_dptable_get_index_path.argtypes = [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.whamd_dptable_get_stats.restype = C.c_int
    L.whamd_dptable_get_stats.argtypes = [H, C.POINTER(SolveStats)]
    L.whamd_dptable_set_option.restype = C.c_int
    L.whamd_dptable_set_option.argtypes = [H, C.c_char_p, C.c_char_p]
    L.whamd_plan_summarize.restype = C.c_int
    L.whamd_plan_summarize.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
        C.POINTER(C.c_uint32), C.c_size_t, C.c_char_p, C.POINTER(PlanSummary),
    ]
    heur_args = [C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.c_int,
                 C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.c_int]
    L.whamd_pedmec_heuristic_create.restype = C.c_int
    L.whamd_pedmec_heuristic_create.argtypes = heur_args + [C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_pedmec_heuristic_enqueue_many.restype = C.c_int
    L.whamd_pedmec_heuristic_enqueue_many.argtypes = [C.POINTER(HeuristicJob), C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_pedmec_heuristic_wait.restype = C.c_int
    L.whamd_pedmec_heuristic_wait.argtypes = [C.c_void_p]
    L.whamd_pedmec_heuristic_column_count.restype = C.c_uint64
    L.whamd_pedmec_heuristic_column_count.argtypes = [C.c_void_p]
    L.whamd_pedmec_heuristic_sample_count.restype = C.c_uint32
    L.whamd_pedmec_heuristic_sample_count.argtypes = [C.c_void_p]
    L.whamd_pedmec_heuristic_read_count.restype = C.c_uint32
    L.whamd_pedmec_heuristic_read_count.argtypes = [C.c_void_p]
    L.whamd_pedmec_heuristic_get.restype = C.c_int
    L.whamd_pedmec_heuristic_get.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int8),
                                             C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.whamd_pedmec_heuristic_get_stats.restype = C.c_int
    L.whamd_pedmec_heuristic_get_stats.argtypes = [C.c_void_p, C.POINTER(HeuristicStats)]
    L.whamd_pedmec_heuristic_destroy.restype = None
    L.whamd_pedmec_heuristic_destroy.argtypes = [C.c_void_p]
    L.whamd_read_sort_hash.restype = C.c_uint64
    L.whamd_read_sort_hash.argtypes = [C.c_char_p, C.c_int]
    L.whamd_genotype_likelihoods.restype = C.c_int
    L.whamd_genotype_likelihoods.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(PedigreeView), C.POINTER(C.c_uint32), C.c_size_t,
        C.c_int, C.c_uint32, C.POINTER(C.c_double), C.c_size_t, C.POINTER(GenotypeStats),
    ]
    L.whamd_readselection.restype = C.c_int
    L.whamd_readselection.argtypes = [
        C.POINTER(ReadSetView), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, C.c_uint32, C.c_int,
        C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
    ]
    L.whamd_realign_detect.restype = C.c_int
    L.whamd_realign_detect.argtypes = [C.POINTER(RealignAlignmentsView), C.POINTER(RealignVariantsView), C.POINTER(RealignReferenceView),
                                       C.POINTER(RealignParams), C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_realign_result_count.restype = C.c_uint64
    L.whamd_realign_result_count.argtypes = [C.c_void_p]
    L.whamd_realign_get.restype = C.c_int
    L.whamd_realign_get.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.whamd_realign_get_stats.restype = C.c_int
    L.whamd_realign_get_stats.argtypes = [C.c_void_p, C.POINTER(RealignStats)]
    L.whamd_realign_destroy.restype = None
    L.whamd_realign_destroy.argtypes = [C.c_void_p]
    L.whamd_edit_distance_batch.restype = C.c_int
    L.whamd_edit_distance_batch.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
                                            C.c_int, C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_int, C.POINTER(C.c_int64)]
    L.whamd_poly_score.restype = C.c_int
    L.whamd_poly_score.argtypes = [C.POINTER(PolyMatrixView), C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_poly_score_matrix_count.restype = C.c_uint64
    L.whamd_poly_score_matrix_count.argtypes = [C.c_void_p]
    L.whamd_poly_score_count.restype = C.c_uint64
    L.whamd_poly_score_count.argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_poly_score_get.restype = C.c_int
    L.whamd_poly_score_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.whamd_poly_score_get_stats.restype = C.c_int
    L.whamd_poly_score_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PolyScoreStats)]
    L.whamd_poly_score_destroy.restype = None
    L.whamd_poly_score_destroy.argtypes = [C.c_void_p]
    L.whamd_poly_estimate_error_rate.restype = C.c_int
    L.whamd_poly_estimate_error_rate.argtypes = [C.POINTER(PolyMatrixView), C.c_uint32, C.POINTER(C.c_double)]
    L.whamd_progeny_score.restype = C.c_int
    L.whamd_progeny_score.argtypes = [C.POINTER(ProgenyView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_progeny_score_problem_count.restype = C.c_uint64
    L.whamd_progeny_score_problem_count.argtypes = [C.c_void_p]
    L.whamd_progeny_score_count.restype = C.c_uint64
    L.whamd_progeny_score_count.argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_progeny_score_get.restype = C.c_int
    L.whamd_progeny_score_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)]
    L.whamd_progeny_score_get_stats.restype = C.c_int
    L.whamd_progeny_score_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ProgenyScoreStats)]
    L.whamd_progeny_score_destroy.restype = None
    L.whamd_progeny_score_destroy.argtypes = [C.c_void_p]
    L.whamd_progeny_variant_types.restype = C.c_int
    L.whamd_progeny_variant_types.argtypes = [C.POINTER(C.c_float), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                              C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.whamd_progeny_gl.restype = C.c_int
    L.whamd_progeny_gl.argtypes = [C.POINTER(ProgenyDepthsView), C.c_uint64, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_double))]
    L.whamd_progeny_score_depths.restype = C.c_int
    L.whamd_progeny_score_depths.argtypes = [C.POINTER(ProgenyDepthsView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_haplotag.restype = C.c_int
    L.whamd_haplotag.argtypes = [C.POINTER(HaplotagView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_haplotag_problem_count.restype = C.c_uint64
    L.whamd_haplotag_problem_count.argtypes = [C.c_void_p]
    L.whamd_haplotag_count.restype = C.c_uint64
    L.whamd_haplotag_count.argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_haplotag_get.restype = C.c_int
    L.whamd_haplotag_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.whamd_haplotag_bx_count.restype = C.c_uint64
    L.whamd_haplotag_bx_count.argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_haplotag_get_bx.restype = C.c_int
    L.whamd_haplotag_get_bx.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.whamd_haplotag_get_stats.restype = C.c_int
    L.whamd_haplotag_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(HaplotagStats)]
    L.whamd_haplotag_destroy.restype = None
    L.whamd_haplotag_destroy.argtypes = [C.c_void_p]
    L.whamd_poly_reorder.restype = C.c_int
    L.whamd_poly_reorder.argtypes = [C.POINTER(PolyReorderView), C.c_uint64, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_poly_reorder_problem_count.restype = C.c_uint64
    L.whamd_poly_reorder_problem_count.argtypes = [C.c_void_p]
    for name in ("whamd_poly_reorder_breakpoint_count", "whamd_poly_reorder_llh_count", "whamd_poly_reorder_window_count"):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_poly_reorder_get_llh.restype = C.c_int
    L.whamd_poly_reorder_get_llh.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.whamd_poly_reorder_get_windows.restype = C.c_int
    L.whamd_poly_reorder_get_windows.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.whamd_poly_reorder_get_phasing.restype = C.c_int
    L.whamd_poly_reorder_get_phasing.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_double)]
    L.whamd_poly_reorder_get_stats.restype = C.c_int
    L.whamd_poly_reorder_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PolyReorderStats)]
    L.whamd_poly_reorder_destroy.restype = None
    L.whamd_poly_reorder_destroy.argtypes = [C.c_void_p]
    L.whamd_poly_compare.restype = C.c_int
    L.whamd_poly_compare.argtypes = [C.POINTER(PolyCompareView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_poly_compare_job_count.restype = C.c_uint64
    L.whamd_poly_compare_job_count.argtypes = [C.c_void_p]
    L.whamd_poly_compare_path_count.restype = C.c_uint64
    L.whamd_poly_compare_path_count.argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_poly_compare_get.restype = C.c_int
    L.whamd_poly_compare_get.argtypes = [C.c_void_p, C.POINTER(PolyCompareJobResult)]
    L.whamd_poly_compare_get_path.restype = C.c_int
    L.whamd_poly_compare_get_path.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                              C.POINTER(C.c_uint32)]
    L.whamd_poly_compare_get_stats.restype = C.c_int
    L.whamd_poly_compare_get_stats.argtypes = [C.c_void_p, C.POINTER(PolyCompareStats)]
    L.whamd_poly_compare_destroy.restype = None
    L.whamd_poly_compare_destroy.argtypes = [C.c_void_p]
    L.whamd_tagphase.restype = C.c_int
    L.whamd_tagphase.argtypes = [C.POINTER(TagphaseView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_tagphase_problem_count.restype = C.c_uint64
    L.whamd_tagphase_problem_count.argtypes = [C.c_void_p]
    for name in ("whamd_tagphase_count", "whamd_tagphase_row_count"):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_tagphase_get.restype = C.c_int
    L.whamd_tagphase_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
    L.whamd_tagphase_get_table.restype = C.c_int
    L.whamd_tagphase_get_table.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_uint64)]
    L.whamd_tagphase_get_stats.restype = C.c_int
    L.whamd_tagphase_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(TagphaseStats)]
    L.whamd_tagphase_destroy.restype = None
    L.whamd_tagphase_destroy.argtypes = [C.c_void_p]
    L.whamd_prior_genotypes.restype = C.c_int
    L.whamd_prior_genotypes.argtypes = [C.POINTER(PriorGenotypesView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_prior_genotypes_problem_count.restype = C.c_uint64
    L.whamd_prior_genotypes_problem_count.argtypes = [C.c_void_p]
    L.whamd_prior_genotypes_count.restype = C.c_uint64
    L.whamd_prior_genotypes_count.argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_prior_genotypes_get.restype = C.c_int
    L.whamd_prior_genotypes_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_int8), C.POINTER(C.c_double), C.POINTER(C.c_int8)]
    L.whamd_prior_genotypes_get_stats.restype = C.c_int
    L.whamd_prior_genotypes_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PriorGenotypesStats)]
    L.whamd_prior_genotypes_destroy.restype = None
    L.whamd_prior_genotypes_destroy.argtypes = [C.c_void_p]
    L.whamd_poly_thread_inputs.restype = C.c_int
    L.whamd_poly_thread_inputs.argtypes = [C.POINTER(PolyThreadView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_poly_thread_problem_count.restype = C.c_uint64
    L.whamd_poly_thread_problem_count.argtypes = [C.c_void_p]
    for name in ("whamd_poly_thread_position_count", "whamd_poly_thread_row_count", "whamd_poly_thread_cov_count"):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_poly_thread_get_rows.restype = C.c_int
    L.whamd_poly_thread_get_rows.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_int8)]
    L.whamd_poly_thread_get_cov.restype = C.c_int
    L.whamd_poly_thread_get_cov.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)]
    L.whamd_poly_thread_get_stats.restype = C.c_int
    L.whamd_poly_thread_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PolyThreadStats)]
    L.whamd_poly_thread_destroy.restype = None
    L.whamd_poly_thread_destroy.argtypes = [C.c_void_p]
    L.whamd_poly_select_clusters.restype = C.c_int
    L.whamd_poly_select_clusters.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.whamd_poly_haplotypes.restype = C.c_int
    L.whamd_poly_haplotypes.argtypes = [C.POINTER(C.c_uint32), C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int8), C.c_int,
                                        C.POINTER(C.c_int8), C.POINTER(C.c_uint32)]
    L.whamd_poly_threader.restype = C.c_int
    L.whamd_poly_threader.argtypes = [C.POINTER(PolyThreaderView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_poly_threader_problem_count.restype = C.c_uint64
    L.whamd_poly_threader_problem_count.argtypes = [C.c_void_p]
    for name in ("whamd_poly_threader_position_count", "whamd_poly_threader_section_count", "whamd_poly_threader_cov_count", "whamd_poly_threader_cost_count"):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_poly_threader_get.restype = C.c_int
    L.whamd_poly_threader_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.whamd_poly_threader_get_stats.restype = C.c_int
    L.whamd_poly_threader_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(PolyThreaderStats)]
    L.whamd_poly_threader_destroy.restype = None
    L.whamd_poly_threader_destroy.argtypes = [C.c_void_p]
    L.whamd_readmerge.restype = C.c_int
    L.whamd_readmerge.argtypes = [C.POINTER(ReadmergeView), C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.whamd_readmerge_problem_count.restype = C.c_uint64
    L.whamd_readmerge_problem_count.argtypes = [C.c_void_p]
    for name in ("whamd_readmerge_count", "whamd_readmerge_super_count", "whamd_readmerge_edge_count"):
        getattr(L, name).restype = C.c_uint64
        getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
    L.whamd_readmerge_get.restype = C.c_int
    L.whamd_readmerge_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.whamd_readmerge_get_edges.restype = C.c_int
    L.whamd_readmerge_get_edges.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint8)]
    L.whamd_readmerge_get_stats.restype = C.c_int
    L.whamd_readmerge_get_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ReadmergeStats)]
    L.whamd_readmerge_destroy.restype = None
    L.whamd_readmerge_destroy.argtypes = [C.c_void_p]
    if L.whamd_abi_version() != ABI_VERSION:
        raise ImportError(f"{path} has ABI version {L.whamd_abi_version()}, this binding was written for {ABI_VERSION} (stale library? run make)")
    return L


# every symbol include/whatshap_amd.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = [
    "whamd_abi_version", "whamd_device_count", "whamd_device_pci_bus_id", "whamd_last_error", "whamd_dptable_create", "whamd_dptable_create_with_options", "whamd_dptable_solve",
    "whamd_dptable_release_device", "whamd_dptable_destroy", "whamd_dptable_column_count", "whamd_dptable_individual_count",
    "whamd_dptable_read_count", "whamd_dptable_positions", "whamd_dptable_get_optimal_score",
    "whamd_dptable_get_super_reads", "whamd_dptable_get_optimal_partitioning", "whamd_dptable_get_index_path",
    "whamd_dptable_get_stats", "whamd_dptable_set_option", "whamd_read_sort_hash", "whamd_plan_summarize",
    "whamd_dptable_enqueue", "whamd_dptable_wait", "whamd_dptable_enqueue_many", "whamd_dptable_wait_many",
    "whamd_pedmec_heuristic_create",
    "whamd_pedmec_heuristic_enqueue_many", "whamd_pedmec_heuristic_wait",
    "whamd_pedmec_heuristic_column_count", "whamd_pedmec_heuristic_sample_count", "whamd_pedmec_heuristic_read_count",
    "whamd_pedmec_heuristic_get", "whamd_pedmec_heuristic_get_stats", "whamd_pedmec_heuristic_destroy",
    "whamd_readselection", "whamd_genotype_likelihoods", "whamd_release_caches", "whamd_host_pool_idle_bytes",
    "whamd_realign_detect", "whamd_realign_result_count", "whamd_realign_get", "whamd_realign_get_stats", "whamd_realign_destroy",
    "whamd_edit_distance_batch",
    "whamd_poly_score", "whamd_poly_score_matrix_count", "whamd_poly_score_count", "whamd_poly_score_get", "whamd_poly_score_get_stats",
    "whamd_poly_score_destroy", "whamd_poly_estimate_error_rate",
    "whamd_progeny_score", "whamd_progeny_score_problem_count", "whamd_progeny_score_count", "whamd_progeny_score_get", "whamd_progeny_score_get_stats",
    "whamd_progeny_score_destroy", "whamd_progeny_variant_types", "whamd_progeny_gl", "whamd_progeny_score_depths",
    "whamd_haplotag", "whamd_haplotag_problem_count", "whamd_haplotag_count", "whamd_haplotag_get", "whamd_haplotag_bx_count", "whamd_haplotag_get_bx",
    "whamd_haplotag_get_stats", "whamd_haplotag_destroy",
    "whamd_poly_reorder", "whamd_poly_reorder_problem_count", "whamd_poly_reorder_breakpoint_count", "whamd_poly_reorder_llh_count",
    "whamd_poly_reorder_window_count", "whamd_poly_reorder_get_llh", "whamd_poly_reorder_get_windows", "whamd_poly_reorder_get_phasing",
    "whamd_poly_reorder_get_stats", "whamd_poly_reorder_destroy",
    "whamd_poly_compare", "whamd_poly_compare_job_count", "whamd_poly_compare_path_count", "whamd_poly_compare_get", "whamd_poly_compare_get_path",
    "whamd_poly_compare_get_stats", "whamd_poly_compare_destroy",
    "whamd_tagphase", "whamd_tagphase_problem_count", "whamd_tagphase_count", "whamd_tagphase_get", "whamd_tagphase_row_count", "whamd_tagphase_get_table",
    "whamd_tagphase_get_stats", "whamd_tagphase_destroy",
    "whamd_prior_genotypes", "whamd_prior_genotypes_problem_count", "whamd_prior_genotypes_count", "whamd_prior_genotypes_get",
    "whamd_prior_genotypes_get_stats", "whamd_prior_genotypes_destroy",
    "whamd_poly_thread_inputs", "whamd_poly_thread_problem_count", "whamd_poly_thread_position_count", "whamd_poly_thread_row_count",
    "whamd_poly_thread_cov_count", "whamd_poly_thread_get_rows", "whamd_poly_thread_get_cov", "whamd_poly_thread_get_stats", "whamd_poly_thread_destroy",
    "whamd_poly_select_clusters", "whamd_poly_haplotypes",
    "whamd_poly_threader", "whamd_poly_threader_problem_count", "whamd_poly_threader_position_count", "whamd_poly_threader_section_count",
    "whamd_poly_threader_cov_count", "whamd_poly_threader_cost_count", "whamd_poly_threader_get", "whamd_poly_threader_get_stats", "whamd_poly_threader_destroy",
    "whamd_readmerge", "whamd_readmerge_problem_count", "whamd_readmerge_count", "whamd_readmerge_super_count", "whamd_readmerge_edge_count",
    "whamd_readmerge_get", "whamd_readmerge_get_edges", "whamd_readmerge_get_stats", "whamd_readmerge_destroy",
]


class SolverError(RuntimeError):
    """RuntimeError with the library's status code attached (the reference raises plain RuntimeError)."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


def raise_status(L, status: int):
    """The library's last error as an exception: ValueError for invalid input (where the reference raises on the same input), else SolverError."""
    msg = L.whamd_last_error().decode("utf-8", "replace")
    if status == WHAMD_ERR_INVALID:
        raise ValueError(msg)
    raise SolverError(status, msg)


def checked(L, status: int) -> None:
    """A getter's or an entry point's status: raises through raise_status unless it is WHAMD_OK."""
    if status != WHAMD_OK:
        raise_status(L, status)


@contextlib.contextmanager
def batch_handle(host: bool, views, product_entry: str, debug_entry: Optional[str], destroy_name: str, *extra_args, device: int = 0):
    """One batch call and the life of its result handle: ``with batch_handle(...) as (L, h)``.  ``views`` is the list of the problems'
    view structs; the product entry point is called as (views, n, *extra_args, device, &h), with ``host`` the debug library's twin as
    (views, n, *extra_args, &h).  A failed call raises (raise_status) before the block is entered; the handle is destroyed on exit."""
    L = debug_lib() if host else lib()
    n = len(views)
    array = (type(views[0]) * n)(*views) if n else None
    h = C.c_void_p()
    if host:
        checked(L, getattr(L, debug_entry)(array, n, *extra_args, C.byref(h)))
    else:
        checked(L, getattr(L, product_entry)(array, n, *extra_args, int(device), C.byref(h)))
    try:
        yield L, h
    finally:
        getattr(L, destroy_name)(h)


def read_stats(L, getter: str, StatsType, h, *index) -> dict:
    """The stats struct of a result handle (of problem ``index``, where the result has one per problem) as a dict."""
    s = StatsType()
    checked(L, getattr(L, getter)(h, *index, C.byref(s)))
    return s.as_dict()


def _check(status: int, L=None):
    if status != WHAMD_OK:
        raise SolverError(status, (L or lib()).whamd_last_error().decode("utf-8", "replace"))


def _library_of(tables):
    """The library that created these tables (product or debug build: never mixed in one call)."""
    libs = {id(getattr(t, "_L", None)): getattr(t, "_L", None) for t in tables}
    if len(libs) != 1:
        raise ValueError("tables of the product and of the debug library cannot share a call")
    return next(iter(libs.values())) or lib()


def enqueue_many(tables) -> None:
    """whamd_dptable_enqueue_many: submits the solves of several tables with interleaved launch sequences."""
    tables = list(tables)
    if not tables:
        return
    arr = (C.c_void_p * len(tables))(*[t._h.value for t in tables])
    _check(_library_of(tables).whamd_dptable_enqueue_many(arr, len(tables)))


def wait_many(tables) -> None:
    """whamd_dptable_wait_many: collects several tables in flight; their host-side result extraction runs on a few threads at once."""
    tables = list(tables)
    if not tables:
        return
    arr = (C.c_void_p * len(tables))(*[t._h.value for t in tables])
    _check(_library_of(tables).whamd_dptable_wait_many(arr, len(tables)))


class NativeTable:
    """Thin RAII wrapper of whamd_dptable: create -> (set_option) -> solve -> getters."""

    def __init__(self, problem: ProblemArrays, device: int = 0, path: Optional[str] = None, solve: bool = True, options: Optional[dict] = None):
        L = self._L = lib()   # the library that makes the handle also queries and destroys it (the debug build has pools and arenas of its own)
        self._h = C.c_void_p()
        self._problem = problem  # keep the arrays alive while create() reads them
        opts = dict(options or {})
        if path is not None:
            opts["path"] = path
        if opts:   # applied before the plan is made: one upload
            keys = (C.c_char_p * len(opts))(*[str(k).encode() for k in opts])
            values = (C.c_char_p * len(opts))(*[str(v).encode() for v in opts.values()])
            _check(L.whamd_dptable_create_with_options(*problem.call_args(), keys, values, C.c_size_t(len(opts)), C.c_int(device), C.byref(self._h)))
        else:
            _check(L.whamd_dptable_create(*problem.call_args(), C.c_int(device), C.byref(self._h)))
        self.n_columns = int(L.whamd_dptable_column_count(self._h))
        self.n_individuals = int(L.whamd_dptable_individual_count(self._h))
        self.n_reads = int(L.whamd_dptable_read_count(self._h))
        if solve:
            self.solve()

    def set_option(self, key: str, value: str):
        _check(self._L.whamd_dptable_set_option(self._h, key.encode(), value.encode()))

    def solve(self):
        _check(self._L.whamd_dptable_solve(self._h))

    def enqueue(self):
        """Submit the solve to the table's stream without waiting (pair with wait())."""
        _check(self._L.whamd_dptable_enqueue(self._h))

    def wait(self):
        _check(self._L.whamd_dptable_wait(self._h))

    def release_device(self):
        """Frees the device side of a solved table; the getters keep working."""
        _check(self._L.whamd_dptable_release_device(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.whamd_dptable_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def positions(self) -> np.ndarray:
        out = np.zeros(self.n_columns, dtype=np.uint32)
        _check(self._L.whamd_dptable_positions(self._h, _ptr(out, C.c_uint32)))
        return out

    def optimal_score(self) -> int:
        v = C.c_uint32()
        _check(self._L.whamd_dptable_get_optimal_score(self._h, C.byref(v)))
        return int(v.value)

    def super_reads(self):
        n, ni = self.n_columns, self.n_individuals
        a0 = np.zeros((ni, n), dtype=np.uint8)
        a1 = np.zeros((ni, n), dtype=np.uint8)
        q = np.zeros((ni, n), dtype=np.uint32)
        tv = np.zeros(n, dtype=np.uint32)
        sid = np.zeros(ni, dtype=np.uint32)
        _check(self._L.whamd_dptable_get_super_reads(
            self._h, _ptr(a0, C.c_uint8), _ptr(a1, C.c_uint8), _ptr(q, C.c_uint32), _ptr(tv, C.c_uint32), _ptr(sid, C.c_uint32)))
        return a0, a1, q, tv, sid

    def partitioning(self) -> np.ndarray:
        out = np.zeros(self.n_reads, dtype=np.uint8)
        _check(self._L.whamd_dptable_get_optimal_partitioning(self._h, _ptr(out, C.c_uint8)))
        return out

    def index_path(self):
        idx = np.zeros(self.n_columns, dtype=np.uint32)
        tv = np.zeros(self.n_columns, dtype=np.uint32)
        _check(self._L.whamd_dptable_get_index_path(self._h, _ptr(idx, C.c_uint32), _ptr(tv, C.c_uint32)))
        return idx, tv

    def stats(self) -> dict:
        s = SolveStats()
        _check(self._L.whamd_dptable_get_stats(self._h, C.byref(s)))
        return s.as_dict()


def plan_summary(problem: ProblemArrays, path: str = "auto") -> dict:
    """Host-only: how whamd_dptable_create would schedule the columns of `problem` (no device needed)."""
    out = PlanSummary()
    _check(lib().whamd_plan_summarize(*problem.call_args(), path.encode(), C.byref(out)))
    return out.as_dict()


def emulate_slot_plan(problem: ProblemArrays, n_columns: int, slot_l: int = 11, symmetry: int = 1, slot_r: int = 2):
    """Host-only planner diagnostic (whamd_debug_emulate_slot_plan): (index path, optimal score, columns inside runs).
    slot_r: reg slots per thread (1, 2 or 3; passed as slot_l + 100 for 3, + 200 for 1)."""
    if slot_r >= 3:
        slot_l += 100
    elif slot_r <= 1:
        slot_l += 200
    idx = np.zeros(max(n_columns, 1), dtype=np.uint32)
    score = C.c_uint32()
    ncols = C.c_uint64()
    D = debug_lib()
    _check(D.whamd_debug_emulate_slot_plan(*problem.call_args(), C.c_int(slot_l), C.c_int(symmetry), _ptr(idx, C.c_uint32),
                                           C.byref(score), C.byref(ncols)), D)
    return idx[:n_columns], int(score.value), int(ncols.value)


def emulate_pedslot_plan(problem: ProblemArrays, n_columns: int, slot_l: int = 0):
    """Host-only diagnostic of the pedigree slot plan (whamd_debug_emulate_pedslot_plan):
    (index path, transmission path, optimal score, columns inside runs)."""
    idx = np.zeros(max(n_columns, 1), dtype=np.uint32)
    trans = np.zeros(max(n_columns, 1), dtype=np.uint32)
    score = C.c_uint32()
    ncols = C.c_uint64()
    D = debug_lib()
    _check(D.whamd_debug_emulate_pedslot_plan(*problem.call_args(), C.c_int(slot_l), _ptr(idx, C.c_uint32), _ptr(trans, C.c_uint32),
                                              C.byref(score), C.byref(ncols)), D)
    return idx[:n_columns], trans[:n_columns], int(score.value), int(ncols.value)


def debug_lazy_terms_check(problem: ProblemArrays, need=None, rounds: int = 1) -> dict:
    """whamd_debug_lazy_terms_check: the lazily built generic term lists (+ fill_lazy_terms on the columns of `need`, in `rounds` calls) against the eager ones."""
    D = debug_lib()
    fn = D.whamd_debug_lazy_terms_check
    fn.restype = C.c_int
    lazy, diff, before, after = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    need_arr = None if need is None else np.ascontiguousarray(need, dtype=np.uint8)
    _check(fn(*problem.call_args(), None if need_arr is None else _ptr(need_arr, C.c_uint8), C.c_int(int(rounds)), C.byref(lazy), C.byref(diff),
              C.byref(before), C.byref(after)), D)
    return {"lazy": bool(lazy.value), "differences": int(diff.value), "built_before": int(before.value), "built_after": int(after.value)}


class DebugGenotypeRun(C.Structure):
    """whamd_debug_genotype_run (include/whatshap_amd_debug.h)."""
    _fields_ = [(name, C.c_uint32) for name in ("c0", "ncols", "rescale_f", "rescale_b", "emit_f", "emit_b", "n_part_out", "part_out_f", "part_out_b",
                                                "part_in_f", "n_part_in_f", "part_in_b", "n_part_in_b", "reserved")]


def debug_genotype_run_plan(problem: ProblemArrays):
    """Host-only (whamd_debug_genotype_run_plan): (the runs of the genotyper's run path as dicts, the scaled column total below which a solve
    leaves the run path); None when the table is not eligible for the run path."""
    D = debug_lib()
    fn = D.whamd_debug_genotype_run_plan
    fn.restype = C.c_int
    a = problem.call_args()
    args = (a[0], a[1], a[2], a[3], a[5], a[6])
    n, min_total = C.c_size_t(), C.c_double()
    status = fn(*args, None, C.c_size_t(0), C.byref(n), C.byref(min_total))
    if status == WHAMD_ERR_UNSUPPORTED:
        return None
    _check(status, D)
    runs = (DebugGenotypeRun * max(n.value, 1))()
    _check(fn(*args, runs, C.c_size_t(n.value), C.byref(n), C.byref(min_total)), D)
    names = [f[0] for f in DebugGenotypeRun._fields_ if f[0] != "reserved"]
    return [{k: int(getattr(runs[i], k)) for k in names} for i in range(n.value)], float(min_total.value)


class DebugKernel(C.Structure):
    """whamd_debug_kernel (include/whatshap_amd_debug.h)."""
    _fields_ = [("kernel", C.c_void_p), ("name", C.c_char_p), ("large_lds_opted_in", C.c_int32), ("debug_only", C.c_int32)]


LAUNCH_SITES = ("column", "run", "slot_run", "batch", "group", "group_walk", "tail", "window_walk", "tables")   # WHAMD_LAUNCH_*
LAUNCH_FACTS = ("lr", "yflags", "spec", "stamps", "tb", "nf", "ncols", "threads", "streamed", "pack", "tight", "variant", "T", "n_ind", "mode", "wide",
                "ped", "sym", "entries")


class DebugLaunch(C.Structure):
    """whamd_debug_launch (include/whatshap_amd_debug.h)."""
    _fields_ = ([("kernel", C.c_void_p), ("site", C.c_uint32), ("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("block", C.c_uint32), ("lds", C.c_uint32),
                 ("own_stream", C.c_uint32), ("forward", C.c_uint32)] + [(f, C.c_int32) for f in LAUNCH_FACTS] +
                [("preview", C.c_int32), ("reserved", C.c_int32), ("count", C.c_uint64), ("name", C.c_char_p)])


class DebugPreview(C.Structure):
    """whamd_debug_preview (include/whatshap_amd_debug.h)."""
    _fields_ = [("ran", C.c_int32), ("continued", C.c_int32), ("pieces", C.c_uint32), ("launched_steps", C.c_uint32), ("agreed_steps", C.c_uint32),
                ("from_hook", C.c_uint32), ("why_not", C.c_char_p)]


def debug_preview(table) -> dict:
    """whamd_debug_dptable_preview: what became of the preview of `table` (made by the debug library): ran, continued, pieces, launched_steps,
    agreed_steps, from_hook (the launches went out from the planner's head hook), why_not."""
    D = debug_lib()
    if table._L is not D:
        raise ValueError("the preview's record exists in the debug library only (use_debug_library() before the table is made)")
    out = DebugPreview()
    _check(D.whamd_debug_dptable_preview(table._h, C.byref(out)), D)
    return {"ran": bool(out.ran), "continued": bool(out.continued), "pieces": int(out.pieces), "launched_steps": int(out.launched_steps),
            "agreed_steps": int(out.agreed_steps), "from_hook": bool(out.from_hook), "why_not": (out.why_not or b"").decode()}


class DebugHeadPlan(C.Structure):
    """whamd_debug_head_plan_result (include/whatshap_amd_debug.h)."""
    _fields_ = [("n_pieces", C.c_uint32), ("head_steps", C.c_uint32), ("n_steps", C.c_uint32), ("hook_calls", C.c_uint32),
                ("digest", C.c_uint64), ("head_digest_in_hook", C.c_uint64), ("head_digest", C.c_uint64),
                ("edge_yflags", C.c_uint32 * 2), ("n_runs", C.c_uint32), ("n_components", C.c_uint32)]


def debug_head_first_plan(problem: ProblemArrays, head_pieces: int = 0) -> dict:
    """whamd_debug_head_first_plan (host only): the slot plan of a single-individual table with the head -- the leading slot runs inside the first `head_pieces`
    plan pieces -- finished first (0: without the hook), as digests: of the whole plan, of the head's part inside the callback and in the finished plan."""
    D = debug_lib()
    fn = D.whamd_debug_head_first_plan
    fn.restype = C.c_int
    out = DebugHeadPlan()
    _check(fn(*problem.call_args(), C.c_uint32(head_pieces), C.byref(out)), D)
    rec = {name: int(getattr(out, name)) for name, _ in DebugHeadPlan._fields_ if name != "edge_yflags"}
    rec["edge_yflags"] = tuple(None if v == 0xFFFFFFFF else int(v) for v in out.edge_yflags)
    return rec


class DebugPreviewPlan(C.Structure):
    """whamd_debug_preview_plan_result (include/whatshap_amd_debug.h)."""
    _fields_ = [("n_pieces", C.c_uint32), ("pieces", C.c_uint32), ("steps", C.c_uint32), ("n_steps", C.c_uint32),
                ("chunked_predicted", C.c_int32), ("chunked", C.c_int32), ("windowed", C.c_int32), ("reserved", C.c_int32),
                ("n_seeds_predicted", C.c_uint32), ("n_seeds", C.c_uint32), ("stride_predicted", C.c_uint32), ("stride", C.c_uint32),
                ("arena_predicted", C.c_uint64), ("arena_laid_out", C.c_uint64), ("exchange_predicted", C.c_uint64), ("exchange_laid_out", C.c_uint64),
                ("why_not", C.c_char_p)]


def debug_preview_plan(problem: ProblemArrays, pieces: int = 0) -> dict:
    """whamd_debug_preview_plan (host only): what a preview over `pieces` plan pieces works out ahead of the create -- per leading step the record offset and
    the seed id -- beside what the create's own layout gives (rec_predicted / rec_laid_out / spec_predicted / spec_laid_out), and the scalars of the struct."""
    D = debug_lib()
    fn = D.whamd_debug_preview_plan
    fn.restype = C.c_int
    out = DebugPreviewPlan()
    _check(fn(*problem.call_args(), C.c_uint32(pieces), C.byref(out), None, None, None, None, C.c_size_t(0)), D)
    n = int(out.steps)
    arrays = {"rec_predicted": np.zeros(max(n, 1), dtype=np.uint64), "rec_laid_out": np.zeros(max(n, 1), dtype=np.uint64),
              "spec_predicted": np.zeros(max(n, 1), dtype=np.uint32), "spec_laid_out": np.zeros(max(n, 1), dtype=np.uint32)}
    _check(fn(*problem.call_args(), C.c_uint32(pieces), C.byref(out), _ptr(arrays["rec_predicted"], C.c_uint64), _ptr(arrays["rec_laid_out"], C.c_uint64),
              _ptr(arrays["spec_predicted"], C.c_uint32), _ptr(arrays["spec_laid_out"], C.c_uint32), C.c_size_t(n)), D)
    rec = {name: (getattr(out, name).decode() if name == "why_not" else int(getattr(out, name))) for name, _ in DebugPreviewPlan._fields_ if name != "reserved"}
    rec.update({k: v[:n] for k, v in arrays.items()})
    return rec


def debug_solve_kernels() -> list:
    """whamd_debug_solve_kernels: the registry of the solve's kernels -- dicts of name (the instantiation's spelling), large_lds_opted_in, debug_only."""
    D = debug_lib()
    n = D.whamd_debug_solve_kernels(None, 0)
    arr = (DebugKernel * n)()
    D.whamd_debug_solve_kernels(arr, n)
    return [{"kernel": k.kernel, "name": k.name.decode(), "large_lds_opted_in": bool(k.large_lds_opted_in), "debug_only": bool(k.debug_only)} for k in arr]


def debug_launches(table) -> list:
    """whamd_debug_dptable_launches: the launch ledger of the solve `table` (made by the debug library) collected last.  One dict per distinct
    launch: name (of the registry), site (LAUNCH_SITES), grid_x, grid_y, block, lds, own_stream, forward, count, preview (the launch was made by the
    create: the table's preview) and the facts the choice was made
    from (LAUNCH_FACTS; None where the launch site does not have the fact).  A kernel the registry does not know is an error."""
    D = debug_lib()
    if table._L is not D:
        raise ValueError("the launch ledger exists in the debug library only (use_debug_library() before the table is made)")
    n = C.c_size_t()
    _check(D.whamd_debug_dptable_launches(table._h, None, 0, C.byref(n)), D)
    arr = (DebugLaunch * max(n.value, 1))()
    _check(D.whamd_debug_dptable_launches(table._h, arr, n.value, C.byref(n)), D)
    out = []
    for r in arr[:n.value]:
        if r.name is None:
            raise RuntimeError(f"a launch of site {LAUNCH_SITES[r.site]} (grid {r.grid_x} x {r.grid_y}, block {r.block}) took a kernel the registry does not list")
        rec = {"name": r.name.decode(), "site": LAUNCH_SITES[r.site], "grid_x": r.grid_x, "grid_y": r.grid_y, "block": r.block, "lds": r.lds,
               "own_stream": bool(r.own_stream), "forward": bool(r.forward), "count": int(r.count), "preview": bool(r.preview)}
        rec.update({f: (None if getattr(r, f) < 0 else getattr(r, f)) for f in LAUNCH_FACTS})
        out.append(rec)
    return out


def _heuristic_result(L, h) -> dict:
    n = int(L.whamd_pedmec_heuristic_column_count(h))
    ns = int(L.whamd_pedmec_heuristic_sample_count(h))
    nr = int(L.whamd_pedmec_heuristic_read_count(h))
    score = C.c_float()
    bip = np.zeros(max(nr, 1), dtype=np.uint8)
    trans = np.zeros(max(n, 1), dtype=np.uint32)
    haps = np.zeros((max(ns, 1), 2, max(n, 1)), dtype=np.int8)
    mut = np.zeros((max(ns, 1), 2, max(n, 1)), dtype=np.uint8)
    sid = np.zeros(max(ns, 1), dtype=np.uint32)
    pos = np.zeros(max(n, 1), dtype=np.uint32)
    _check(L.whamd_pedmec_heuristic_get(h, C.byref(score), _ptr(bip, C.c_uint8), _ptr(trans, C.c_uint32), haps.ctypes.data_as(C.POINTER(C.c_int8)),
                                        _ptr(mut, C.c_uint8), _ptr(sid, C.c_uint32), _ptr(pos, C.c_uint32)), L)
    stats = HeuristicStats()
    _check(L.whamd_pedmec_heuristic_get_stats(h, C.byref(stats)), L)
    return {"score": float(score.value), "bipartition": bip[:nr], "transmission": trans[:n], "haplotypes": haps[:ns, :, :n], "mutated": mut[:ns, :, :n],
            "sample_ids": sid[:ns], "positions": pos[:n], "stats": stats.as_dict()}


def pedmec_heuristic(problem: ProblemArrays, row_limit: int = 256, allow_mutations: bool = True, device: int = 0, host_diagnostic: bool = False) -> dict:
    """whamd_pedmec_heuristic_create + _get: the beam search of PedMecHeuristic (constructor + solve) and everything its getters
    return.  host_diagnostic: the same solver source on one CPU thread (tests only)."""
    L = debug_lib() if host_diagnostic else lib()   # (the handle stays with the library that made it)
    h = C.c_void_p()
    a = problem.call_args()
    if host_diagnostic:
        _check(L.whamd_debug_pedmec_heuristic_create_host(*a, C.c_uint32(int(row_limit)), C.c_int(1 if allow_mutations else 0), C.byref(h)), L)
    else:
        _check(L.whamd_pedmec_heuristic_create(*a, C.c_uint32(int(row_limit)), C.c_int(1 if allow_mutations else 0), C.c_int(int(device)), C.byref(h)))
    try:
        return _heuristic_result(L, h)
    finally:
        L.whamd_pedmec_heuristic_destroy(h)


class HeuristicBatch:
    """whamd_pedmec_heuristic_enqueue_many: several tables in ONE launch (one persistent workgroup each) on a stream of the batch's own;
    `results()` waits and returns one dict per table (as pedmec_heuristic)."""

    def __init__(self, problems, row_limit: int = 256, allow_mutations: bool = True, device: int = 0):
        L = lib()
        problems = list(problems)
        self._L = L
        self._n = len(problems)
        self._handles = (C.c_void_p * max(self._n, 1))()
        jobs = (HeuristicJob * max(self._n, 1))()
        for i, p in enumerate(problems):   # (the problems outlive the call: the arrays are only read during _enqueue_many)
            jobs[i].readset = C.pointer(p.readset_view)
            jobs[i].recombcost = _ptr(p.recombcost, C.c_uint32)
            jobs[i].n_recombcost = p.recombcost.size
            jobs[i].pedigree = C.pointer(p.pedigree_view)
            jobs[i].distrust_genotypes = 1 if p.distrust_genotypes else 0
            jobs[i].positions = _ptr(p.positions, C.c_uint32)
            jobs[i].n_positions = 0 if p.positions is None else p.positions.size
            jobs[i].row_limit = int(row_limit)
            jobs[i].allow_mutations = 1 if allow_mutations else 0
        if self._n:
            _check(L.whamd_pedmec_heuristic_enqueue_many(jobs, self._n, C.c_int(int(device)), self._handles))

    def results(self):
        out = []
        try:
            for i in range(self._n):
                _check(self._L.whamd_pedmec_heuristic_wait(self._handles[i]))
                out.append(_heuristic_result(self._L, self._handles[i]))
        finally:
            self.close()
        return out

    def close(self):
        for i in range(self._n):
            if self._handles[i]:
                self._L.whamd_pedmec_heuristic_destroy(self._handles[i])
                self._handles[i] = None
        self._n = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pedmec_heuristic_many(problems, row_limit: int = 256, allow_mutations: bool = True, device: int = 0):
    """Several tables through one batched launch; one result dict per table."""
    return HeuristicBatch(problems, row_limit, allow_mutations, device).results()


def host_pool_idle_bytes() -> int:
    """whamd_host_pool_idle_bytes: host memory the library keeps between tables (given back by release_caches())."""
    fn = lib().whamd_host_pool_idle_bytes
    fn.restype = C.c_uint64
    return int(fn())


def device_count() -> int:
    return int(lib().whamd_device_count())


def device_pci_bus_id(device: int) -> str:
    """whamd_device_pci_bus_id: "0000:c5:00.0" of HIP device `device` (raises SolverError / WHAMD_ERR_DEVICE if there is none)."""
    buf = C.create_string_buffer(64)
    fn = lib().whamd_device_pci_bus_id
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    _check(fn(int(device), buf, 64))
    return buf.value.decode()


def readselection(read_ptr, var_position, var_quality, max_cov: int, read_source_id=None, preferred_source_ids=None,
                  bridging: bool = True) -> np.ndarray:
    """whamd_readselection on flat arrays: boolean mask [n_reads] of the selected reads."""
    read_ptr = np.ascontiguousarray(read_ptr, dtype=np.uint64)
    if read_ptr.size == 0:
        read_ptr = np.zeros(1, dtype=np.uint64)
    var_position = np.ascontiguousarray(var_position, dtype=np.int32)
    var_quality = np.ascontiguousarray(var_quality, dtype=np.uint32)
    n_reads = read_ptr.size - 1
    assert var_position.size == var_quality.size == int(read_ptr[-1])
    view = ReadSetView(n_reads, _ptr(read_ptr, C.c_uint64), _ptr(var_position, C.c_int32), None, _ptr(var_quality, C.c_uint32), None)
    preferred = np.ascontiguousarray(sorted(preferred_source_ids) if preferred_source_ids is not None else [], dtype=np.int32)
    sources = None
    if preferred.size:
        sources = np.ascontiguousarray(read_source_id, dtype=np.int32)
        assert sources.size == n_reads
    selected = np.zeros(max(n_reads, 1), dtype=np.uint8)
    count = C.c_uint64()
    _check(lib().whamd_readselection(C.byref(view), None if sources is None else _ptr(sources, C.c_int32),
                                     _ptr(preferred, C.c_int32) if preferred.size else None, preferred.size,
                                     C.c_uint32(int(max_cov)), C.c_int(1 if bridging else 0), _ptr(selected, C.c_uint8), C.byref(count)))
    return selected[:n_reads].astype(bool)


def genotype_likelihoods(problem: ProblemArrays, n_columns: int, device: int = 0, window: int = 0):
    """whamd_genotype_likelihoods: (likelihoods [individuals, columns, 3], stats dict)."""
    n_ind = problem.n_individuals
    gl = np.zeros((n_ind, int(n_columns), 3), dtype=np.float64)
    stats = GenotypeStats()
    a = problem.call_args()
    _check(lib().whamd_genotype_likelihoods(a[0], a[1], a[2], a[3], a[5], a[6], C.c_int(int(device)), C.c_uint32(int(window)),
                                            _ptr(gl, C.c_double), C.c_size_t(max(gl.size, 1) if gl.size else 0), C.byref(stats)))
    if int(stats.n_columns) != int(n_columns):
        # the library strides its output by ITS column count: a different count here would silently mis-align every individual after the first
        raise SolverError(WHAMD_ERR_INVALID, f"genotype_likelihoods: caller assumed {n_columns} columns, the library found {int(stats.n_columns)}")
    return gl, stats.as_dict()


def release_caches() -> None:
    """whamd_release_caches: frees the device memory the genotyping path keeps between calls."""
    lib().whamd_release_caches.restype = None
    lib().whamd_release_caches()


def read_sort_hash(name: str, source_id: int) -> int:
    return int(lib().whamd_read_sort_hash(name.encode("utf-8"), int(source_id)))
