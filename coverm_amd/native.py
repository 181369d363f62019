"""ctypes binding of libcovermhip.so (include/covermhip.h).

This is the same binding shape a Rust `extern "C"` block would have.  Loading fails
loudly when the shared library is missing: there is no Python or CPU fallback for the hot path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcovermhip.so")

COV_OK = 0
ERR_UNSORTED, ERR_NM_MISSING, ERR_NM_BADTYPE, ERR_POS_OOB, ERR_BAD_CIGAR, ERR_BAD_TID = 1, 2, 3, 4, 6, 7
ERR_INVALID_ARG, ERR_HIP, ERR_STATE = 16, 17, 18
WANT_HIST, WANT_IDENTITY = 1, 2
WANT_IDENTITY_PRIMARY_ONLY, WANT_IDENTITY_NONSUPP_ONLY = 4, 8
K_PREP, K_RANGES, K_PILEUP, K_IDENTITY, K_HIST, K_HIST_COMPACT, K_ESTIMATE, K_COUNT = 0, 1, 2, 3, 4, 5, 6, 15
K_GENOME = 7      # cov_set_genomes: reduce + histogram merge + estimate over genomes (Session.genome_kernel_ms)
K_GROUP = 8       # cov_group_records: order check + sort passes + gather of the last call (Session.group_kernel_ms)
K_SEP = 10        # cov_set_genome_runs: the entry table of the finish, in front of K_GENOME (Session.sep_kernel_ms)
K_GENE_READS = 11 # cov_interval_reads_compute: the kernels of the last call (Session.gene_reads_kernel_ms)
K_DEPTH_RUNS = 12 # cov_depth_runs_compute: the run kernels of the last chunk (Session.depth_runs_kernel_ms)
K_DEPTH_BINS = 13 # cov_depth_bins_compute: the bin kernels of the last chunk (Session.depth_bins_kernel_ms)
K_DEPTH_REGIONS = 14 # cov_depth_regions_compute: the region kernels of the last chunk (Session.depth_regions_kernel_ms)
K_SAM = 9         # cov_sam_*: the decode kernels of the last SAM text ingest (Session.sam_kernel_ms)
KERNEL_NAMES = {K_PREP: "k_prep", K_RANGES: "k_ranges", K_PILEUP: "k_pileup", K_IDENTITY: "k_identity",
                K_HIST: "k_hist", K_HIST_COMPACT: "k_hist_compact", K_ESTIMATE: "k_estimate"}


class CovConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("include_improper_pairs", C.c_uint8), ("include_supplementary", C.c_uint8),
                ("include_secondary", C.c_uint8), ("filter_single", C.c_uint8), ("min_mapq", C.c_uint8),
                ("reserved0", C.c_uint8 * 3), ("min_aligned_length", C.c_uint32),
                ("min_percent_identity", C.c_float), ("min_aligned_percent", C.c_float),
                ("contig_end_exclusion", C.c_uint64), ("want", C.c_uint32), ("reserved1", C.c_uint32)]


class CovBatch(C.Structure):
    _fields_ = [("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p),
                ("nm", C.c_void_p), ("nm_kind", C.c_void_p), ("l_seq", C.c_void_p), ("cigar_off", C.c_void_p),
                ("cigar", C.c_void_p), ("n_records", C.c_uint64)]


class CovSummary(C.Structure):
    _fields_ = [("num_detected_primary_alignments", C.c_uint64), ("n_records", C.c_uint64),
                ("n_considered", C.c_uint64), ("hist_total", C.c_uint64)]


# numpy mirror of cov_contig_stats (128 bytes)
CONTIG_STATS_DTYPE = np.dtype([
    ("n_primary", "<u8"), ("n_pass", "<u8"), ("n_nonsupp", "<u8"), ("sum_nm", "<u8"), ("sum_indel", "<u8"),
    ("sum_identity_primary", "<f8"), ("sum_identity_nonsupp", "<f8"), ("win_sum_d", "<u8"), ("win_sum_d2", "<u8"),
    ("win_covered", "<u8"), ("full_covered", "<u8"), ("first_record", "<u8"), ("last_record", "<u8"),
    ("win_min_d", "<u4"), ("win_max_d", "<u4"), ("hist_len", "<u4"), ("reserved", "<u4"), ("hist_off", "<u8")])
assert CONTIG_STATS_DTYPE.itemsize == 128

# numpy mirror of cov_genome_stats (24 bytes)
GENOME_STATS_DTYPE = np.dtype([("reads_in_genome", "<u8"), ("genome_len", "<u8"), ("n_contigs_seen", "<u4"), ("any_nonzero", "<u4")])
assert GENOME_STATS_DTYPE.itemsize == 24

# numpy mirror of cov_genome_entry (24 bytes)
GENOME_ENTRY_DTYPE = np.dtype([("reads", "<u8"), ("first_tid", "<u4"), ("gid", "<i4"), ("n_contigs_seen", "<u4"), ("any_nonzero", "<u4")])
assert GENOME_ENTRY_DTYPE.itemsize == 24

# numpy mirrors of cov_interval (24 bytes) and cov_interval_reads (32 bytes)
INTERVAL_DTYPE = np.dtype([("tid", "<u4"), ("pad", "<u4"), ("start", "<u8"), ("end", "<u8")])
INTERVAL_READS_DTYPE = np.dtype([("n_reads", "<u8"), ("mismatches", "<u8"), ("sum_identity", "<f8"), ("contig_taken", "<u8")])
assert INTERVAL_DTYPE.itemsize == 24 and INTERVAL_READS_DTYPE.itemsize == 32

# numpy mirror of cov_depth_run (8 bytes)
DEPTH_RUN_DTYPE = np.dtype([("start", "<u4"), ("depth", "<i4")])
assert DEPTH_RUN_DTYPE.itemsize == 8


class CovDepthRunsInfo(C.Structure):
    _fields_ = [("arena_bases", C.c_uint64), ("n_runs", C.c_uint64), ("arena_ms", C.c_double), ("runs_ms", C.c_double),
                ("tid_lo", C.c_uint32), ("tid_next", C.c_uint32)]


DEPTH_MAX_CUTS = 16      # COV_DEPTH_MAX_CUTS: values of a cut list (cov_depth_class_runs_compute, cov_depth_thresholds_set)

# numpy mirror of cov_depth_bin (24 bytes)
DEPTH_BIN_DTYPE = np.dtype([("sum", "<u8"), ("min", "<i4"), ("max", "<i4"), ("covered", "<u4"), ("reserved", "<u4")])
assert DEPTH_BIN_DTYPE.itemsize == 24


class CovDepthBinsInfo(C.Structure):
    _fields_ = [("arena_bases", C.c_uint64), ("n_bins", C.c_uint64), ("arena_ms", C.c_double), ("bins_ms", C.c_double),
                ("tid_lo", C.c_uint32), ("tid_next", C.c_uint32), ("bin_size", C.c_uint32), ("reserved", C.c_uint32)]


# numpy mirror of cov_depth_region (16 bytes): [start, end) of target tid, 0-based, half open
DEPTH_REGION_DTYPE = np.dtype([("tid", "<u4"), ("start", "<u4"), ("end", "<u4"), ("reserved", "<u4")])
assert DEPTH_REGION_DTYPE.itemsize == 16


class CovDepthRegionsInfo(C.Structure):
    _fields_ = [("arena_bases", C.c_uint64), ("n_regions", C.c_uint64), ("n_pieces", C.c_uint64), ("arena_ms", C.c_double), ("regions_ms", C.c_double),
                ("tid_lo", C.c_uint32), ("tid_next", C.c_uint32)]


EXPORTS = ["cov_abi_version", "cov_create", "cov_destroy", "cov_last_error", "cov_set_targets",
           "cov_set_target_mask", "cov_push_batch", "cov_push_batch_device", "cov_finish", "cov_fetch_hist",
           "cov_copy_depth", "cov_reset", "cov_kernel_ms", "cov_algorithmic_bytes", "cov_last_paths", "cov_pileup_schedule", "cov_copy_run_words",
           "cov_set_genomes", "cov_finish_genomes", "cov_fetch_genome_estimates", "cov_fetch_genome_stats",
           "cov_set_genome_runs", "cov_genome_entry_count", "cov_fetch_genome_entries",
           "cov_sam_begin", "cov_sam_window_bytes", "cov_sam_slot_wait", "cov_sam_feed", "cov_sam_end", "cov_ingest_last_stats",
           "cov_interval_reads_compute", "cov_depth_runs_compute", "cov_depth_runs_fetch", "cov_depth_runs_last",
           "cov_depth_bins_compute", "cov_depth_bins_fetch", "cov_depth_bins_last",
           "cov_depth_regions_set", "cov_depth_regions_compute", "cov_depth_regions_fetch", "cov_depth_regions_last",
           "cov_depth_class_runs_compute", "cov_depth_thresholds_set", "cov_depth_regions_counts_fetch"]

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def _torch_hip_first():
    """PyTorch-ROCm ships its own copy of the HIP runtime.  If torch is already imported in this process its runtime
    must come up BEFORE libcovermhip.so is loaded: the loader then binds our NEEDED libamdhip64 to the copy torch
    loaded (same SONAME) and both share one runtime; in the other order torch later reports "No HIP GPUs are available"."""
    import sys
    t = sys.modules.get("torch")
    if t is None:
        return
    try:
        if t.cuda.is_available():
            t.cuda.init()
    except Exception:
        pass


def lib():
    """Loads libcovermhip.so.  Raises if it has not been built: the HIP path is the only path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            "%s not found — build it with `python -m coverm_amd.build` (hipcc, gfx950). "
            "coverm_amd has no CPU fallback for the coverage hot path." % LIB_PATH)
    _torch_hip_first()
    L = C.CDLL(LIB_PATH)
    L.cov_abi_version.restype = C.c_int
    L.cov_last_error.restype = C.c_char_p
    L.cov_last_error.argtypes = [C.c_void_p]
    L.cov_create.argtypes = [C.POINTER(CovConfig), C.POINTER(C.c_void_p)]
    L.cov_destroy.argtypes = [C.c_void_p]
    L.cov_destroy.restype = None
    L.cov_set_targets.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.cov_set_target_mask.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_push_batch.argtypes = [C.c_void_p, C.POINTER(CovBatch)]
    L.cov_push_batch_device.argtypes = [C.c_void_p, C.POINTER(CovBatch)]
    L.cov_finish.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CovSummary)]
    L.cov_fetch_hist.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_copy_depth.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.cov_reset.argtypes = [C.c_void_p]
    L.cov_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.cov_algorithmic_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.cov_last_paths.argtypes = [C.c_void_p, C.POINTER(C.c_uint32 * 6)]
    L.cov_pileup_schedule.argtypes = [C.c_void_p, C.POINTER(C.c_uint32 * 4)]
    L.cov_copy_run_words.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_copy_records.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.cov_set_estimators.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.cov_fetch_estimates.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_set_genomes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.cov_finish_genomes.argtypes = [C.c_void_p, C.POINTER(CovSummary)]
    L.cov_fetch_genome_estimates.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_fetch_genome_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_set_genome_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.cov_genome_entry_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.cov_fetch_genome_entries.argtypes = [C.c_void_p, C.c_void_p]
    L.cov_store_spills.argtypes = [C.c_void_p]
    L.cov_store_spills.restype = C.c_uint32
    L.cov_group_records.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.cov_ingest_want_grouping.argtypes = [C.c_void_p, C.c_int]
    L.cov_interval_reads_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.cov_depth_runs_compute.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.cov_depth_runs_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cov_depth_runs_last.argtypes = [C.c_void_p, C.POINTER(CovDepthRunsInfo)]
    L.cov_depth_bins_compute.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.cov_depth_bins_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cov_depth_bins_last.argtypes = [C.c_void_p, C.POINTER(CovDepthBinsInfo)]
    L.cov_depth_regions_set.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.cov_depth_regions_compute.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.cov_depth_regions_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cov_depth_regions_last.argtypes = [C.c_void_p, C.POINTER(CovDepthRegionsInfo)]
    L.cov_depth_class_runs_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.cov_depth_thresholds_set.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.cov_depth_regions_counts_fetch.argtypes = [C.c_void_p, C.c_void_p]
    _lib = L
    return L


class CovError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("covermhip status %d: %s" % (status, message))
        self.status = status
        self.message = message
