"""Thin Python face of a covermhip session (one sample on one GPU).

Mirrors the C ABI 1:1 — create / set_targets / push / finish / fetch_hist / copy_depth — and adds
nothing of its own: the statistics come from the HIP kernels.  Host arrays are numpy; device arrays
may be anything exposing `data_ptr()` (torch tensors), which is how bench.py hands over HBM-resident
batches without a copy.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import native
from .native import CovBatch, CovConfig, CovError, CovSummary


@dataclass
class RecordBatch:
    """SoA batch of BAM records in file order (cov_batch)."""
    tid: np.ndarray        # int32
    pos: np.ndarray        # int32
    flag: np.ndarray       # uint16
    mapq: np.ndarray       # uint8
    nm: np.ndarray         # uint32
    nm_kind: np.ndarray    # uint8
    l_seq: np.ndarray      # uint32
    cigar_off: np.ndarray  # uint32, n+1
    cigar: np.ndarray      # uint32

    @property
    def n_records(self):
        return int(self.tid.shape[0])

    @staticmethod
    def from_arrays(tid, pos, flag, mapq, nm, nm_kind, l_seq, cigar_off, cigar):
        a = np.ascontiguousarray
        return RecordBatch(a(tid, np.int32), a(pos, np.int32), a(flag, np.uint16), a(mapq, np.uint8),
                           a(nm, np.uint32), a(nm_kind, np.uint8), a(np.asarray(l_seq).astype(np.uint32)),
                           a(cigar_off, np.uint32), a(cigar, np.uint32))

    def slice(self, lo, hi):
        """Records [lo, hi) sharing the CIGAR array (cigar_off keeps absolute offsets)."""
        return RecordBatch(self.tid[lo:hi], self.pos[lo:hi], self.flag[lo:hi], self.mapq[lo:hi], self.nm[lo:hi],
                           self.nm_kind[lo:hi], self.l_seq[lo:hi], self.cigar_off[lo:hi + 1], self.cigar)


def _ptr(x):
    if isinstance(x, np.ndarray):
        return x.ctypes.data if x.size else None
    return x.data_ptr()  # torch tensor


@dataclass
class FilterConfig:
    """FlagFilter (lib.rs:60-64) + the single-read thresholds of FilterParameters (coverm.rs:1648-1657)."""
    include_improper_pairs: bool = True
    include_supplementary: bool = True
    include_secondary: bool = False
    filter_single: bool = False
    min_mapq: int = 255
    min_aligned_length: int = 0
    min_percent_identity: float = 0.0
    min_aligned_percent: float = 0.0


def make_config(device: int = 0, filt: Optional[FilterConfig] = None, contig_end_exclusion: int = 75,
                want_hist: bool = False, want_identity=False) -> CovConfig:
    """cov_config from a FilterConfig.  want_identity: False, True (both sums) or "primary" / "nonsupp"."""
    filt = filt or FilterConfig()
    cfg = CovConfig()
    cfg.device = device
    cfg.include_improper_pairs = int(filt.include_improper_pairs)
    cfg.include_supplementary = int(filt.include_supplementary)
    cfg.include_secondary = int(filt.include_secondary)
    cfg.filter_single = int(filt.filter_single)
    cfg.min_mapq = filt.min_mapq
    cfg.min_aligned_length = filt.min_aligned_length
    cfg.min_percent_identity = filt.min_percent_identity
    cfg.min_aligned_percent = filt.min_aligned_percent
    cfg.contig_end_exclusion = contig_end_exclusion
    cfg.want = (native.WANT_HIST if want_hist else 0) | (native.WANT_IDENTITY if want_identity else 0)
    if want_identity == "primary":
        cfg.want |= native.WANT_IDENTITY_PRIMARY_ONLY
    elif want_identity == "nonsupp":
        cfg.want |= native.WANT_IDENTITY_NONSUPP_ONLY
    return cfg


class Session:
    def __init__(self, device: int = 0, filt: Optional[FilterConfig] = None, contig_end_exclusion: int = 75,
                 want_hist: bool = False, want_identity: bool = False):
        self._lib = native.lib()
        cfg = make_config(device, filt, contig_end_exclusion, want_hist, want_identity)
        self.cfg = cfg
        self._h = C.c_void_p()
        st = self._lib.cov_create(C.byref(cfg), C.byref(self._h))
        if st != native.COV_OK:
            raise CovError(st, self._lib.cov_last_error(None).decode())
        self.n_targets = 0
        self.target_len = None
        self._keep = []   # host/device arrays that must outlive the pushes
        self.summary = None
        self.stats = None

    # -- lifecycle
    def close(self):
        if self._h:
            self._lib.cov_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st):
        if st != native.COV_OK:
            raise CovError(st, self._lib.cov_last_error(self._h).decode())

    # -- ABI
    def set_targets(self, target_len, mask=None):
        tl = np.ascontiguousarray(target_len, dtype=np.uint64)
        self._check(self._lib.cov_set_targets(self._h, len(tl), tl.ctypes.data if len(tl) else None))
        self.n_targets = len(tl)
        self.target_len = tl
        self._runs = False                         # (cov_set_targets and cov_set_target_mask turn genomes and runs off)
        self._n_regions, self._region_tids = 0, np.zeros(0, np.int64)      # (and cov_set_targets drops the depth regions)
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert len(m) == len(tl)
            self._check(self._lib.cov_set_target_mask(self._h, m.ctypes.data if len(m) else None))

    def _batch(self, b, n=None):
        cb = CovBatch()
        for k in ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq", "cigar_off", "cigar"):
            setattr(cb, k, _ptr(getattr(b, k) if not isinstance(b, dict) else b[k]))
        cb.n_records = n if n is not None else b.n_records
        return cb

    def push(self, batch: RecordBatch):
        cb = self._batch(batch)
        self._check(self._lib.cov_push_batch(self._h, C.byref(cb)))

    def push_device(self, tensors: dict, n_records: int):
        """`tensors`: dict of device arrays (torch) with the cov_batch field names; adopted without a copy."""
        self._keep.append(tensors)
        cb = self._batch(tensors, n_records)
        self._check(self._lib.cov_push_batch_device(self._h, C.byref(cb)))

    def reset(self):
        self._check(self._lib.cov_reset(self._h))
        self._keep.clear()

    def finish(self):
        stats = np.empty(self.n_targets, dtype=native.CONTIG_STATS_DTYPE)      # (cov_finish writes every entry)
        summ = CovSummary()
        self._check(self._lib.cov_finish(self._h, stats.ctypes.data if self.n_targets else None, C.byref(summ)))
        self.stats = stats
        self.summary = summ
        return stats, summ

    def hist(self):
        n = int(self.summary.hist_total)
        h = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.cov_fetch_hist(self._h, h.ctypes.data if n else None))
        return h

    def depth(self, tid: int):
        d = np.zeros(int(self.target_len[tid]), dtype=np.int32)
        self._check(self._lib.cov_copy_depth(self._h, tid, d.ctypes.data if d.size else None))
        return d

    def depth_runs(self, tid_lo: int = 0, tid_hi: Optional[int] = None, chunks=None, _cuts=None):
        """cov_depth_runs_compute / cov_depth_runs_fetch over targets [tid_lo, tid_hi) (default: all), chunk by chunk: the per-base depth
        run-length encoded on the device.  Returns (run_off, start, depth): the runs of target tid_lo + k are entries
        run_off[k] .. run_off[k + 1] (uint64, tid_hi - tid_lo + 1 entries), start[j] the run's first base (uint32, 0-based, inside its
        target), depth[j] its depth (int32); a run ends where the next one of its target starts, or at the target's length.  `chunks`: a
        list that receives one dict per chunk (cov_depth_runs_info: tid_lo, tid_next, arena_bases, n_runs, arena_ms, runs_ms)."""
        hi = self.n_targets if tid_hi is None else int(tid_hi)
        lo = int(tid_lo)
        offs, parts, base = [np.zeros(1, dtype=np.uint64)], [], 0
        while lo < hi:
            nxt, n = C.c_uint32(0), C.c_uint64(0)
            if _cuts is None:
                self._check(self._lib.cov_depth_runs_compute(self._h, C.c_uint32(lo), C.c_uint32(hi), C.byref(nxt), C.byref(n)))
            else:      # (depth_class_runs: the same chunks, fetch and info)
                self._check(self._lib.cov_depth_class_runs_compute(self._h, _cuts.ctypes.data if _cuts.size else None, C.c_uint32(_cuts.size), C.c_uint32(lo),
                                                                   C.c_uint32(hi), C.byref(nxt), C.byref(n)))
            ro = np.zeros(nxt.value - lo + 1, dtype=np.uint64)
            runs = np.zeros(int(n.value), dtype=native.DEPTH_RUN_DTYPE)
            self._check(self._lib.cov_depth_runs_fetch(self._h, ro.ctypes.data, runs.ctypes.data if runs.size else None))
            if chunks is not None:
                info = native.CovDepthRunsInfo()
                self._check(self._lib.cov_depth_runs_last(self._h, C.byref(info)))
                chunks.append({k: getattr(info, k) for k, _ in info._fields_})
            offs.append(ro[1:] + np.uint64(base))
            parts.append(runs)
            base += int(n.value)
            lo = nxt.value
        runs = np.concatenate(parts) if parts else np.zeros(0, dtype=native.DEPTH_RUN_DTYPE)
        return np.concatenate(offs), np.ascontiguousarray(runs["start"]), np.ascontiguousarray(runs["depth"])

    @staticmethod
    def _cut_list(values):
        """A cut list as the int32 array the library validates (a value outside int32 cannot be one: refused here)."""
        a = np.asarray(list(values), dtype=np.int64).reshape(-1)
        if ((a < -2 ** 31) | (a > 2 ** 31 - 1)).any():
            raise ValueError("a cut is outside the 32-bit range")
        return np.ascontiguousarray(a.astype(np.int32))

    def depth_class_runs(self, cuts, tid_lo: int = 0, tid_hi: Optional[int] = None, chunks=None):
        """cov_depth_class_runs_compute / cov_depth_runs_fetch over targets [tid_lo, tid_hi) (default: all), chunk by chunk: the per-base
        depth classified against `cuts` (1 .. 16 ascending values in 0 .. 2^31 - 1; the class of a depth d is the number of cuts <= d) and
        run-length encoded by class on the device.  Returns (run_off, start, cls), the shape depth_runs returns: every class is there,
        0 and len(cuts) included.  `chunks` as for depth_runs."""
        return self.depth_runs(tid_lo, tid_hi, chunks, _cuts=self._cut_list(cuts))

    def depth_runs_kernel_ms(self):
        """(ms, launches) of the run kernels of the last chunk of depth_runs or depth_class_runs (COV_K_DEPTH_RUNS)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_DEPTH_RUNS, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def depth_bins(self, bin_size: int, tid_lo: int = 0, tid_hi: Optional[int] = None, chunks=None):
        """cov_depth_bins_compute / cov_depth_bins_fetch over targets [tid_lo, tid_hi) (default: all), chunk by chunk: the per-base depth
        reduced over windows of `bin_size` bases on the device.  Returns (bin_off, bins): the bins of target tid_lo + k are entries
        bin_off[k] .. bin_off[k + 1] (uint64, tid_hi - tid_lo + 1 entries) of `bins`, a structured array (native.DEPTH_BIN_DTYPE: sum, min,
        max, covered); bin b of a target covers bases [b * bin_size, min((b + 1) * bin_size, length)).  `chunks`: a list that receives one
        dict per chunk (cov_depth_bins_info: tid_lo, tid_next, arena_bases, n_bins, arena_ms, bins_ms, bin_size)."""
        if not 0 <= int(bin_size) <= 0xffffffff:
            raise ValueError("bin_size out of range")
        hi = self.n_targets if tid_hi is None else int(tid_hi)
        lo = int(tid_lo)
        offs, parts, base = [np.zeros(1, dtype=np.uint64)], [], 0
        while lo < hi:
            nxt, n = C.c_uint32(0), C.c_uint64(0)
            self._check(self._lib.cov_depth_bins_compute(self._h, C.c_uint32(int(bin_size)), C.c_uint32(lo), C.c_uint32(hi), C.byref(nxt), C.byref(n)))
            bo = np.zeros(nxt.value - lo + 1, dtype=np.uint64)
            bins = np.zeros(int(n.value), dtype=native.DEPTH_BIN_DTYPE)
            self._check(self._lib.cov_depth_bins_fetch(self._h, bo.ctypes.data, bins.ctypes.data if bins.size else None))
            if chunks is not None:
                info = native.CovDepthBinsInfo()
                self._check(self._lib.cov_depth_bins_last(self._h, C.byref(info)))
                chunks.append({k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"})
            offs.append(bo[1:] + np.uint64(base))
            parts.append(bins)
            base += int(n.value)
            lo = nxt.value
        return np.concatenate(offs), (np.concatenate(parts) if parts else np.zeros(0, dtype=native.DEPTH_BIN_DTYPE))

    def depth_bins_kernel_ms(self):
        """(ms, launches) of the bin kernels of the last chunk of depth_bins (COV_K_DEPTH_BINS): six launches, k_depth_marks, the rank
        scan's three, k_bins_init and k_depth_bins (four for a chunk without a bin)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_DEPTH_BINS, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_depth_regions(self, regions):
        """cov_depth_regions_set: the regions Session.depth_regions reduces, in ANY order, overlaps and duplicates allowed.  `regions`: a
        native.DEPTH_REGION_DTYPE array, or an iterable of (tid, start, end) with 0 <= start < end <= the target's length ([start, end),
        0-based, half open); nothing (or an empty list) clears them.  Needs set_targets; a new set_targets drops them."""
        if isinstance(regions, np.ndarray) and regions.dtype == native.DEPTH_REGION_DTYPE:
            arr = np.ascontiguousarray(regions)
        else:
            rows = list(regions) if regions is not None else []
            arr = np.zeros(len(rows), dtype=native.DEPTH_REGION_DTYPE)
            if rows:
                a = np.asarray(rows, dtype=np.int64).reshape(len(rows), 3)
                if (a < 0).any() or (a > 0xffffffff).any():
                    raise ValueError("a region's tid, start or end is outside 0 .. 2^32 - 1")
                arr["tid"], arr["start"], arr["end"] = a[:, 0], a[:, 1], a[:, 2]
        self._check(self._lib.cov_depth_regions_set(self._h, arr.ctypes.data if arr.size else None, C.c_uint64(arr.size)))
        self._region_tids = np.unique(arr["tid"]).astype(np.int64)
        self._n_regions = int(arr.size)

    def depth_regions(self, chunks=None, _each=None):
        """cov_depth_regions_compute / cov_depth_regions_fetch over the regions of set_depth_regions, chunk by chunk: per region the sum,
        min, max and covered bases of its per-base depth, reduced on the device.  Returns a native.DEPTH_BIN_DTYPE array IN THE ORDER THE
        REGIONS WERE GIVEN.  Targets without a region are skipped: a chunk begins at the first target at or behind the last chunk's
        tid_next that has a region, so only those chunks' depth is materialised.  `chunks`: a list that receives one dict per chunk
        actually computed (cov_depth_regions_info: tid_lo, tid_next, arena_bases, n_regions, n_pieces, arena_ms, regions_ms)."""
        n = getattr(self, "_n_regions", 0)
        tids = getattr(self, "_region_tids", np.zeros(0, np.int64))
        out = np.zeros(n, dtype=native.DEPTH_BIN_DTYPE)
        hi = self.n_targets
        if n == 0:      # nothing set: the call refuses with its own words
            nxt, m = C.c_uint32(0), C.c_uint64(0)
            self._check(self._lib.cov_depth_regions_compute(self._h, C.c_uint32(0), C.c_uint32(hi), C.byref(nxt), C.byref(m)))
            return out
        at = 0
        while at < len(tids):
            lo = int(tids[at])
            nxt, m = C.c_uint32(0), C.c_uint64(0)
            self._check(self._lib.cov_depth_regions_compute(self._h, C.c_uint32(lo), C.c_uint32(hi), C.byref(nxt), C.byref(m)))
            idx = np.zeros(int(m.value), dtype=np.uint64)
            res = np.zeros(int(m.value), dtype=native.DEPTH_BIN_DTYPE)
            self._check(self._lib.cov_depth_regions_fetch(self._h, idx.ctypes.data if idx.size else None, res.ctypes.data if res.size else None))
            out[idx.astype(np.int64)] = res
            if _each is not None:      # (depth_region_counts: the chunk's counts, while the chunk is there)
                _each(idx)
            if chunks is not None:
                info = native.CovDepthRegionsInfo()
                self._check(self._lib.cov_depth_regions_last(self._h, C.byref(info)))
                chunks.append({k: getattr(info, k) for k, _ in info._fields_})
            at = int(np.searchsorted(tids, nxt.value, side="left"))
        return out

    def set_depth_thresholds(self, thr):
        """cov_depth_thresholds_set: the thresholds depth_region_counts counts (1 .. 16 ascending values in 0 .. 2^31 - 1); nothing (or an
        empty list) clears them.  Valid any time; kept over set_targets, reset and finish."""
        arr = self._cut_list(thr if thr is not None else [])
        self._check(self._lib.cov_depth_thresholds_set(self._h, arr.ctypes.data if arr.size else None, C.c_uint32(arr.size)))
        self._n_thr = int(arr.size)

    def depth_region_counts(self, chunks=None):
        """depth_regions with the thresholds of set_depth_thresholds: returns (bins, counts), both IN THE ORDER THE REGIONS WERE GIVEN;
        bins is what depth_regions returns, counts[i, j] (uint32, shape (n_regions, K)) the bases of region i with depth >= threshold j."""
        k = getattr(self, "_n_thr", 0)
        counts = np.zeros((getattr(self, "_n_regions", 0), k), dtype=np.uint32)

        def take(idx):
            part = np.zeros((len(idx), k), dtype=np.uint32)
            self._check(self._lib.cov_depth_regions_counts_fetch(self._h, part.ctypes.data if part.size else None))
            counts[idx.astype(np.int64)] = part
        bins = self.depth_regions(chunks=chunks, _each=take)
        if counts.shape[0] == 0:      # (no chunk ran: the fetch refuses with its own words when no thresholds are set)
            self._check(self._lib.cov_depth_regions_counts_fetch(self._h, None))
        return bins, counts

    def depth_regions_kernel_ms(self):
        """(ms, launches) of the region kernels of the last chunk of depth_regions (COV_K_DEPTH_REGIONS): six launches, k_depth_marks, the
        rank scan's three, k_bins_init and k_depth_regions (four for a chunk without a region).  With thresholds set the launches are the
        same six (or four): k_depth_regions_thr takes k_depth_regions' place, and the counts are zeroed by a fill, which is no launch."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_DEPTH_REGIONS, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_estimators(self, estimators):
        """cov_set_estimators: CoverageEstimator::calculate_coverage of every contig on the device at each finish (contig mode).
        `estimators`: coverm_amd.host.CoverageEstimator structures (same layout as cov_estimator); [] turns it off."""
        n = len(estimators)
        arr = (type(estimators[0]) * n)(*estimators) if n else None
        self._n_est = n
        self._check(self._lib.cov_set_estimators(self._h, arr, C.c_uint32(n)))

    def estimates(self):
        """cov_fetch_estimates: n_targets x n_estimators f32 of the last finish."""
        out = np.empty((self.n_targets, getattr(self, "_n_est", 0)), dtype=np.float32)
        self._check(self._lib.cov_fetch_estimates(self._h, out.ctypes.data if out.size else None))
        return out

    def set_genomes(self, genome_of_tid, n_genomes: int):
        """cov_set_genomes (after set_targets): genome_of_tid[t] = genome of target t, -1 = outside every genome.  Implies the target mask;
        with estimators set, every finish then also aggregates the contigs into genomes and evaluates the estimators per genome on the
        device.  None / n_genomes = 0 turns it off."""
        self._runs = False
        if genome_of_tid is None or n_genomes == 0:
            self._n_genomes = 0
            self._check(self._lib.cov_set_genomes(self._h, None, C.c_uint32(0)))
            return
        g = np.ascontiguousarray(genome_of_tid, dtype=np.int32)
        assert len(g) == self.n_targets
        self._n_genomes = int(n_genomes)
        self._check(self._lib.cov_set_genomes(self._h, g.ctypes.data if len(g) else None, C.c_uint32(n_genomes)))

    def set_genome_runs(self, gid_of_tid, n_gids: int):
        """cov_set_genome_runs (after set_targets): gid_of_tid[t] >= 0 = dense id of target t's genome (the name's prefix before the
        separator; all 0 in single-genome mode).  With estimators set, every finish then builds the entries of the separator /
        single-genome scan on the device and evaluates the estimators per entry: genome_entries(), genome_estimates().  Sets no mask
        and turns set_genomes off; None / n_gids = 0 turns it off."""
        self._n_genomes = 0
        if gid_of_tid is None or n_gids == 0:
            self._runs = False
            self._check(self._lib.cov_set_genome_runs(self._h, None, C.c_uint32(0)))
            return
        g = np.ascontiguousarray(gid_of_tid, dtype=np.int32)
        assert len(g) == self.n_targets
        self._check(self._lib.cov_set_genome_runs(self._h, g.ctypes.data if len(g) else None, C.c_uint32(n_gids)))
        self._runs = True

    def genome_entry_count(self) -> int:
        """cov_genome_entry_count: entries of the last finish (set_genome_runs)."""
        n = C.c_uint32(0)
        self._check(self._lib.cov_genome_entry_count(self._h, C.byref(n)))
        return n.value

    def genome_entries(self):
        """cov_fetch_genome_entries: one native.GENOME_ENTRY_DTYPE entry per entry of the scan, in the order it prints them."""
        out = np.zeros(self.genome_entry_count(), dtype=native.GENOME_ENTRY_DTYPE)
        self._check(self._lib.cov_fetch_genome_entries(self._h, out.ctypes.data if out.size else None))
        return out

    def finish_genomes(self):
        """cov_finish_genomes: the pipeline and its verdicts without the per-contig statistics (genomes and estimators set)."""
        summ = CovSummary()
        self._check(self._lib.cov_finish_genomes(self._h, C.byref(summ)))
        self.summary = summ
        return summ

    def genome_estimates(self):
        """cov_fetch_genome_estimates: n_genomes (set_genomes) or n_entries (set_genome_runs) x n_estimators f32 of the last finish."""
        n = self.genome_entry_count() if getattr(self, "_runs", False) else getattr(self, "_n_genomes", 0)
        out = np.empty((n, getattr(self, "_n_est", 0)), dtype=np.float32)
        self._check(self._lib.cov_fetch_genome_estimates(self._h, out.ctypes.data if out.size else None))
        return out

    def genome_stats(self):
        """cov_fetch_genome_stats: one native.GENOME_STATS_DTYPE entry per genome."""
        out = np.zeros(getattr(self, "_n_genomes", 0), dtype=native.GENOME_STATS_DTYPE)
        self._check(self._lib.cov_fetch_genome_stats(self._h, out.ctypes.data if out.size else None))
        return out

    def genome_kernel_ms(self):
        """(ms, launches) of the genome kernels of the last finish (COV_K_GENOME)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_GENOME, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def group_records(self):
        """cov_group_records: the records of every reference made contiguous on the device (stable: references in ascending tid order, records
        without a reference last, the file's order kept inside a reference), for a sample that is not sorted by reference.  Between the
        last push / ingest and the pair filter / finish.  Returns the number of records whose index changed (0: the store was grouped
        already and was left alone)."""
        n = C.c_uint64(0)
        self._check(self._lib.cov_group_records(self._h, C.byref(n)))
        return int(n.value)

    def sep_kernel_ms(self):
        """(ms, launches) of the kernels that built the separator entries' table in the last finish (COV_K_SEP, set_genome_runs)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_SEP, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def group_kernel_ms(self):
        """(ms, launches) of the last group_records (COV_K_GROUP)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_GROUP, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def interval_reads(self, intervals, want_identity=False):
        """cov_interval_reads_compute: the per-gene read aggregates of --gff from the session's own record store (before or after finish).
        `intervals`: (tid, start, end) triples, 0-based half-open.  Returns (reads, mapped_total, sorted_by_start): `reads` a
        native.INTERVAL_READS_DTYPE array (n_reads, mismatches, sum_identity, contig_taken), or None when sorted_by_start is False (a start
        decreases inside a reference: nothing was computed, the host's record pass takes such a sample).  Raises CovError with the
        reference's own verdicts (COV_ERR_NM_* / COV_ERR_UNSORTED / COV_ERR_BAD_TID) and COV_ERR_STATE after a spill."""
        iv = np.zeros(len(intervals), dtype=native.INTERVAL_DTYPE)
        for k, (t, a, b) in enumerate(intervals):
            iv[k] = (t, 0, a, b)
        out = np.zeros(len(iv), dtype=native.INTERVAL_READS_DTYPE)
        mapped, srt = C.c_uint64(0), C.c_int(0)
        self._check(self._lib.cov_interval_reads_compute(self._h, iv.ctypes.data if len(iv) else None, C.c_uint64(len(iv)), C.c_int(1 if want_identity else 0),
                                                         out.ctypes.data if len(iv) else None, C.byref(mapped), C.byref(srt)))
        return (out if srt.value else None), int(mapped.value), bool(srt.value)

    def gene_reads_kernel_ms(self):
        """(ms, launches) of the kernels of the last interval_reads (COV_K_GENE_READS)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_GENE_READS, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sam_ingest(self, path_or_fileobj, mates=False, group=False):
        """SAM text decoded on the device into this session's store (cov_sam_*): a path, "-" for standard input, or an object with fileno().
        Sets the targets from the @SQ lines; returns (ref_names, ref_lens, n_records, timing dict) — see coverm_amd.bam.sam_ingest."""
        from . import bam
        return bam.sam_ingest(self, path_or_fileobj, want_mates=mates, group=group)

    def sam_kernel_ms(self):
        """(ms, launches) of the decode kernels of the last SAM text ingest (COV_K_SAM)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(self._lib.cov_kernel_ms(self._h, native.K_SAM, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def store_spills(self):
        return int(self._lib.cov_store_spills(self._h))

    def kernel_ms(self):
        out = {}
        for k, name in native.KERNEL_NAMES.items():
            ms = C.c_double(0)
            n = C.c_uint32(0)
            self._check(self._lib.cov_kernel_ms(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def last_paths(self):
        """cov_last_paths: which branches of the device pipeline the last finish took (diagnostics for the parity tests)."""
        v = (C.c_uint32 * 6)()
        self._check(self._lib.cov_last_paths(self._h, C.byref(v)))
        return dict(listed_steps=int(v[0]), generic_only=bool(v[1]), slow_tiles=int(v[2]), bucket_records=int(v[3]),
                    bucket_entries=int(v[4]), passes=int(v[5]))

    def pileup_schedule(self):
        """cov_pileup_schedule: how the last finish handed k_pileup_fast's tiles to its waves: tiles on the deep-tile list (0: none used),
        waves launched, tiles per chunk, the list's threshold (COVERM_KNOBS pileup_deep_min)."""
        v = (C.c_uint32 * 4)()
        self._check(self._lib.cov_pileup_schedule(self._h, C.byref(v)))
        return dict(deep_tiles=int(v[0]), waves=int(v[1]), chunk_tiles=int(v[2]), deep_min=int(v[3]))

    def run_words(self):
        """cov_copy_run_words: the run word k_prep left for every record of the store in the last finish, as uint64 (x | y << 32).  Raises
        CovError (COV_ERR_STATE) when there are none for the whole store: no records, an adopted device batch, a spilled store."""
        n = C.c_uint64(0)
        self._check(self._lib.cov_copy_records(self._h, None, C.byref(n), None))      # (how many records the store holds)
        out = np.zeros(max(1, int(n.value)), dtype=np.uint64)
        self._check(self._lib.cov_copy_run_words(self._h, out.ctypes.data_as(C.c_void_p)))
        return out[:int(n.value)]

    def algorithmic_bytes(self):
        b = C.c_uint64(0)
        self._check(self._lib.cov_algorithmic_bytes(self._h, C.byref(b)))
        return int(b.value)
