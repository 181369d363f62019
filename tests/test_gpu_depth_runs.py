"""Depth runs on the device (cov_depth_runs_compute / cov_depth_runs_fetch through Session.depth_runs): the runs equal the run-length
encoding of np.cumsum(O.contig_deltas(...)) — the oracle depth tests/test_gpu_abi_parity.py compares Session.depth with — on the synthetic
shapes of tests/depth_runs_ref.py built as real records and on the reference's fixture files, under the default flags and under a reader
filter; forced chunks of 2 048 bases give the same runs and offsets; the contig block on the device is untouched; a spilled store is refused;
and the runs integrate to the full-length depth sum."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd.engine import CovSummary, FilterConfig, RecordBatch, Session
from coverm_amd import native
from coverm_amd.native import CovError, ERR_STATE
from oracle import bamio
from oracle import oracle as O
from oracle.bamio import BamData
from tests import depth_runs_ref as R
from tests.knobs import set_knobs
from tests.test_depth_runs_core import plan_ref

pytestmark = pytest.mark.gpu

RAW = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw")
FIXTURES = sorted(f for f in os.listdir(RAW) if f.endswith(".bam") and "unsorted" not in f)
SMALL = [f for f in FIXTURES if f != "eg2.bam"]      # (eg2: 54 579 references, 7 * 10^8 bases — one pass with the default chunk)


def records_for(depths):
    """Reads (one M run each) whose pileup is exactly `depths`: level k of a target is covered by one read per stretch with depth >= k."""
    tid, pos, ln = [], [], []
    for t, d in enumerate(depths):
        for k in range(1, int(d.max()) + 1 if d.size else 1):
            edge = np.diff(np.concatenate([[0], (d >= k).astype(np.int8), [0]]))
            s, e = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
            tid.append(np.full(len(s), t)); pos.append(s); ln.append(e - s)
    cat = lambda x: np.concatenate(x).astype(np.int64) if x else np.zeros(0, np.int64)
    tid, pos, ln = cat(tid), cat(pos), cat(ln)
    o = np.lexsort((pos, tid))
    tid, pos, ln = tid[o], pos[o], ln[o]
    n = len(tid)
    z = np.zeros(n, np.int32)
    return BamData(["s%d" % t for t in range(len(depths))], np.asarray([len(d) for d in depths], np.int64), tid.astype(np.int32), pos.astype(np.int32),
                   np.zeros(n, np.uint16), np.full(n, 40, np.uint8), np.minimum(ln, 1 << 20).astype(np.int32), np.zeros(n, np.uint32), np.ones(n, np.uint8),
                   np.arange(n + 1, dtype=np.uint32), ((ln << 4) | 0).astype(np.uint32), z - 1, z - 1, z, [b"r%d" % i for i in range(n)], "")


def to_batch(b):
    return RecordBatch.from_arrays(b.tid, b.pos, b.flag, b.mapq, b.nm, b.nm_kind, b.l_seq, b.cigar_off, b.cigar)


def oracle_depths(b, ff, ofp=None):
    """Per-target oracle depth; a target without a record is all zero (not asked of the oracle: eg2 has 54 579 of them)."""
    order, _ = O.reader_stage(b, ofp)
    touched = set(int(t) for t in np.unique(b.tid) if 0 <= t < len(b.ref_lens))
    return [np.cumsum(O.contig_deltas(b, ff, t, order), dtype=np.int64).astype(np.int32) if t in touched else np.zeros(int(L), np.int32)
            for t, L in enumerate(b.ref_lens)]


def device_block(s):
    """The [DevGlobal][DevContig x n] block as it lies on the device now, decoded as cov_finish decodes it (cov_gather of one rank: plain copies)."""
    L = s._lib
    L.cov_gather.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32]
    L.cov_gathered.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(CovSummary)]
    arr = (C.c_void_p * 1)(s._h)
    s._check(L.cov_gather(arr, 1, 0))
    st = np.zeros(s.n_targets, native.CONTIG_STATS_DTYPE)
    summ = CovSummary()
    s._check(L.cov_gathered(s._h, 0, st.ctypes.data if s.n_targets else None, C.byref(summ)))
    return st


def check(b, ff=(True, True, False), fp=None, also_chunked=None, monkeypatch=None):
    off = O.FlagFilter(*ff)
    ofp, filt = None, FilterConfig(*ff)
    if fp is not None:
        ofp = O.FilterParameters(off, **fp)
        filt = FilterConfig(*ff, filter_single=True, min_mapq=ofp.min_mapq, min_aligned_length=ofp.min_aligned_length_single,
                            min_percent_identity=ofp.min_percent_identity_single, min_aligned_percent=ofp.min_aligned_percent_single)
    depths = oracle_depths(b, off, ofp)
    want_off, want_start, want_depth = R.runs_of(depths)
    results = []
    for budget in [None] + ([also_chunked] if also_chunked else []):
        if budget:
            set_knobs(monkeypatch, depth_chunk_bases=budget)      # read by cov_create
        with Session(0, filt, 0) as s:
            s.set_targets(b.ref_lens)
            s.push(to_batch(b))
            st, _ = s.finish()
            before = device_block(s)
            chunks = []
            run_off, start, depth = s.depth_runs(chunks=chunks)
            after = device_block(s)
            assert before.tobytes() == after.tobytes()      # the pileup ran against the scratch copy
            for f in ("n_pass", "win_sum_d", "win_sum_d2", "full_covered", "win_max_d"):
                np.testing.assert_array_equal(after[f], st[f], err_msg=f)
            ms, launches = s.depth_runs_kernel_ms()
            assert launches == 7 and ms > 0
            if budget:      # the chunks are the planner's (tests/test_depth_runs_core.py checks it against this restatement)
                assert [c["tid_next"] for c in chunks] == plan_ref([int(L) for L in b.ref_lens], budget)
            assert chunks[0]["tid_lo"] == 0 and chunks[-1]["tid_next"] == len(b.ref_lens) and sum(c["n_runs"] for c in chunks) == len(start)
            # a sub-range answers for its targets alone
            if len(b.ref_lens) >= 3:
                o2, s2, d2 = s.depth_runs(1, len(b.ref_lens) - 1)
                lo, hi = int(want_off[1]), int(want_off[len(b.ref_lens) - 1])
                np.testing.assert_array_equal(o2, want_off[1:len(b.ref_lens)] - want_off[1])
                np.testing.assert_array_equal(s2, want_start[lo:hi]); np.testing.assert_array_equal(d2, want_depth[lo:hi])
        np.testing.assert_array_equal(run_off, want_off)
        np.testing.assert_array_equal(start, want_start)
        np.testing.assert_array_equal(depth, want_depth)
        # the track integrates to the table: sum of depth * (end - start) per target = the full-length depth sum of cov_finish
        # (contig_end_exclusion 0: the window is the whole target)
        nxt = np.append(start[1:], 0).astype(np.int64)
        last = np.zeros(len(start), bool)
        last[(run_off[1:][run_off[1:] > run_off[:-1]] - 1).astype(np.int64)] = True
        owner = np.repeat(np.arange(len(b.ref_lens)), np.diff(run_off.astype(np.int64)))
        end = np.where(last, np.asarray(b.ref_lens, np.int64)[owner], nxt)
        area = np.bincount(owner, weights=None if not len(start) else depth.astype(np.int64) * (end - start), minlength=len(b.ref_lens)).astype(np.uint64)
        np.testing.assert_array_equal(area, st["win_sum_d"])
        results.append((run_off, start, depth))
    if also_chunked:
        for a, c in zip(results[0], results[1]):
            assert a.dtype == c.dtype and a.tobytes() == c.tobytes()


@pytest.fixture(scope="module")
def shape_records():
    return {name: records_for(depths) for name, depths in R.shapes().items()}


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_synthetic_shapes(shape_records, name, monkeypatch):
    b = shape_records[name]
    intended = R.shapes()[name]
    got = oracle_depths(b, O.FlagFilter(True, True, False))
    assert all((g == w).all() for g, w in zip(got, intended)), "the records do not pile up to the shape"
    check(b, also_chunked=2048, monkeypatch=monkeypatch)


@pytest.mark.parametrize("name", SMALL)
def test_fixture_default_flags(name, monkeypatch):
    check(bamio.read_bam(os.path.join(RAW, name)), also_chunked=2048, monkeypatch=monkeypatch)


def test_fixture_of_54579_references():
    check(bamio.read_bam(os.path.join(RAW, "eg2.bam")))


@pytest.mark.parametrize("name,ff,fp", [("2seqs.bad_read.1.bam", (True, True, True), dict(min_percent_identity_single=0.99)),
                                        ("k141_2005182.head11.bam", (True, True, True), dict(min_percent_identity_single=float(np.float32(0.97001)))),
                                        ("2seqs.bad_read.1.with_supplementary.bam", (True, False, False), None),
                                        ("7seqs.reads_for_seq1_and_seq2.bam", (False, True, True), None)])
def test_fixture_filters(name, ff, fp, monkeypatch):
    check(bamio.read_bam(os.path.join(RAW, name)), ff=ff, fp=fp, also_chunked=2048, monkeypatch=monkeypatch)


def test_states(monkeypatch):
    b = bamio.read_bam(os.path.join(RAW, "7seqs.reads_for_seq1_and_seq2.bam"))
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        with pytest.raises(CovError) as ei:      # before a finish
            s.depth_runs()
        assert ei.value.status == ERR_STATE
        s.finish()
        ro = np.zeros(8, np.uint64)
        assert s._lib.cov_depth_runs_fetch(s._h, ro.ctypes.data, None) == ERR_STATE      # no chunk computed yet
        nxt, n = C.c_uint32(0), C.c_uint64(0)
        assert s._lib.cov_depth_runs_compute(s._h, 3, 3, C.byref(nxt), C.byref(n)) == native.ERR_INVALID_ARG
        assert s._lib.cov_depth_runs_compute(s._h, 0, 8, C.byref(nxt), C.byref(n)) == native.ERR_INVALID_ARG
        s.depth_runs()
        s.finish()                                # a new finish drops the chunk
        assert s._lib.cov_depth_runs_fetch(s._h, ro.ctypes.data, None) == ERR_STATE


def test_spilled_store_is_refused(monkeypatch):
    from coverm_amd import synth
    set_knobs(monkeypatch, store_cap_records=10000, store_cap_cigar=100000)
    ref = synth.make_reference(12, 200_000, seed=3, min_len=1500, max_len=40_000)
    batch = synth.make_reads(ref, 30_000, seed=4)
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(ref.lengths)
        for lo in range(0, batch.n_records, 997):
            s.push(batch.slice(lo, min(batch.n_records, lo + 997)))
        s.finish()
        assert s.store_spills() >= 1
        with pytest.raises(CovError) as ei:
            s.depth_runs()
        assert ei.value.status == ERR_STATE and "already left the bounded record store" in ei.value.message
