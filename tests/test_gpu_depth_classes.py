"""Depth classes on the device: the quantised runs (cov_depth_class_runs_compute through Session.depth_class_runs) equal the run-length
encoding of numpy's searchsorted over the oracle depth, and the threshold counts of the regions (cov_depth_thresholds_set /
cov_depth_regions_counts_fetch through Session.set_depth_thresholds / depth_region_counts) equal (slice >= t).sum(), in input order — on
the synthetic shapes of tests/depth_runs_ref.py and tests/depth_classes_ref.py built as real records, with the region sets of
tests/depth_regions_ref.py, and on the reference's fixture files under the default flags and under a reader filter.  All integers,
compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from coverm_amd import native
from coverm_amd.native import CovError, ERR_INVALID_ARG, ERR_STATE
from oracle import bamio
from oracle import oracle as O
from tests import depth_classes_ref as K
from tests import depth_regions_ref as G
from tests import depth_runs_ref as R
from tests.knobs import set_knobs
from tests.test_depth_runs_core import plan_ref
from tests.test_gpu_depth_runs import RAW, device_block, oracle_depths, records_for, to_batch

pytestmark = pytest.mark.gpu

W = G.W
SHAPES = K.shapes()
RUN_LISTS = ("MIXED", "ZERO_ONE", "ONE", "TOP")
K16 = tuple(range(0, 32, 2))      # sixteen thresholds, 0 first


def open_session(b, filt=None):
    s = Session(0, filt or FilterConfig(), 0)
    s.set_targets(b.ref_lens)
    s.push(to_batch(b))
    return s


@pytest.fixture(scope="module")
def shape_records():
    return {name: records_for(depths) for name, depths in SHAPES.items()}


@pytest.fixture(scope="module")
def class_wants():
    """name -> cut list -> (run_off, start, cls): computed once, shared, never changed."""
    return {name: {c: K.class_runs_of(depths, K.CUT_LISTS[c]) for c in RUN_LISTS + ("UNIT",)} for name, depths in SHAPES.items()}


def assert_runs(got, want, msg):
    for g, w, dt in zip(got, want, (np.uint64, np.uint32, np.int32)):
        assert g.dtype == dt, msg
        np.testing.assert_array_equal(g, w, err_msg=msg)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_class_runs_of_the_shapes(shape_records, class_wants, name):
    b, depths = shape_records[name], SHAPES[name]
    got = oracle_depths(b, O.FlagFilter(True, True, False))
    assert all((g == w).all() for g, w in zip(got, depths)), "the records do not pile up to the shape"
    with open_session(b) as s:
        st, _ = s.finish()
        before = device_block(s)
        for c in RUN_LISTS:
            chunks = []
            res = s.depth_class_runs(K.CUT_LISTS[c], chunks=chunks)
            assert_runs(res, class_wants[name][c], "%s %s" % (name, c))
            ms, launches = s.depth_runs_kernel_ms()
            assert launches == 7 and ms > 0
            assert len(chunks) == 1 and chunks[0]["n_runs"] == len(res[1]) and chunks[0]["tid_next"] == len(depths)
        after = device_block(s)
        assert before.tobytes() == after.tobytes()      # the pileup ran against the scratch copy
        # covered or not: the class-2 stretches of a target sum to the table's covered bases
        off, start, cls = s.depth_class_runs(K.ZERO_ONE)
        assert not (cls == 0).any()
        for t, d in enumerate(depths):
            lo, hi = int(off[t]), int(off[t + 1])
            end = np.append(start[lo + 1:hi], len(d)).astype(np.int64)[:hi - lo]
            assert int(((end - start[lo:hi]) * (cls[lo:hi] == 2)).sum()) == int(st["full_covered"][t]), (name, t)
        # class = depth + 1: the class runs are the depth runs
        if all(int(np.max(d, initial=0)) <= 14 for d in depths):
            uo, us, uc = s.depth_class_runs(K.UNIT)
            do, ds, dd = s.depth_runs()
            assert uo.tobytes() == do.tobytes() and us.tobytes() == ds.tobytes() and (uc == dd + 1).all()
        else:      # (depths of 15 and more share the last class)
            assert_runs(s.depth_class_runs(K.UNIT), class_wants[name]["UNIT"], name + " UNIT")
        # a sub-range answers for its targets alone
        if len(depths) >= 3:
            wo, ws, wc = class_wants[name]["MIXED"]
            o2, s2, c2 = s.depth_class_runs(K.MIXED, 1, len(depths) - 1)
            lo, hi = int(wo[1]), int(wo[len(depths) - 1])
            np.testing.assert_array_equal(o2, wo[1:len(depths)] - wo[1])
            np.testing.assert_array_equal(s2, ws[lo:hi]); np.testing.assert_array_equal(c2, wc[lo:hi])


@pytest.mark.parametrize("name", ["edge_lengths", "alternating_in_class"])
def test_class_runs_forced_chunks(shape_records, class_wants, name, monkeypatch):
    b = shape_records[name]
    lens = [int(L) for L in b.ref_lens]
    set_knobs(monkeypatch, depth_chunk_bases=2048)      # read by cov_create
    with open_session(b) as s:
        s.finish()
        for c in ("MIXED", "ONE"):
            chunks = []
            res = s.depth_class_runs(K.CUT_LISTS[c], chunks=chunks)
            assert_runs(res, class_wants[name][c], "chunked %s %s" % (name, c))
            assert [k["tid_next"] for k in chunks] == plan_ref(lens, 2048) and len(chunks) > 1


@pytest.fixture(scope="module")
def count_wants():
    """name -> set -> (regions, {threshold list -> counts}, reduce): computed once, shared, never changed."""
    out = {}
    for name, depths in R.shapes().items():
        sets = G.region_sets([len(d) for d in depths])
        out[name] = {k: (regs, {tn: K.counts(depths, regs, thr) for tn, thr in THR_LISTS.items()}, G.reduce(depths, regs)) for k, regs in sets.items() if regs}
    return out


THR_LISTS = {"MIXED": K.MIXED, "UNIT": K.UNIT, "ONE_BASE": (1,), "K16": K16}


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_threshold_counts_of_the_shapes(shape_records, count_wants, name):
    b = shape_records[name]
    assert sorted(len(t) for t in THR_LISTS.values()) == [1, 4, 16, 16]
    with open_session(b) as s:
        s.finish()
        for k, (regs, wants, red) in sorted(count_wants[name].items()):
            s.set_depth_thresholds([])
            s.set_depth_regions(regs)
            plain = s.depth_regions()
            assert s.depth_regions_kernel_ms()[1] == 6
            for tn, thr in sorted(THR_LISTS.items()):
                msg = "%s %s %s" % (name, k, tn)
                s.set_depth_thresholds(thr)
                bins, cnt = s.depth_region_counts()
                assert cnt.dtype == np.uint32 and cnt.shape == (len(regs), len(thr)), msg
                np.testing.assert_array_equal(cnt, wants[tn], err_msg=msg)
                assert bins.tobytes() == plain.tobytes() == red.tobytes(), msg      # the results are the bytes they are without thresholds
                assert s.depth_regions().tobytes() == plain.tobytes(), msg
                ms, launches = s.depth_regions_kernel_ms()
                assert ms > 0 and launches == 6
                # invariants
                ln = np.asarray([e - a for _, a, e in regs], np.int64)
                c64 = cnt.astype(np.int64)
                assert (np.diff(c64, axis=1) <= 0).all(), msg
                for j, t in enumerate(thr):
                    if t == 0:
                        np.testing.assert_array_equal(c64[:, j], ln, err_msg=msg)
                    if t == 1:
                        np.testing.assert_array_equal(cnt[:, j], bins["covered"], err_msg=msg)
                    assert (c64[bins["max"] < t, j] == 0).all(), msg
            s.set_depth_thresholds(None)      # cleared: the plain kernel again
            assert s.depth_regions().tobytes() == plain.tobytes() and s.depth_regions_kernel_ms()[1] == 6
    if name == "empty_targets_only":
        assert not count_wants[name]


def test_counts_of_a_region_given_several_times_are_identical(shape_records, count_wants):
    """The 13-piece region given six times: thirteen waves add into one row, two sessions, two calls each."""
    name = "runs_cross_boundaries"
    b = shape_records[name]
    regs, wants, _ = count_wants[name]["overlap"]
    assert regs.count((0, 0, 49229)) >= 6 and G.pieces_of(0, 49229) == 13
    got = []
    for _ in range(2):
        with open_session(b) as s:
            s.finish()
            s.set_depth_regions(regs)
            s.set_depth_thresholds(K16)
            for _ in range(2):
                got.append(s.depth_region_counts()[1].tobytes())
    assert got[0] == got[1] == got[2] == got[3] == wants["K16"].tobytes()


@pytest.mark.parametrize("name", ["runs_cross_boundaries", "edge_lengths", "starts_at_every_residue"])
def test_counts_of_windows_by_tiling(shape_records, name):
    b, depths = shape_records[name], R.shapes()[name]
    lens = [int(L) for L in b.ref_lens]
    with open_session(b) as s:
        s.finish()
        s.set_depth_thresholds(K.MIXED)
        for bs in (1, 5, 256, 1000, W + 1):
            regs = [(t, j * bs, min((j + 1) * bs, L)) for t, L in enumerate(lens) for j in range((L + bs - 1) // bs)]
            s.set_depth_regions(regs)
            _, cnt = s.depth_region_counts()
            np.testing.assert_array_equal(cnt, K.counts(depths, regs, K.MIXED), err_msg="B=%d" % bs)


def test_counts_forced_chunks(shape_records, count_wants, monkeypatch):
    name = "edge_lengths"
    b = shape_records[name]
    set_knobs(monkeypatch, depth_chunk_bases=2048)      # read by cov_create
    with open_session(b) as s:
        s.finish()
        s.set_depth_thresholds(K.UNIT)
        for k, (regs, wants, red) in sorted(count_wants[name].items()):
            s.set_depth_regions(regs)
            chunks = []
            bins, cnt = s.depth_region_counts(chunks=chunks)
            assert len(chunks) > 1 and bins.tobytes() == red.tobytes()
            np.testing.assert_array_equal(cnt, wants["UNIT"], err_msg=k)


def check_fixture(b, monkeypatch, ff=(True, True, False), fp=None):
    off_f = O.FlagFilter(*ff)
    ofp, filt = None, FilterConfig(*ff)
    if fp is not None:
        ofp = O.FilterParameters(off_f, **fp)
        filt = FilterConfig(*ff, filter_single=True, min_mapq=ofp.min_mapq, min_aligned_length=ofp.min_aligned_length_single,
                            min_percent_identity=ofp.min_percent_identity_single, min_aligned_percent=ofp.min_aligned_percent_single)
    depths = oracle_depths(b, off_f, ofp)
    lens = [int(L) for L in b.ref_lens]
    sets = G.region_sets(lens)
    regs = sets["edges"] + sets["random"]
    thr = (1, 2, 3, 5)
    want_runs = K.class_runs_of(depths, K.MIXED)
    want_cnt = K.counts(depths, regs, thr)
    for budget in (None, 2048):
        if budget:
            set_knobs(monkeypatch, depth_chunk_bases=budget)      # read by cov_create
        with open_session(b, filt) as s:
            s.finish()
            assert_runs(s.depth_class_runs(K.MIXED), want_runs, "fixture runs")
            s.set_depth_regions(regs)
            s.set_depth_thresholds(thr)
            bins, cnt = s.depth_region_counts()
            np.testing.assert_array_equal(cnt, want_cnt)
            assert bins.tobytes() == G.reduce(depths, regs).tobytes()


def test_fixture_default_flags(monkeypatch):
    check_fixture(bamio.read_bam(os.path.join(RAW, "7seqs.reads_for_seq1_and_seq2.bam")), monkeypatch)


def test_fixture_reader_filter(monkeypatch):
    check_fixture(bamio.read_bam(os.path.join(RAW, "2seqs.bad_read.1.bam")), monkeypatch, ff=(True, True, True), fp=dict(min_percent_identity_single=0.99))


def test_states_and_refusals():
    b = bamio.read_bam(os.path.join(RAW, "7seqs.reads_for_seq1_and_seq2.bam"))
    n = len(b.ref_lens)
    lens = [int(L) for L in b.ref_lens]
    t0 = next(t for t, L in enumerate(lens) if L >= 10)
    with Session(0, FilterConfig(), 0) as s:
        L = s._lib
        err = lambda: L.cov_last_error(s._h).decode()
        i32 = lambda v: np.asarray(v, np.int32)
        nxt, cnt = C.c_uint32(0), C.c_uint64(0)
        buf = np.zeros(64, np.uint32)
        s.set_depth_thresholds((1, 10, 30))      # valid any time after cov_create, kept over set_targets
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        with pytest.raises(CovError) as ei:      # before a finish
            s.depth_class_runs(K.MIXED)
        assert ei.value.status == ERR_STATE and "cov_depth_class_runs_compute: needs a cov_finish" in ei.value.message
        s.finish()
        # bad cut lists, with the first offending index
        for cuts, at in (((), 0), (tuple(range(17)), 16), ((1, 5, 4, 9), 2), ((1, 5, 5), 2), ((0, -3, 4), 1)):
            a = i32(cuts)
            assert L.cov_depth_class_runs_compute(s._h, a.ctypes.data if a.size else None, a.size, 0, n, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
            assert "cov_depth_class_runs_compute: value %d:" % at in err(), err()
            assert L.cov_depth_thresholds_set(s._h, a.ctypes.data if a.size else None, a.size) == (ERR_INVALID_ARG if a.size else 0)
            if a.size:
                assert "cov_depth_thresholds_set: value %d:" % at in err(), err()
        assert L.cov_depth_thresholds_set(s._h, None, 3) == ERR_INVALID_ARG
        good = i32(K.MIXED)
        assert L.cov_depth_class_runs_compute(s._h, good.ctypes.data, 4, 3, 3, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
        assert L.cov_depth_class_runs_compute(s._h, good.ctypes.data, 4, 0, n + 1, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
        # (the empty list above cleared the thresholds) a counts fetch without thresholds
        s.set_depth_regions([(t0, 0, 5), (t0, 1, 2), (t0, 2, 10)])
        plain = s.depth_regions()
        assert L.cov_depth_regions_counts_fetch(s._h, buf.ctypes.data) == ERR_STATE and "no thresholds set" in err()
        with pytest.raises(CovError) as ei:
            s.depth_region_counts()
        assert ei.value.status == ERR_STATE and "no thresholds set" in ei.value.message
        # setting thresholds drops the regions chunk that awaits its fetch: a counts fetch without a chunk
        idx, res = np.zeros(8, np.uint64), np.zeros(8, native.DEPTH_BIN_DTYPE)
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == 0
        s.set_depth_thresholds((1, 10, 30))
        assert L.cov_depth_regions_counts_fetch(s._h, buf.ctypes.data) == ERR_STATE and "no chunk computed" in err()
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == ERR_STATE and "no chunk computed" in err()
        bins, counts = s.depth_region_counts()
        assert bins.tobytes() == plain.tobytes() and counts.shape == (3, 3)
        assert L.cov_depth_regions_counts_fetch(s._h, buf.ctypes.data) == 0 and buf[:9].tobytes() == counts.tobytes()
        assert L.cov_depth_regions_counts_fetch(s._h, None) == ERR_INVALID_ARG
        # another party takes the arena: the regions' sentence, word for word
        s.depth_class_runs(K.MIXED)
        assert L.cov_depth_regions_counts_fetch(s._h, buf.ctypes.data) == ERR_STATE
        assert err() == "cov_depth_regions_fetch: the chunk's arena was taken by a cov_depth_runs_compute since (cov_depth_regions_compute again)"
        s.depth_region_counts()
        ro = np.zeros(n + 1, np.uint64)
        assert L.cov_depth_runs_fetch(s._h, ro.ctypes.data, None) == ERR_STATE      # the class runs' chunk is the runs' chunk
        assert err() == "cov_depth_runs_fetch: the chunk's arena was taken by a cov_depth_regions_compute since (cov_depth_runs_compute again)"
        # kept over a finish, a reset and set_targets
        s.finish()
        assert L.cov_depth_regions_counts_fetch(s._h, buf.ctypes.data) == ERR_STATE and "no chunk computed" in err()
        assert s.depth_region_counts()[1].tobytes() == counts.tobytes()
        s.reset()
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        s.finish()
        s.set_depth_regions([(t0, 0, 5), (t0, 1, 2), (t0, 2, 10)])
        assert s.depth_region_counts()[1].tobytes() == counts.tobytes()
        # a chunk without a region: four launches, nothing to fetch
        if t0 + 1 < n:
            assert L.cov_depth_regions_compute(s._h, t0 + 1, n, C.byref(nxt), C.byref(cnt)) == 0 and cnt.value == 0
            assert L.cov_depth_regions_counts_fetch(s._h, None) == 0 and s.depth_regions_kernel_ms()[1] == 4


def test_class_runs_of_a_spilled_store_are_refused(monkeypatch):
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
            s.depth_class_runs(K.MIXED)
        assert ei.value.status == ERR_STATE and "already left the bounded record store" in ei.value.message
