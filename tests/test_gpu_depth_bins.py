"""Depth bins on the device (cov_depth_bins_compute / cov_depth_bins_fetch through Session.depth_bins): bin_off and every field of every bin
equal numpy's reduceat over the oracle depth — on the synthetic shapes of tests/depth_runs_ref.py built as real records, at the bin sizes
where a lane's word, a wave's load, a wave's stretch and a target boundary meet, and on the reference's fixture files under the default
flags and under a reader filter; forced chunks give the same bins; the contig block on the device is untouched; the bins integrate to the
table of the same session; the runs and the bins refuse each other's fetch."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from coverm_amd import native
from coverm_amd.native import CovError, ERR_INVALID_ARG, ERR_STATE
from oracle import bamio
from oracle import oracle as O
from tests import depth_bins_ref as B
from tests import depth_runs_ref as R
from tests.knobs import set_knobs
from tests.test_depth_runs_core import plan_ref
from tests.test_gpu_depth_runs import RAW, SMALL, device_block, oracle_depths, records_for, to_batch

pytestmark = pytest.mark.gpu

W = B.stretch_bases()
BIN_SIZES = [1, 3, 4, 5, 64, 255, 256, 257, 1000, W - 1, W + 1, 16384, 50000]      # (the largest shape is 49 229 bases)


def assert_bins(got_off, got, want_off, want, msg=""):
    assert got.dtype == native.DEPTH_BIN_DTYPE and got_off.dtype == np.uint64
    np.testing.assert_array_equal(got_off, want_off, err_msg=msg)
    for f in ("sum", "min", "max", "covered", "reserved"):
        np.testing.assert_array_equal(got[f], want[f], err_msg="%s %s" % (msg, f))


def open_session(b, filt=None):
    s = Session(0, filt or FilterConfig(), 0)
    s.set_targets(b.ref_lens)
    s.push(to_batch(b))
    return s


@pytest.fixture(scope="module")
def shape_records():
    return {name: records_for(depths) for name, depths in R.shapes().items()}


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_synthetic_shapes(shape_records, name):
    b, depths = shape_records[name], R.shapes()[name]
    n = len(depths)
    with open_session(b) as s:
        st, _ = s.finish()
        before = device_block(s)
        for bs in BIN_SIZES:
            want_off, want = B.bins_of(depths, bs)
            chunks = []
            off, bins = s.depth_bins(bs, chunks=chunks)
            assert_bins(off, bins, want_off, want, "%s B=%d" % (name, bs))
            assert len(chunks) == 1 and chunks[0]["tid_lo"] == 0 and chunks[0]["tid_next"] == n and chunks[0]["n_bins"] == len(want) and chunks[0]["bin_size"] == bs
            assert chunks[0]["arena_bases"] == 4 * sum(max(1, (len(d) + 3) // 4) for d in depths)
            ms, launches = s.depth_bins_kernel_ms()
            assert ms > 0 and launches == (6 if len(want) else 4)      # marks, the rank scan's three, init, reduce
            if n >= 3:      # a sub-range answers for its targets alone
                o2, b2 = s.depth_bins(bs, 1, n - 1)
                lo, hi = int(want_off[1]), int(want_off[n - 1])
                assert_bins(o2, b2, want_off[1:n] - want_off[1], want[lo:hi], "%s B=%d sub-range" % (name, bs))
        after = device_block(s)
        assert before.tobytes() == after.tobytes()      # the pileup ran against the scratch copy
        for f in ("n_pass", "win_sum_d", "win_sum_d2", "full_covered", "win_max_d"):
            np.testing.assert_array_equal(after[f], st[f], err_msg=f)


def invariants(s, st, lens, bs):
    """The bins of a session against the table of the same session (contig_end_exclusion 0: the window is the whole target)."""
    off, bins = s.depth_bins(bs)
    o = off.astype(np.int64)
    owner = np.repeat(np.arange(len(lens)), np.diff(o))
    np.testing.assert_array_equal(np.bincount(owner, weights=bins["sum"].astype(np.float64), minlength=len(lens)).astype(np.uint64), st["win_sum_d"])
    np.testing.assert_array_equal(np.bincount(owner, weights=bins["covered"], minlength=len(lens)).astype(np.uint64), st["full_covered"])
    mx = np.zeros(len(lens), np.int64)
    np.maximum.at(mx, owner, bins["max"].astype(np.int64))
    np.testing.assert_array_equal(mx, st["win_max_d"].astype(np.int64))
    assert (bins["min"] <= bins["max"]).all() and (bins["min"] >= 0).all() and (bins["reserved"] == 0).all()
    return off, bins


@pytest.mark.parametrize("name", ["runs_cross_boundaries", "starts_at_every_residue", "all_zero"])
def test_invariants_and_bin_size_one(shape_records, name):
    b = shape_records[name]
    lens = [int(L) for L in b.ref_lens]
    with open_session(b) as s:
        st, _ = s.finish()
        for bs in (3, 1000, W + 1):
            invariants(s, st, lens, bs)
        off, bins = invariants(s, st, lens, 1)
        np.testing.assert_array_equal(bins["sum"], bins["min"].astype(np.uint64))
        np.testing.assert_array_equal(bins["min"], bins["max"])
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
        # ... and these equal the expansion of depth_runs()
        run_off, start, depth = s.depth_runs()
        ro = run_off.astype(np.int64)
        owner = np.repeat(np.arange(len(lens)), np.diff(ro))
        nxt = np.append(start[1:], 0).astype(np.int64)
        last = np.zeros(len(start), bool)
        last[ro[1:][ro[1:] > ro[:-1]] - 1] = True
        end = np.where(last, np.asarray(lens, np.int64)[owner], nxt)
        np.testing.assert_array_equal(np.repeat(depth, end - start.astype(np.int64)), bins["max"])


def check_fixture(b, monkeypatch, ff=(True, True, False), fp=None, sizes=(100, 1000), chunked=2048):
    off_f = O.FlagFilter(*ff)
    ofp, filt = None, FilterConfig(*ff)
    if fp is not None:
        ofp = O.FilterParameters(off_f, **fp)
        filt = FilterConfig(*ff, filter_single=True, min_mapq=ofp.min_mapq, min_aligned_length=ofp.min_aligned_length_single,
                            min_percent_identity=ofp.min_percent_identity_single, min_aligned_percent=ofp.min_aligned_percent_single)
    depths = oracle_depths(b, off_f, ofp)
    lens = [int(L) for L in b.ref_lens]
    whole = {}
    with open_session(b, filt) as s:
        st, _ = s.finish()
        for bs in sizes:
            want_off, want = B.bins_of(depths, bs)
            off, bins = invariants(s, st, lens, bs)
            assert_bins(off, bins, want_off, want, "B=%d" % bs)
            whole[bs] = (off, bins)
    if chunked:      # forced chunks: the planner's boundaries, the same bytes
        set_knobs(monkeypatch, depth_chunk_bases=chunked)      # read by cov_create
        with open_session(b, filt) as s:
            s.finish()
            for bs in sizes:
                chunks = []
                off, bins = s.depth_bins(bs, chunks=chunks)
                assert [c["tid_next"] for c in chunks] == plan_ref(lens, chunked)
                assert chunks[0]["tid_lo"] == 0 and sum(c["n_bins"] for c in chunks) == len(bins)
                assert off.tobytes() == whole[bs][0].tobytes() and bins.tobytes() == whole[bs][1].tobytes()


@pytest.mark.parametrize("name", SMALL)
def test_fixture_default_flags(name, monkeypatch):
    check_fixture(bamio.read_bam(os.path.join(RAW, name)), monkeypatch)


def test_fixture_reader_filter(monkeypatch):
    check_fixture(bamio.read_bam(os.path.join(RAW, "2seqs.bad_read.1.bam")), monkeypatch, ff=(True, True, True), fp=dict(min_percent_identity_single=0.99))


def test_fixture_of_54579_references(monkeypatch):
    check_fixture(bamio.read_bam(os.path.join(RAW, "eg2.bam")), monkeypatch, sizes=(1000,), chunked=None)


def test_forced_chunks_on_a_shape(shape_records, monkeypatch):
    b, depths = shape_records["edge_lengths"], R.shapes()["edge_lengths"]
    lens = [len(d) for d in depths]
    set_knobs(monkeypatch, depth_chunk_bases=2048)
    with open_session(b) as s:
        s.finish()
        for bs in (1, 5, 256, 1000):
            chunks = []
            off, bins = s.depth_bins(bs, chunks=chunks)
            assert [c["tid_next"] for c in chunks] == plan_ref(lens, 2048) and len(chunks) > 1
            assert_bins(off, bins, *B.bins_of(depths, bs), "chunked B=%d" % bs)


def test_two_runs_give_identical_bytes(shape_records):
    b = shape_records["runs_cross_boundaries"]
    got = []
    for _ in range(2):
        with open_session(b) as s:
            s.finish()
            for bs in (5, 1000, 50000):      # 50 000: every wave of a target adds into one bin
                off, bins = s.depth_bins(bs)
                got.append((bs, off.tobytes(), bins.tobytes()))
                off, bins = s.depth_bins(bs)
                assert got[-1] == (bs, off.tobytes(), bins.tobytes())
    assert got[:3] == got[3:]


def test_states_and_refusals():
    b = bamio.read_bam(os.path.join(RAW, "7seqs.reads_for_seq1_and_seq2.bam"))
    n = len(b.ref_lens)
    with open_session(b) as s:
        L = s._lib
        err = lambda: L.cov_last_error(s._h).decode()
        with pytest.raises(CovError) as ei:      # before a finish
            s.depth_bins(100)
        assert ei.value.status == ERR_STATE and "needs a cov_finish" in ei.value.message
        s.finish()
        off = np.zeros(n + 1, np.uint64)
        assert L.cov_depth_bins_fetch(s._h, off.ctypes.data, None) == ERR_STATE      # no chunk computed yet
        assert "no chunk computed" in err()
        nxt, cnt = C.c_uint32(0), C.c_uint64(0)
        for bad in (0, 2 ** 31, 2 ** 32 - 1):
            assert L.cov_depth_bins_compute(s._h, bad, 0, n, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
            assert "bin size" in err()
        assert L.cov_depth_bins_compute(s._h, 2 ** 31 - 1, 0, n, C.byref(nxt), C.byref(cnt)) == 0 and cnt.value == sum(1 for x in b.ref_lens if x)
        assert L.cov_depth_bins_compute(s._h, 100, 3, 3, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
        assert L.cov_depth_bins_compute(s._h, 100, 0, n + 1, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
        # the runs and the bins share the chunk's arena
        ro = np.zeros(n + 1, np.uint64)
        s.depth_runs()
        assert L.cov_depth_bins_fetch(s._h, off.ctypes.data, None) == ERR_STATE and "cov_depth_runs_compute" in err()
        assert L.cov_depth_bins_compute(s._h, 100, 0, n, C.byref(nxt), C.byref(cnt)) == 0
        assert L.cov_depth_runs_fetch(s._h, ro.ctypes.data, None) == ERR_STATE and "cov_depth_bins_compute" in err()
        bins = np.zeros(cnt.value, native.DEPTH_BIN_DTYPE)
        assert L.cov_depth_bins_fetch(s._h, off.ctypes.data, bins.ctypes.data) == 0 and off[-1] == cnt.value
        s.finish()                                # a new finish drops the chunk
        assert L.cov_depth_bins_fetch(s._h, off.ctypes.data, None) == ERR_STATE and "no chunk computed" in err()


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
            s.depth_bins(1000)
        assert ei.value.status == ERR_STATE and "already left the bounded record store" in ei.value.message
