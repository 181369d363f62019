"""Depth regions on the device (cov_depth_regions_set / _compute / _fetch through Session.set_depth_regions / depth_regions): every field of
every region equals numpy's slice of the oracle depth, in input order — on the synthetic shapes of tests/depth_runs_ref.py built as real
records with the region sets of tests/depth_regions_ref.py (word residues at both ends, a wave load's boundary, the piece boundary, overlaps
and interleaved targets, random), and on the reference's fixture files under the default flags and under a reader filter; regions that tile
a target give the bytes of Session.depth_bins; whole targets give the table of the same session; forced chunks give the same bytes and only
chunks that hold a region are computed; the contig block on the device is untouched; runs, bins and regions refuse each other's fetch."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from coverm_amd import native
from coverm_amd.native import CovError, ERR_INVALID_ARG, ERR_STATE
from oracle import bamio
from oracle import oracle as O
from tests import depth_regions_ref as G
from tests import depth_runs_ref as R
from tests.knobs import set_knobs
from tests.test_depth_runs_core import plan_ref
from tests.test_gpu_depth_runs import RAW, SMALL, device_block, oracle_depths, records_for, to_batch

pytestmark = pytest.mark.gpu

W = G.W


def assert_regions(got, want, msg=""):
    assert got.dtype == native.DEPTH_BIN_DTYPE and len(got) == len(want)
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


@pytest.fixture(scope="module")
def shape_wants():
    """name -> set -> (regions, expected fields): computed once, shared, never changed."""
    out = {}
    for name, depths in R.shapes().items():
        sets = G.region_sets([len(d) for d in depths])
        out[name] = {k: (regs, G.reduce(depths, regs)) for k, regs in sets.items()}
    return out


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_synthetic_shapes(shape_records, shape_wants, name):
    b, depths = shape_records[name], R.shapes()[name]
    n = len(depths)
    with open_session(b) as s:
        st, _ = s.finish()
        before = device_block(s)
        for k, (regs, want) in sorted(shape_wants[name].items()):
            s.set_depth_regions(regs)
            if not regs:      # (no target long enough for this set, or empty targets only) setting nothing clears: the compute says so
                with pytest.raises(CovError) as ei:
                    s.depth_regions()
                assert ei.value.status == ERR_STATE and "no regions set" in ei.value.message
                continue
            chunks = []
            got = s.depth_regions(chunks=chunks)
            assert_regions(got, want, "%s %s" % (name, k))
            assert len(chunks) == 1 and chunks[0]["tid_lo"] == min(t for t, _, _ in regs) and chunks[0]["tid_next"] == n and chunks[0]["n_regions"] == len(regs)
            assert chunks[0]["n_pieces"] == sum(G.pieces_of(a, e) for _, a, e in regs)
            assert chunks[0]["arena_bases"] == 4 * sum(max(1, (len(d) + 3) // 4) for d in depths[chunks[0]["tid_lo"]:])
            ms, launches = s.depth_regions_kernel_ms()
            assert ms > 0 and launches == 6      # marks, the rank scan's three, init, reduce
        after = device_block(s)
        assert before.tobytes() == after.tobytes()      # the pileup ran against the scratch copy
        for f in ("n_pass", "win_sum_d", "win_sum_d2", "full_covered", "win_max_d"):
            np.testing.assert_array_equal(after[f], st[f], err_msg=f)


@pytest.mark.parametrize("name", ["runs_cross_boundaries", "edge_lengths", "starts_at_every_residue"])
def test_regions_that_tile_a_target_are_the_bins(shape_records, name):
    b = shape_records[name]
    lens = [int(L) for L in b.ref_lens]
    with open_session(b) as s:
        s.finish()
        for bs in (1, 5, 256, 1000, W + 1):
            _, bins = s.depth_bins(bs)
            regs = [(t, j * bs, min((j + 1) * bs, L)) for t, L in enumerate(lens) for j in range((L + bs - 1) // bs)]
            s.set_depth_regions(regs)
            assert s.depth_regions().tobytes() == bins.tobytes(), "B=%d" % bs


@pytest.mark.parametrize("name", ["runs_cross_boundaries", "all_zero", "equal_across_boundaries"])
def test_whole_targets_are_the_table(shape_records, name):
    b = shape_records[name]
    lens = [int(L) for L in b.ref_lens]
    live = [t for t, L in enumerate(lens) if L]
    with open_session(b) as s:
        st, _ = s.finish()
        s.set_depth_regions([(t, 0, lens[t]) for t in live])
        got = s.depth_regions()
        np.testing.assert_array_equal(got["sum"], st["win_sum_d"][live])
        np.testing.assert_array_equal(got["covered"].astype(np.uint64), st["full_covered"][live].astype(np.uint64))
        np.testing.assert_array_equal(got["max"].astype(np.int64), st["win_max_d"][live].astype(np.int64))
        assert (got["min"] <= got["max"]).all() and (got["min"] >= 0).all() and (got["reserved"] == 0).all()


def test_forced_chunks_and_chunk_skipping(shape_records, shape_wants, monkeypatch):
    name = "edge_lengths"
    b, depths = shape_records[name], R.shapes()[name]
    lens = [len(d) for d in depths]
    whole = {}
    with open_session(b) as s:
        s.finish()
        for k, (regs, _) in shape_wants[name].items():
            if regs:      # (no target of this shape is long enough for the piece set)
                s.set_depth_regions(regs)
                whole[k] = s.depth_regions().tobytes()
    set_knobs(monkeypatch, depth_chunk_bases=2048)      # read by cov_create
    plan = plan_ref(lens, 2048)
    assert len(plan) > 2 and sorted(whole) == ["edges", "overlap", "random", "steps"]
    with open_session(b) as s:
        s.finish()
        for k, (regs, want) in sorted(shape_wants[name].items()):
            if not regs:
                continue
            s.set_depth_regions(regs)
            chunks = []
            got = s.depth_regions(chunks=chunks)
            assert_regions(got, want, "chunked %s" % k)
            assert got.tobytes() == whole[k] and len(chunks) > 1 and sum(c["n_regions"] for c in chunks) == len(regs)
            assert all(c["n_regions"] > 0 for c in chunks)
        # regions on the first and the last non-empty target only: the chunks between them are never computed
        first, last = min(t for t, L in enumerate(lens) if L), max(t for t, L in enumerate(lens) if L)
        regs = [(last, 0, lens[last]), (first, 0, lens[first]), (last, lens[last] - 1, lens[last])]
        s.set_depth_regions(regs)
        chunks = []
        got = s.depth_regions(chunks=chunks)
        assert_regions(got, G.reduce(depths, regs), "skipping")
        assert [c["tid_lo"] for c in chunks] == [first, last] and [c["n_regions"] for c in chunks] == [1, 2]
        assert chunks[0]["tid_next"] == plan_ref(lens[first:], 2048)[0] + first and chunks[0]["tid_next"] <= last and len(chunks) < len(plan)


def test_two_sessions_two_calls_give_identical_bytes(shape_records, shape_wants):
    name = "runs_cross_boundaries"
    b = shape_records[name]
    regs, want = shape_wants[name]["overlap"]
    big = (0, 0, 49229)
    assert regs.count(big) >= 3 and G.pieces_of(0, 49229) == 13      # thirteen waves add into one value, three times over
    got = []
    for _ in range(2):
        with open_session(b) as s:
            s.finish()
            s.set_depth_regions(regs)
            for _ in range(2):
                got.append(s.depth_regions().tobytes())
    assert got[0] == got[1] == got[2] == got[3] == want.tobytes()


def check_fixture(b, monkeypatch, ff=(True, True, False), fp=None, chunked=2048):
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
    want = G.reduce(depths, regs)
    with open_session(b, filt) as s:
        s.finish()
        s.set_depth_regions(regs)
        got = s.depth_regions()
        assert_regions(got, want)
    set_knobs(monkeypatch, depth_chunk_bases=chunked)      # read by cov_create
    with open_session(b, filt) as s:
        s.finish()
        s.set_depth_regions(regs)
        assert s.depth_regions().tobytes() == got.tobytes()


@pytest.mark.parametrize("name", SMALL)
def test_fixture_default_flags(name, monkeypatch):
    check_fixture(bamio.read_bam(os.path.join(RAW, name)), monkeypatch)


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
        one = np.zeros(1, native.DEPTH_REGION_DTYPE)
        one[0] = (t0, 0, 5, 0)
        assert L.cov_depth_regions_set(s._h, one.ctypes.data, 1) == ERR_STATE and "cov_set_targets" in err()      # before set_targets
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        nxt, cnt = C.c_uint32(0), C.c_uint64(0)
        s.set_depth_regions([(t0, 0, 5)])
        with pytest.raises(CovError) as ei:      # before a finish
            s.depth_regions()
        assert ei.value.status == ERR_STATE and "needs a cov_finish" in ei.value.message
        s.finish()
        idx, res = np.zeros(8, np.uint64), np.zeros(8, native.DEPTH_BIN_DTYPE)
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == ERR_STATE and "no chunk computed" in err()
        # every refusal of set names the index of the first offending region, and leaves the regions set before
        good = [(t0, 0, 5), (t0, 1, 2), (t0, 2, 10)]
        for at, bad, what in ((2, (n, 0, 1, 0), "tid"), (1, (t0, 5, 5, 0), "start >= end"), (3, (t0, 6, 5, 0), "start >= end"), (0, (t0, 0, lens[t0] + 1, 0), "length"),
                              (2, (t0, 0, 1, 7), "reserved")):
            arr = np.zeros(4, native.DEPTH_REGION_DTYPE)
            rows = [g + (0,) for g in good]
            rows.insert(at, bad)
            for i, r in enumerate(rows):
                arr[i] = r
            assert L.cov_depth_regions_set(s._h, arr.ctypes.data, 4) == ERR_INVALID_ARG
            assert "region %d:" % at in err() and what in err()
        assert L.cov_depth_regions_set(s._h, one.ctypes.data, 2 ** 32) == ERR_INVALID_ARG and "2^32" in err()
        assert L.cov_depth_regions_set(s._h, None, 3) == ERR_INVALID_ARG
        assert len(s.depth_regions()) == 1      # still the one region set before the refusals
        assert L.cov_depth_regions_compute(s._h, 3, 3, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
        assert L.cov_depth_regions_compute(s._h, 0, n + 1, C.byref(nxt), C.byref(cnt)) == ERR_INVALID_ARG
        # a chunk without a region is legal
        if t0 + 1 < n:
            assert L.cov_depth_regions_compute(s._h, t0 + 1, n, C.byref(nxt), C.byref(cnt)) == 0 and cnt.value == 0 and nxt.value == n
            assert L.cov_depth_regions_fetch(s._h, None, None) == 0
            assert s.depth_regions_kernel_ms()[1] == 4
        # n = 0 clears the regions
        s.set_depth_regions([])
        assert L.cov_depth_regions_compute(s._h, 0, n, C.byref(nxt), C.byref(cnt)) == ERR_STATE and "no regions set" in err()
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == ERR_STATE
        # runs, bins and regions share the chunk's arena: each compute takes it from the other two
        s.set_depth_regions(good)
        off, ro = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        want = s.depth_regions()
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == 0 and res[:3].tobytes() == want.tobytes() and idx[:3].tolist() == [0, 1, 2]
        s.depth_runs()
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == ERR_STATE
        assert err() == "cov_depth_regions_fetch: the chunk's arena was taken by a cov_depth_runs_compute since (cov_depth_regions_compute again)"
        s.depth_regions()
        assert L.cov_depth_runs_fetch(s._h, ro.ctypes.data, None) == ERR_STATE
        assert err() == "cov_depth_runs_fetch: the chunk's arena was taken by a cov_depth_regions_compute since (cov_depth_runs_compute again)"
        s.depth_bins(100)
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == ERR_STATE
        assert err() == "cov_depth_regions_fetch: the chunk's arena was taken by a cov_depth_bins_compute since (cov_depth_regions_compute again)"
        assert L.cov_depth_runs_fetch(s._h, ro.ctypes.data, None) == ERR_STATE and "no chunk computed" not in err() and "cov_depth_regions_compute since" in err()
        s.depth_regions()
        assert L.cov_depth_bins_fetch(s._h, off.ctypes.data, None) == ERR_STATE
        assert err() == "cov_depth_bins_fetch: the chunk's arena was taken by a cov_depth_regions_compute since (cov_depth_bins_compute again)"
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == 0 and res[:3].tobytes() == want.tobytes()
        # a new finish drops the chunk and keeps the regions; so does a reset
        s.finish()
        assert L.cov_depth_regions_fetch(s._h, idx.ctypes.data, res.ctypes.data) == ERR_STATE and "no chunk computed" in err()
        assert s.depth_regions().tobytes() == want.tobytes()
        s.reset()
        s.push(to_batch(b))
        s.finish()
        assert s.depth_regions().tobytes() == want.tobytes()
        # set_targets drops the regions
        s.reset()
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        s.finish()
        assert L.cov_depth_regions_compute(s._h, 0, n, C.byref(nxt), C.byref(cnt)) == ERR_STATE and "no regions set" in err()


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
        s.set_depth_regions([(0, 0, 100)])
        with pytest.raises(CovError) as ei:
            s.depth_regions()
        assert ei.value.status == ERR_STATE and "already left the bounded record store" in ei.value.message
