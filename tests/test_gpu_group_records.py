"""cov_group_records (csrc/group_kernels.hip.h): a record store that is not sorted by reference, grouped on the device.  The expected side is
always numpy's stable order of the same records (tests/grouping.py) and the oracle over that sequence — never the code under test.
Inputs: the reference's fixture BAMs and coverm_amd.synth samples, shuffled three ways (random permutation, name order, blocks of 1 000
records swapped)."""
import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd import host, synth
from coverm_amd.engine import FilterConfig, Session
from coverm_amd.host import CoverageEstimator as E
from coverm_amd.native import CovError, ERR_STATE, ERR_UNSORTED
from oracle import bamio
from oracle import oracle as O
from tests.fixtures import load_fixture
from tests.golden import cases
from tests.grouping import assert_same_records, grouped_order, shuffles, take_bamdata, take_batch
from tests.knobs import set_knobs
from tests.test_gpu_abi_parity import to_bamdata, to_batch
from tests.test_host_golden import _paired_sample

pytestmark = pytest.mark.gpu

FIXTURES = [f for f in cases.FIXTURE_FILES if "unsorted" not in f]      # (the error fixtures: their verdict is the subject of other tests)


def store_after_grouping(batch, ref_lens):
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref_lens)
        s.push(batch)
        moved = s.group_records()
        return cbam.session_records(s), moved, s.group_kernel_ms()


def check_store(batch, ref_lens):
    order = grouped_order(batch.tid, len(ref_lens))
    got, moved, (ms, launches) = store_after_grouping(batch, ref_lens)
    assert_same_records(got, take_batch(batch, order))
    assert moved == int((order != np.arange(batch.n_records)).sum())
    assert launches >= (1 if batch.n_records >= 2 else 0) and ms >= 0      # (fewer than two records: nothing to check, nothing launched)
    return moved


def est_set(excl):
    return [E.new_estimator_mean(0.0, excl, False), E.new_estimator_trimmed_mean(0.05, 0.95, 0.0, excl), E.new_estimator_covered_fraction(0.0),
            E.new_estimator_variance(0.0, excl), E.new_estimator_read_count(), E.new_estimator_reads_per_base(), E.new_estimator_rpkm(0.0), E.new_estimator_anir()]


def check_finish(shuffled: bamio.BamData, excl, ff=(True, True, False), chunks=1):
    """push (in file order, unsorted) -> group_records -> finish: every integer, the histogram and the identity sums equal the oracle's over the
    grouped sequence; k_estimate's floats equal the host evaluation of those statistics."""
    g = take_bamdata(shuffled, grouped_order(shuffled.tid, len(shuffled.ref_lens)))
    off = O.FlagFilter(*ff)
    exp, exp_hist, prim = O.integer_stats(g, off, None, excl, None)
    batch = to_batch(shuffled)
    est = est_set(excl)
    names, lens = list(shuffled.ref_names), np.asarray(shuffled.ref_lens, np.int64)
    with Session(0, FilterConfig(*ff), excl, want_hist=True, want_identity=True) as s:
        s.set_targets(lens)
        s.set_estimators(est)
        edges = np.linspace(0, batch.n_records, chunks + 1).astype(int)
        for lo, hi in zip(edges[:-1], edges[1:]):
            s.push(batch.slice(lo, hi))
        s.group_records()
        st, summ = s.finish()
        hist = s.hist()
        ef = s.estimates()
    assert summ.num_detected_primary_alignments == prim
    live = exp["seen"] == 1
    for f in ("n_primary", "n_pass", "n_nonsupp"):
        np.testing.assert_array_equal(st[f], exp[f], err_msg=f)
    for f in ("sum_nm", "sum_indel", "win_sum_d", "win_sum_d2", "win_covered", "full_covered", "win_min_d", "win_max_d", "first_record", "last_record", "hist_len"):
        np.testing.assert_array_equal(st[f][live], exp[f][live], err_msg=f)
    np.testing.assert_array_equal(st["sum_identity_primary"][live].view(np.uint64), exp["id_primary"][live].view(np.uint64))
    np.testing.assert_array_equal(st["sum_identity_nonsupp"][live].view(np.uint64), exp["id_nonsupp"][live].view(np.uint64))
    ho, eo, hl = st["hist_off"].astype(np.int64), exp["hist_off"].astype(np.int64), exp["hist_len"].astype(np.int64)
    for t in np.nonzero(live)[0]:
        np.testing.assert_array_equal(hist[ho[t]:ho[t] + hl[t]], exp_hist[eo[t]:eo[t] + hl[t]], err_msg="hist of contig %d" % t)
    takers = []
    for dev in (True, False):
        taker = host.CoverageTaker.new_cached_single_float_coverage_taker(len(est))
        sample = host.SampleResult("s", st, None if dev else hist, int(summ.num_detected_primary_alignments))
        host.contig_coverage(names, lens, [sample], taker, est, True, **(dict(estimates=[ef]) if dev else {}))
        takers.append(taker.cached_coverages(0))
    np.testing.assert_array_equal(takers[0].view(np.uint32), takers[1].view(np.uint32))


# ---- 1. the store after group_records() is numpy's stable order, byte for byte
@pytest.mark.parametrize("name", FIXTURES)
def test_store_fixtures(name):
    b = load_fixture(name)
    n = len(b.tid)
    for kind, perm in shuffles(n, 5, b.qname).items():
        check_store(to_batch(take_bamdata(b, perm)), b.ref_lens)


@pytest.mark.parametrize("n_contigs,n_reads", [(5_000, 400_000), (200_000, 400_000), (3, 70_000), (300, 4097)])
def test_store_synthetic(n_contigs, n_reads):
    ref = synth.make_reference(n_contigs, max(30_000_000, n_contigs * 2000), seed=21, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, n_reads, seed=22)
    assert check_store(batch, ref.lengths) == 0                                  # grouped input: nothing moves, the store is left alone
    for kind, perm in shuffles(n_reads, 23).items():
        assert check_store(take_batch(batch, perm), ref.lengths) > 0, kind


def test_store_records_without_a_reference_come_last():
    ref = synth.make_reference(700, 30_000_000, seed=31, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 120_000, seed=32)
    batch.tid = batch.tid.copy()
    batch.tid[::17] = -1
    sh = take_batch(batch, shuffles(batch.n_records, 33)["random"])
    check_store(sh, ref.lengths)
    got, _, _ = store_after_grouping(sh, ref.lengths)
    n_unmapped = int((sh.tid < 0).sum())
    assert (got.tid[-n_unmapped:] == -1).all() and (np.diff(got.tid[:-n_unmapped]) >= 0).all()


def test_store_long_reads():
    """CIGARs of thousands of words: the gather moves more than 2^16 words per region of records."""
    ref = synth.make_reference(40, 40_000_000, seed=41, min_len=200_000, max_len=3_000_000)
    batch = synth.make_long_reads(ref, 6_000, seed=42)
    assert int(batch.cigar_off[-1]) > 6_000 * 100
    for kind, perm in shuffles(batch.n_records, 43).items():
        check_store(take_batch(batch, perm), ref.lengths)


# ---- 2. finish after grouping == the oracle over the grouped sequence
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("excl", [0, 75])
def test_finish_fixtures(name, excl):
    b = load_fixture(name)
    for kind, perm in shuffles(len(b.tid), 7, b.qname).items():
        check_finish(take_bamdata(b, perm), excl)


@pytest.mark.parametrize("n_contigs", [5_000, 200_000])
def test_finish_synthetic(n_contigs):
    ref = synth.make_reference(n_contigs, max(100_000_000, n_contigs * 2000), seed=51, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 400_000, seed=52)
    for kind, perm in shuffles(batch.n_records, 53).items():
        check_finish(to_bamdata(take_batch(batch, perm), ref.lengths, ref.names), 75, chunks=3)


def test_finish_long_reads_and_unmapped():
    ref = synth.make_reference(30, 30_000_000, seed=61, min_len=200_000, max_len=3_000_000)
    batch = synth.make_long_reads(ref, 3_000, seed=62)
    check_finish(to_bamdata(take_batch(batch, shuffles(batch.n_records, 63)["random"]), ref.lengths, ref.names), 0)
    ref = synth.make_reference(300, 30_000_000, seed=64, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 100_000, seed=65)
    batch.tid = batch.tid.copy()
    sel = np.arange(0, batch.n_records, 13)
    batch.tid[sel] = -1
    batch.flag = batch.flag.copy()
    batch.flag[sel] |= 0x4                                   # records without a reference are unmapped
    for kind, perm in shuffles(batch.n_records, 66).items():
        check_finish(to_bamdata(take_batch(batch, perm), ref.lengths, ref.names), 75)


# ---- 3. without group_records() nothing changes: the same batches still end in the reference's error
def test_without_grouping_the_file_is_still_unsorted():
    ref = synth.make_reference(300, 30_000_000, seed=71, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 50_000, seed=72)
    for kind, perm in shuffles(batch.n_records, 73).items():
        with Session(0, FilterConfig(), 75) as s:
            s.set_targets(ref.lengths)
            s.push(take_batch(batch, perm))
            with pytest.raises(CovError) as ei:
                s.finish()
            assert ei.value.status == ERR_UNSORTED and "BAM file appears to be unsorted" in ei.value.message, kind


# ---- 4. device ingest of a shuffled BAM with group=True; the pair filter behind it
FIELDS = ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq")


def _written(tmp_path, d, name="s.bam"):
    p = str(tmp_path / name)
    bamio.write_bam(p, d, level=1)
    return p


@pytest.mark.parametrize("want_mates", [False, True])
def test_device_ingest_then_group(tmp_path, want_mates):
    b = _paired_sample(20_000, seed=81)
    for kind, perm in shuffles(len(b.tid), 82, b.qname).items():
        sh = take_bamdata(b, perm)
        p = _written(tmp_path, sh, kind + ".bam")
        with Session(0, FilterConfig(), 75) as s:
            if want_mates:
                with pytest.raises(cbam.IngestFallback):             # as before: mates without the announcement hand the file back
                    cbam.gpu_ingest(s, p, threads=2, want_mates=True)
                s.reset()
            _, _, n, _ = cbam.gpu_ingest(s, p, threads=2, want_mates=want_mates, group=True)
            assert n == len(b.tid)
            assert_same_records(cbam.session_records(s), to_batch(take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens)))))


PAIR_CASES = [c for c in cases.FILTER_CASES if c.get("mode") in ((False, True), (True, True), None)]


def _pair_selection(path, ofp):
    fs, fpairs = O.filter_mode(ofp)
    with Session(0, FilterConfig(), 75) as s:
        cbam.gpu_ingest(s, path, threads=2, want_mates=True, group=True)
        nsel, nprim = cbam.pair_filter_apply(s, fs, ofp.min_mapq, (ofp.min_aligned_length_single, ofp.min_percent_identity_single, ofp.min_aligned_percent_single),
                                             (ofp.min_aligned_length_pair, ofp.min_percent_identity_pair, ofp.min_aligned_percent_pair))
        got = cbam.session_records(s)
    assert got.n_records == nsel
    return got, nprim


def _check_pair(tmp_path, sh, ofp, tag):
    g = take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens)))
    order, prim = O.reader_stage(g, ofp)                      # the oracle's reader filter over the grouped sequence: records and order
    got, nprim = _pair_selection(_written(tmp_path, sh, tag + ".bam"), ofp)
    assert_same_records(got, to_batch(take_bamdata(g, np.asarray(order, np.int64))))
    assert nprim == prim
    return len(order)


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: c["id"])
def test_pair_filter_after_grouping_goldens(tmp_path, case):
    d = load_fixture(case["bam"])
    ofp = O.FilterParameters(O.FlagFilter(*case["ff"]), case["single"][0], case["single"][1], case["single"][2], case["mapq"], case["pair"][0], case["pair"][1], case["pair"][2])
    if not O.filter_mode(ofp)[1]:
        return                                                  # the single-read branch has no reader-stage pair filter to follow
    for kind, perm in shuffles(len(d.tid), 91, d.qname).items():
        _check_pair(tmp_path, take_bamdata(d, perm), ofp, kind)


@pytest.mark.parametrize("params", [dict(min_percent_identity_pair=0.95), dict(min_aligned_length_pair=200, min_mapq=20), dict(min_percent_identity_single=0.9, min_aligned_percent_pair=0.8)])
def test_pair_filter_after_grouping_synthetic(tmp_path, params):
    b = _paired_sample(30_000, seed=93)
    ofp = O.FilterParameters(O.FlagFilter(True, True, False), **params)
    for kind, perm in shuffles(len(b.tid), 94, b.qname).items():
        assert _check_pair(tmp_path, take_bamdata(b, perm), ofp, kind) > 1000


# ---- 5. COV_ERR_STATE
def _state_error(s):
    with pytest.raises(CovError) as ei:
        s.group_records()
    assert ei.value.status == ERR_STATE
    return ei.value.message


def test_refuses_an_adopted_store():
    import torch
    ref = synth.make_reference(50, 5_000_000, seed=101, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 5_000, seed=102)
    dev = {k: torch.from_numpy(getattr(batch, k)).to("cuda:0") for k in ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq", "cigar_off", "cigar")}
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref.lengths)
        s.push_device(dev, batch.n_records)
        assert "adopted" in _state_error(s)


def test_refuses_a_span_session(tmp_path):
    ref = synth.make_reference(200, 20_000_000, seed=103, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 60_000, seed=104)
    p = str(tmp_path / "sorted.bam")
    cbam.write_bam(p, ref.names, ref.lengths, batch)
    with Session(0, FilterConfig(), 75) as s:
        cbam.gpu_ingest(s, p, threads=2, span=(0, 2))
        assert "span" in _state_error(s)
        s.reset()
        cbam.gpu_ingest(s, p, threads=2)
        assert s.group_records() == 0


def test_refuses_after_a_spill(monkeypatch):
    set_knobs(monkeypatch, store_cap_records=50000, store_cap_cigar=200000)
    ref = synth.make_reference(300, 30_000_000, seed=105, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 200_000, seed=106)
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref.lengths)
        for lo in range(0, batch.n_records, 9973):
            s.push(batch.slice(lo, min(batch.n_records, lo + 9973)))
        assert s.store_spills() >= 1
        assert "must fit the record store" in _state_error(s)


# ---- 6. the permutation is the same in every run
def test_two_sessions_give_identical_stores():
    ref = synth.make_reference(5_000, 100_000_000, seed=111, min_len=1500, max_len=600_000)
    batch = take_batch(synth.make_reads(ref, 400_000, seed=112), shuffles(400_000, 113)["random"])
    a, _, _ = store_after_grouping(batch, ref.lengths)
    b, _, _ = store_after_grouping(batch, ref.lengths)
    assert_same_records(a, b)
