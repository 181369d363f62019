"""The record store's shared seams (csrc/record_store.h, admit_window in csrc/covermhip.hip): columns that grow keep their content, a store
swapped in by cov_group_records grows again, and a window of ingested records is admitted — spill first, size, reserve — the same way
whether the BGZF ingest or the SAM text ingest asks.  The expected side is numpy over the pushed arrays, the oracle over the same sequence,
or an uncapped session fed by cov_push_batch; never the path under test."""
import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd import synth
from coverm_amd.engine import FilterConfig, RecordBatch, Session
from oracle import bamio
from oracle import oracle as O
from tests import namehash, samtext
from tests.grouping import assert_same_records, grouped_order, take_bamdata
from tests.knobs import set_knobs
from tests.test_gpu_abi_parity import to_bamdata, to_batch
from tests.test_host_golden import _paired_sample

pytestmark = pytest.mark.gpu


# ---- 1. growth keeps content
def test_three_pushes_that_each_pass_the_capacity():
    """1 000, 3 000 and 9 000 records: every push needs more than one and a half times what the columns hold, so every column is reallocated
    with its first R (cigar_off: R + 1) elements kept.  The second batch addresses its CIGAR words from a non-zero offset that is not the
    store's word count, the third from zero: both are rebased."""
    ref = synth.make_reference(40, 8_000_000, seed=201, min_len=1500, max_len=600_000)
    whole = synth.make_reads(ref, 13_000, seed=202)
    assert int(whole.cigar_off[0]) == 0 and int(whole.cigar_off[-1]) > 13_000      # (some reads carry more than one operation)
    co = whole.cigar_off.astype(np.int64)
    junk = 7
    second = whole.slice(1_000, 4_000)
    second = RecordBatch(second.tid, second.pos, second.flag, second.mapq, second.nm, second.nm_kind, second.l_seq,
                         (co[1_000:4_001] + junk).astype(np.uint32), np.concatenate([np.full(junk, 0xdead, np.uint32), whole.cigar]))
    third = whole.slice(4_000, 13_000)
    third = RecordBatch(third.tid, third.pos, third.flag, third.mapq, third.nm, third.nm_kind, third.l_seq,
                        (co[4_000:] - co[4_000]).astype(np.uint32), np.ascontiguousarray(whole.cigar[co[4_000]:]))
    assert int(second.cigar_off[0]) not in (0, int(co[1_000])) and int(third.cigar_off[0]) == 0
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref.lengths)
        for b in (whole.slice(0, 1_000), second, third):
            s.push(b)
        got = cbam.session_records(s)
    assert int(got.cigar_off[-1]) == len(got.cigar) == int(co[-1])      # the closing offset is the word count
    assert_same_records(got, RecordBatch.from_arrays(whole.tid, whole.pos, whole.flag, whole.mapq, whole.nm, whole.nm_kind, whole.l_seq, whole.cigar_off,
                                                     whole.cigar[:co[-1]]))


# ---- 2. a gathered store grows again
def assert_equals_oracle(st, summ, hist, g: bamio.BamData, excl):
    exp, exp_hist, prim = O.integer_stats(g, O.FlagFilter(True, True, False), None, excl, None)
    assert summ.num_detected_primary_alignments == prim and int(summ.n_records) == g.n_records
    live = exp["seen"] == 1
    assert live.sum() >= 4
    for f in ("n_primary", "n_pass", "n_nonsupp"):
        np.testing.assert_array_equal(st[f], exp[f], err_msg=f)
    for f in ("sum_nm", "sum_indel", "win_sum_d", "win_sum_d2", "win_covered", "full_covered", "win_min_d", "win_max_d", "first_record", "last_record", "hist_len"):
        np.testing.assert_array_equal(st[f][live], exp[f][live], err_msg=f)
    np.testing.assert_array_equal(st["sum_identity_primary"][live].view(np.uint64), exp["id_primary"][live].view(np.uint64))
    np.testing.assert_array_equal(st["sum_identity_nonsupp"][live].view(np.uint64), exp["id_nonsupp"][live].view(np.uint64))
    ho, eo, hl = st["hist_off"].astype(np.int64), exp["hist_off"].astype(np.int64), exp["hist_len"].astype(np.int64)
    for t in np.nonzero(live)[0]:
        np.testing.assert_array_equal(hist[ho[t]:ho[t] + hl[t]], exp_hist[eo[t]:eo[t] + hl[t]], err_msg="hist of contig %d" % t)


@pytest.fixture(scope="module")
def out_of_order():
    """~2 000 records over 5 references in a random order, 500 more of the last reference to follow, and the sequence the store must hold
    in the end: the first lot in numpy's stable grouped order, then the rest."""
    base = _paired_sample(1_600, seed=211)
    rng = np.random.default_rng(212)
    last = np.nonzero(np.asarray(base.tid) == 4)[0][-500:]
    rest = np.setdiff1d(np.arange(base.n_records), last)
    assert len(last) == 500 and len(rest) > 2_000
    sh = rng.permutation(rest)[:2_000]
    shuffled, more = take_bamdata(base, sh), take_bamdata(base, last)
    grouped = sh[grouped_order(shuffled.tid, 5)]
    assert (grouped != sh).sum() > 1_000
    return shuffled, more, take_bamdata(base, np.concatenate([grouped, last]))


def test_push_group_push(out_of_order):
    shuffled, more, want = out_of_order
    batch = to_batch(shuffled)
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        s.set_targets(np.asarray(shuffled.ref_lens, np.int64))
        s.push(batch.slice(0, 700))
        s.push(batch.slice(700, batch.n_records))
        assert s.group_records() > 1_000      # the store is now the gathered one: columns of exactly the selected size
        s.push(to_batch(more))
        assert_same_records(cbam.session_records(s), to_batch(want))
        st, summ = s.finish()
        assert_equals_oracle(st, summ, s.hist(), want, 75)


def test_ingest_with_mates_group_push(tmp_path, out_of_order):
    """The same through a device ingest that keeps the mate columns: they travel through the swap with the other nine."""
    shuffled, more, want = out_of_order
    p = str(tmp_path / "shuffled.bam")
    bamio.write_bam(p, shuffled, level=1)
    n = shuffled.n_records
    order = grouped_order(shuffled.tid, 5)
    k1, k2 = namehash.name_hashes([shuffled.qname[i] for i in order])
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        assert cbam.gpu_ingest(s, p, threads=2, want_mates=True, group=True)[2] == n
        mtid, qh1, qh2 = cbam.session_mates(s, n)
        np.testing.assert_array_equal(mtid, np.asarray(shuffled.mtid)[order])
        np.testing.assert_array_equal(qh1, k1)
        np.testing.assert_array_equal(qh2, k2)
        s.push(to_batch(more))
        assert_same_records(cbam.session_records(s), to_batch(want))
        st, summ = s.finish()
        assert_equals_oracle(st, summ, s.hist(), want, 75)


# ---- 3. window admission, both callers
def test_bgzf_and_sam_windows_spill_alike(tmp_path, monkeypatch):
    """60 000 reads over 50 references under a cap of 20 000 records: as a BAM in windows of 64 BGZF blocks and as SAM text in windows of
    2 MB.  Both ingests spill at least twice, and their per-contig statistics equal each other's and those of the same records pushed
    into a session without a cap."""
    ref = synth.make_reference(50, 10_000_000, seed=221, min_len=1500, max_len=600_000)
    batch = synth.make_reads(ref, 60_000, seed=222)
    lens = np.asarray(ref.lengths, np.int64)
    bam_path, sam_path = str(tmp_path / "s.bam"), str(tmp_path / "s.sam")
    cbam.write_bam(bam_path, ref.names, ref.lengths, batch, with_seq=1, threads=8)
    with open(sam_path, "wb") as f:
        f.write(samtext.render(to_bamdata(batch, ref.lengths, ref.names), seed=223))
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(lens)
        s.push(batch)
        want_st, want_summ = s.finish()
    assert (want_st["n_pass"] > 0).sum() >= 40
    set_knobs(monkeypatch, store_cap_records=20000, ingest_round_blocks=64, sam_window_bytes=2_000_000)
    got = {}
    for route, path in (("bgzf", bam_path), ("sam", sam_path)):
        with Session(0, FilterConfig(), 75) as s:
            assert cbam.gpu_ingest(s, path, threads=2)[2] == batch.n_records
            st, summ = s.finish()
            got[route] = (st, summ, s.store_spills())
            print("%s: %d spills" % (route, got[route][2]))
    for route, (st, summ, n_spills) in got.items():
        assert n_spills >= 2, route
        assert int(summ.n_records) == batch.n_records and summ.num_detected_primary_alignments == want_summ.num_detected_primary_alignments, route
        for k in st.dtype.names:
            np.testing.assert_array_equal(st[k], want_st[k], err_msg="%s %s" % (route, k))
    assert got["bgzf"][0].tobytes() == got["sam"][0].tobytes()
