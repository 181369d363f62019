"""The long-CIGAR path at its decision points: what a record's CIGAR comes to (cigar_sum3, the state machine of prep_step_generic and its copy
in k_prep7s, cigar_walk_wave, cigar_walk_slow, run_word) and how its runs reach the pileup (k_cx_expand, the bucket scan, k_ranges, apply /
add_run of k_pileup_fast, k_pileup_fast2t and k_pileup_stream, the repeated pass of cov_finish).

The cases and their plain model are in tests/cigar_cases.py, and tests/test_cigar_cases.py has checked on the CPU that every case has the
property it is named for.  Here every case runs through compare() — statistics, histograms, identity sums and the depth of the touched contigs
bit for bit against the oracle — and, so that a record which took the wrong branch with the right depth does not pass, the run word of EVERY
record (cov_copy_run_words: type, start and, for SINGLE / DOUBLE, the packed fields) and the bucket counters of cov_last_paths are compared
with the model's.  Every case runs as a sample k_prep_lean takes and as one k_prep_generic walks alone, under the default kernels,
COVERM_FAST_TABLES=2, COVERM_PILEUP=stream and COVERM_PREP_KERNEL=7.

Read but not tested: merged runs of 2^30 bases and reference skips of 2^31 between two M operations need contigs of gigabases.
"""
import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from oracle import oracle as O
from tests import cigar_cases as cc
from tests.test_gpu_abi_parity import compare

pytestmark = pytest.mark.gpu

CONFIGS = {"default": {}, "two-tables": {"COVERM_FAST_TABLES": "2"}, "stream": {"COVERM_PILEUP": "stream"}, "prep7": {"COVERM_PREP_KERNEL": "7"}}
KNOBS = ("COVERM_FAST_TABLES", "COVERM_PILEUP", "COVERM_PREP_KERNEL")
SIZES = pytest.mark.parametrize("small", [False, True], ids=["lean", "generic-only"])
CONFIG = pytest.mark.parametrize("config", list(CONFIGS))
OFF = O.FlagFilter(True, True, False)

_bams = {}


def configure(monkeypatch, config):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in CONFIGS[config].items():
        monkeypatch.setenv(k, v)


def bam_of(case):
    if case.name not in _bams:
        _bams[case.name] = case.bam()
    return _bams[case.name]


def assert_words(case, got, fp=None):
    want = case.words(fp)
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: %d run words differ, the first at record %d (lane %d%s): device %s, model %s (%s), CIGAR %s" % (
            case.name, len(bad), i, i % 64, ", a deviating record" if i in case.dev else "", cc.decode_word(got[i]), cc.decode_word(want[i]),
            case.verdicts[i].kind, case.recs[i][2][:12]))


def run_case(case, monkeypatch, config, fp=None):
    configure(monkeypatch, config)
    paths, words = {}, []
    compare(bam_of(case), ff=(True, True, False), fp=fp, excl=75, check_depth=case.depth_of, paths_out=paths, run_words_out=words)
    assert_words(case, words[0], fp)
    assert paths["bucket_records"] == case.bucket_records(fp) and paths["bucket_entries"] == case.bucket_entries(fp), (paths, case.bucket_records(fp), case.bucket_entries(fp))
    assert paths["passes"] == (2 if case.bucket_entries(fp) else 1), paths          # (a fresh session: any bucket entry is more than its buffer holds)
    if config != "prep7":
        assert paths["generic_only"] == case.small, paths
    if case.slow_tiles is not None and config != "stream":
        assert paths["slow_tiles"] == case.slow_tiles, paths
    return paths


@CONFIG
@SIZES
@pytest.mark.parametrize("name", sorted(cc.BUILDERS))
def test_case(name, small, config, monkeypatch):
    """Groups A to F of tests/cigar_cases.py: run-word classification at the edges of RW_DOUBLE's fields, zero-length operations and CIGARs
    without M/=/X, the operation-count thresholds, the wave walk's bookkeeping, several long records in one step, k_cx_expand against tiles,
    contig ends and the scan's blocks, and what the three pileup kernels make of DOUBLE, COMPLEX and bucket entries at a tile's borders and
    limits."""
    run_case(cc.build(name, small), monkeypatch, config)


@CONFIG
@SIZES
@pytest.mark.parametrize("name", sorted(cc.HUGE_BUILDERS))
def test_skips_of_two_to_the_24_beside_long_records(name, small, config, monkeypatch):
    """Two records of more than 128 operations at lanes 0 and 63 of a step, between them a record with an N of exactly 2^24 bases (absurd: the
    serial walk; big: never a bucket record) and one of 2^24 - 1 (the ordinary walks, and with 130 operations a bucket record whose entries
    lie 16.8 M bases apart), on a contig of 16.9 M bases."""
    run_case(cc.build(name, small), monkeypatch, config)


@CONFIG
def test_repeated_pass_at_exact_capacity(config, monkeypatch):
    """cov_finish repeats the pipeline when the bucket buffer is smaller than the entries counted, and then reserves T + T / 8 + 1024: a
    sample of T entries in a fresh session takes two passes, one of exactly T + T / 8 + 1024 entries fits, one more entry does not."""
    configure(monkeypatch, config)
    t = 2048
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        for total, passes in [(t, 2), (t + t // 8 + 1024, 1), (t + t // 8 + 1025, 2)]:
            case = cc.case_bucket_entries_exactly(total)
            b = case.bam()
            exp, exp_hist, prim = O.integer_stats(b, OFF, None, 75, None)
            s.reset()
            s.set_targets(case.ref_lens)
            s.push(case.batch())
            st, summ = s.finish()
            paths = s.last_paths()
            assert paths["passes"] == passes and paths["bucket_entries"] == total and paths["bucket_records"] == len(case.dev), (total, paths)
            assert_words(case, s.run_words())
            hist = s.hist()
            live = exp["seen"] == 1
            assert summ.num_detected_primary_alignments == prim
            for f in ("n_primary", "n_pass", "n_nonsupp", "sum_nm", "sum_indel", "win_sum_d", "win_sum_d2", "win_covered", "full_covered", "win_min_d", "win_max_d", "hist_len"):
                np.testing.assert_array_equal(st[f][live], exp[f][live], err_msg="%d entries: %s" % (total, f))
            np.testing.assert_array_equal(st["sum_identity_primary"][live].view(np.uint64), exp["id_primary"][live].view(np.uint64))
            for c in np.nonzero(live)[0]:
                n_b = int(exp["hist_len"][c])
                np.testing.assert_array_equal(hist[int(st["hist_off"][c]):int(st["hist_off"][c]) + n_b], exp_hist[int(exp["hist_off"][c]):int(exp["hist_off"][c]) + n_b])
            np.testing.assert_array_equal(s.depth(0), np.cumsum(O.contig_deltas(b, OFF, 0), dtype=np.int64).astype(np.int32))
            np.testing.assert_array_equal(s.depth(0), case.depth(0))


_Q = np.float32(cc.FILTER_ALIGNED) / np.float32(100)
THRESHOLDS = {"length-at": (dict(min_aligned_length_single=cc.FILTER_ALIGNED), True),
              "length-above": (dict(min_aligned_length_single=cc.FILTER_ALIGNED + 1), False),
              "percent-at": (dict(min_aligned_percent_single=float(_Q)), True),
              "percent-above": (dict(min_aligned_percent_single=float(np.nextafter(_Q, np.float32(1)))), False)}


@CONFIG
@SIZES
@pytest.mark.parametrize("threshold", list(THRESHOLDS))
def test_reader_filter_on_the_walked_aligned_length(threshold, small, config, monkeypatch):
    """One record through each walk (closed form, state machine, whole wave, serial), all of 62 aligned bases in a read of 100: they survive
    min_aligned_length_single = 62 and the f32 quotient 62 / 100 as min_aligned_percent_single, and none survives one more, or the next float."""
    fp, alive = THRESHOLDS[threshold]
    case = cc.build("filter-on-each-walk", small)
    assert all(case.survives(case.verdicts[i], fp) == alive for i in case.dev)
    run_case(case, monkeypatch, config, fp=fp)
    configure(monkeypatch, config)
    with Session(0, FilterConfig(True, True, False, filter_single=True, min_aligned_length=fp.get("min_aligned_length_single", 0),
                                 min_aligned_percent=fp.get("min_aligned_percent_single", 0.0)), 75) as s:
        s.set_targets(case.ref_lens)
        s.push(case.batch())
        st, _ = s.finish()
        assert int(st["n_pass"][0]) == sum(1 for r in case.recs if r[0] == 0) - (0 if alive else len(case.dev))


def test_run_words_need_a_finish_over_the_whole_store():
    """cov_copy_run_words answers COV_ERR_STATE when the last finish left no run words for the store: no finish, no records."""
    from coverm_amd.native import CovError
    case = cc.build("fields-3ops", False)
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(case.ref_lens)
        with pytest.raises(CovError):
            s.run_words()
        s.finish()
        with pytest.raises(CovError):
            s.run_words()
        s.push(case.batch())
        s.finish()
        assert_words(case, s.run_words())
        assert set(s.last_paths()) >= {"listed_steps", "generic_only", "slow_tiles", "bucket_records", "bucket_entries", "passes"}
