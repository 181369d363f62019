"""The long-CIGAR cases of tests/cigar_cases.py on the CPU: the oracle accepts every one of them, the plain model's depth is the oracle's, and
every case has the property it is named for — a case that has lost its property is a bug of its builder and must not reach
tests/test_gpu_cigar_paths.py as a pass that means nothing."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import cigar_cases as cc

OFF = O.FlagFilter(True, True, False)
NAMES = sorted(cc.BUILDERS) + sorted(cc.HUGE_BUILDERS)


def _first(ops, pred, start=0):
    return next(i for i in range(start, len(ops)) if pred(ops[i]))


def check_expect(case, i, exp):
    tid, pos, ops = case.recs[i]
    v = case.verdicts[i]
    L = int(case.ref_lens[tid])
    what = "%s record %d %s" % (case.name, i, exp)
    for k, want in exp.items():
        if k in ("kind", "n_runs", "len1", "len2", "gap", "aligned", "n_ops", "big"):
            assert getattr(v, k) == want, (what, k, getattr(v, k))
        elif k == "gap_index":
            assert ops[want] == (4, "D"), what
            gaps = [j for j, o in enumerate(ops) if o[1] in "DN" and o[0] > 0]
            assert want in gaps and len(gaps) == v.n_runs - 1, what
        elif k == "first_match":
            assert _first(ops, lambda o: o[1] in "M=X") == want and all(o[1] == "I" for o in ops[:want]), what
        elif k == "second_run_first_op":
            g = _first(ops, lambda o: o[1] in "DN")
            assert _first(ops, lambda o: o[1] in "M=X", g) == want, what
        elif k == "op_tiles":
            s, e = [(s, e) for _, s, e in v.entries][-1]
            assert sum(1 for _, s2, e2 in v.entries if (s2, e2) == (s, e)) == want, (what, v.entries[-6:])
        elif k == "run1_end":
            assert v.runs[0][1] == want, what
        elif k == "gap_over":
            assert v.runs[0][1] < want < v.runs[1][0], what
        elif k == "run2_start":
            assert v.runs[1][0] == want, what
        elif k == "run2_past":
            assert want == L and v.runs[1][0] < L < v.runs[1][1], what
        elif k == "run2_end":
            assert want == L and v.runs[1][1] == L, what
        elif k == "tiles_of_runs":
            assert len({s // cc.TILE for s, _ in v.runs}) == want, what
        else:
            raise AssertionError("unknown expectation %s" % k)
    if v.kind == "DOUBLE":      # the decoded word says what the model says
        assert cc.decode_word(v.word) == ("DOUBLE", v.runs[0][0], (v.len1, v.gap, v.len2)), what


@pytest.mark.parametrize("small", [False, True], ids=["lean", "generic-only"])
@pytest.mark.parametrize("name", NAMES)
def test_case_is_accepted_and_has_its_property(name, small):
    case = cc.build(name, small)
    b = case.bam()
    O.integer_stats(b, OFF, None, 75, None)                                      # raises on a record the reference would refuse
    for t in case.depth_of:
        np.testing.assert_array_equal(np.cumsum(O.contig_deltas(b, OFF, t), dtype=np.int64).astype(np.int32), case.depth(t), err_msg="contig %d" % t)
    # the sample: sorted by position inside a contig, and of the size that picks the prep kernel
    tid = np.asarray([r[0] for r in case.recs])
    pos = np.asarray([r[1] for r in case.recs])
    assert (np.diff(tid) >= 0).all() and ((np.diff(pos) >= 0) | (np.diff(tid) > 0)).all()
    assert (case.n < 128 * len(case.ref_lens)) == small
    assert case.n <= 11_000
    # the deviating records: where the case wants them, what the case wants them to be; every other record is a 100M read
    assert len(case.dev) == len(case.expect) and len(set(case.dev)) == len(case.dev)
    for i, exp in zip(case.dev, case.expect):
        check_expect(case, i, exp)
    if not case.lanes_free:
        assert all(i % 64 in cc.LANES for i in case.dev) or "long-records" in case.name, [i % 64 for i in case.dev]
    others = set(range(case.n)) - set(case.dev)
    assert all(case.recs[i][2] == cc.BG and case.verdicts[i].kind == "SINGLE" for i in others)
    if case.case_property is not None:
        case.case_property(case)


def test_lanes_of_the_records_that_share_a_step():
    for small in (False, True):
        c = cc.build("long-records-two", small)
        assert [i % 64 for i in c.dev] == [0, 63] and c.dev[0] // 64 == c.dev[1] // 64
        c = cc.build("long-records-three", small)
        assert [i % 64 for i in c.dev] == [30, 31, 32] and len({i // 64 for i in c.dev}) == 1
        c = cc.build("long-records-all-64", small)
        assert [i % 64 for i in c.dev] == list(range(64)) and len({i // 64 for i in c.dev}) == 1
        assert all(c.verdicts[i].n_ops > 128 for i in c.dev)
        for name in cc.HUGE_BUILDERS:
            c = cc.build(name, small)
            assert c.dev[0] % 64 == 0 and c.dev[1] == c.dev[0] + 63 and sorted(c.dev[2:]) == [c.dev[0] + 1, c.dev[0] + 2]
            assert [c.verdicts[i].big for i in c.dev] == [False, False, True, False]


def test_one_deviating_record_per_step_where_the_case_is_about_the_step():
    """Operation counts: the record sits among 63 one-operation records (the step's trip count is an __any, the closed form an __all)."""
    for name in ("op-counts-1runs", "op-counts-2runs", "op-counts-3runs", "fields-3ops", "fields-11ops", "fields-40ops", "fields-131ops"):
        for small in (False, True):
            c = cc.build(name, small)
            assert len({i // 64 for i in c.dev}) == len(c.dev)
    c = cc.build("op-counts-2runs", False)
    assert sorted(c.verdicts[i].n_ops for i in c.dev) == sorted(cc.OP_COUNTS)
    c = cc.build("op-counts-3runs", False)
    assert sorted(c.verdicts[i].n_ops for i in c.dev) == sorted(n for n in cc.OP_COUNTS if n > 4)


def test_field_edges_are_all_there():
    for n_ops in (3, 11, 40, 131):
        c = cc.build("fields-%dops" % n_ops, False)
        vs = [c.verdicts[i] for i in c.dev]
        assert all(v.n_ops == n_ops and v.n_runs == 2 for v in vs)
        assert {v.len1 for v in vs} >= {1, 1023, 1024} and {v.len2 for v in vs} >= {1, 1023, 1024} and {v.gap for v in vs} >= {1, 255, 256}
        doubles = [v for v in vs if v.kind == "DOUBLE"]
        assert len(doubles) == 8 and len(vs) == 12
        assert sum(v.len1 == 1023 for v in doubles) == 1 and sum(v.len2 == 1023 for v in doubles) == 1 and sum(v.gap == 255 for v in doubles) == 2
        assert {v.kind for v in vs if v.kind != "DOUBLE"} == {"BUCKET" if n_ops > 16 else "COMPLEX"}


def test_exact_entry_counts_of_the_repeated_pass():
    t = 2048
    for total in (t, t + t // 8 + 1024, t + t // 8 + 1025):
        c = cc.case_bucket_entries_exactly(total)
        assert c.bucket_entries() == total and all(c.verdicts[i].kind == "BUCKET" for i in c.dev)
        O.integer_stats(c.bam(), OFF, None, 75, None)
        np.testing.assert_array_equal(np.cumsum(O.contig_deltas(c.bam(), OFF, 0), dtype=np.int64).astype(np.int32), c.depth(0))


def test_filter_thresholds_flip_exactly_the_four_records():
    c = cc.build("filter-on-each-walk", False)
    a = cc.FILTER_ALIGNED
    q = np.float32(a) / np.float32(100)
    for fp, alive in [(dict(min_aligned_length_single=a), True), (dict(min_aligned_length_single=a + 1), False),
                      (dict(min_aligned_percent_single=float(q)), True), (dict(min_aligned_percent_single=float(np.nextafter(q, np.float32(1)))), False)]:
        ofp = O.FilterParameters(OFF, **fp)
        order, _ = O.reader_stage(c.bam(), ofp)
        kept = set(int(i) for i in order)
        assert all((i in kept) == alive for i in c.dev), fp
        assert all(i in kept for i in range(c.n) if i not in c.dev)
        assert [i in kept for i in range(c.n)] == [c.survives(v, fp) for v in c.verdicts]
