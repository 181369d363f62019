"""Reader-stage pair filter on the device (cov_pair_filter_apply, csrc/pair_kernels.hip.h): over what the device ingest extracted
(mate reference + read-name hash) it must select exactly the records, in exactly the order, that the oracle's restatement of
ReferenceSortedBamFilter::read (filter.rs:117-228) returns — on the reference's own filter goldens, on synthetic pairs at scale,
with read names that repeat (the park / take-out sequence), and across table chunks."""
import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd.engine import FilterConfig, Session
from oracle import bamio
from oracle import oracle as O
from tests.fixtures import load_fixture
from tests.golden import cases
from tests.test_host_golden import _paired_sample
from tests.knobs import set_knobs

pytestmark = pytest.mark.gpu
FIELDS = ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq")


def _device_selection(path, ofp, threads=3):
    fs, fpairs = O.filter_mode(ofp)
    assert fpairs
    with Session(0, FilterConfig(), 75) as s:
        cbam.gpu_ingest(s, path, threads=threads, want_mates=True)
        nsel, nprim = cbam.pair_filter_apply(s, fs, ofp.min_mapq, (ofp.min_aligned_length_single, ofp.min_percent_identity_single, ofp.min_aligned_percent_single),
                                             (ofp.min_aligned_length_pair, ofp.min_percent_identity_pair, ofp.min_aligned_percent_pair))
        got = cbam.session_records(s)
    assert got.n_records == nsel
    return got, nprim


def _expect(b, ofp):
    order, prim = O.reader_stage(b, ofp)
    return np.asarray(order, dtype=np.int64), prim


def _compare(got, b, order):
    assert got.n_records == len(order)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), np.asarray(getattr(b, f))[order].astype(getattr(got, f).dtype), err_msg=f)
    ncig = (b.cigar_off[1:].astype(np.int64) - b.cigar_off[:-1].astype(np.int64))[order]
    np.testing.assert_array_equal(np.diff(got.cigar_off.astype(np.int64)), ncig)
    exp_cig = np.concatenate([b.cigar[b.cigar_off[i]:b.cigar_off[i + 1]] for i in order]) if len(order) else np.zeros(0, np.uint32)
    np.testing.assert_array_equal(got.cigar, exp_cig)


PAIR_CASES = [c for c in cases.FILTER_CASES if c.get("mode") in ((False, True), (True, True), None)]


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: c["id"])
def test_reference_filter_goldens_on_the_device(tmp_path, case):
    """filter.rs:342-844: the expected read-name sequences of the reference's own tests, device ingest forced."""
    d = load_fixture(case["bam"])
    p = str(tmp_path / "f.bam")
    bamio.write_bam(p, d, level=6)
    ofp = O.FilterParameters(O.FlagFilter(*case["ff"]), case["single"][0], case["single"][1], case["single"][2], case["mapq"],
                             case["pair"][0], case["pair"][1], case["pair"][2])
    if not O.filter_mode(ofp)[1]:
        pytest.skip("single-read branch (k_prep)")
    got, nprim = _device_selection(p, ofp)
    order, prim = _expect(d, ofp)
    _compare(got, d, order)
    assert nprim == prim
    if "count" in case:
        assert got.n_records == case["count"]
    elif case.get("exhaustive"):
        assert [d.qname[i].decode() for i in order] == case["qnames"]


@pytest.mark.parametrize("chunk", [0, 2048])
@pytest.mark.parametrize("params", [dict(min_percent_identity_pair=0.95), dict(min_aligned_length_pair=200, min_mapq=20),
                                    dict(min_percent_identity_single=0.9, min_aligned_percent_pair=0.8), dict(min_mapq=30, proper=True)])
def test_synthetic_pairs_with_repeated_names(tmp_path, monkeypatch, params, chunk):
    """40 k synthetic pairs: mates on other contigs, missing mates, improper pairs, secondary records and ~2 % of the names used by two
    or more pairs (entries with more than two records: collected, replayed in file order, judged).  chunk = 2048: dozens of table
    chunks cut at reference boundaries."""
    if chunk:
        set_knobs(monkeypatch, pair_chunk=chunk)
    params = dict(params)
    proper = params.pop("proper", False)
    b = _paired_sample(40_000, seed=3)
    p = str(tmp_path / "pairs.bam")
    bamio.write_bam(p, b, level=1)
    ofp = O.FilterParameters(O.FlagFilter(not proper, True, False), **params)
    got, nprim = _device_selection(p, ofp)
    order, prim = _expect(b, ofp)
    assert len(order) > 1000
    _compare(got, b, order)
    assert nprim == prim


def _adjacent_pairs(n):
    """n records on one contig: record 0 alone (its mate is not in the file), then the pairs (1, 2), (3, 4), ...; an even n leaves the last
    record alone as well.  Every third pair misses the identity bound and every fifth record has a CIGAR of three words, so neither scan's
    items (two slots at a kept pair's second record; a selected record's CIGAR words) are all equal."""
    i = np.arange(n)
    pair = (i + 1) // 2                                        # 0: record 0; k >= 1: records 2 k - 1 and 2 k
    alone = (i == 0) | ((i == n - 1) & (n % 2 == 0))
    second = ~alone & (i % 2 == 0)
    flag = np.where(second, 147, 99).astype(np.uint16)
    nm = np.where(pair % 3 == 0, 40, i % 4).astype(np.uint32)
    three = i % 5 == 0
    n_ops = np.where(three, 3, 1)
    coff = np.zeros(n + 1, np.uint32)
    np.cumsum(n_ops, out=coff[1:])
    cigar = np.zeros(int(coff[-1]), np.uint32)
    cigar[coff[:-1]] = np.where(three, 50 << 4, 100 << 4)
    cigar[coff[:-1][three] + 1] = (2 << 4) | 1                 # 50M 2I 50M
    cigar[coff[:-1][three] + 2] = 50 << 4
    z = np.zeros(n, np.int32)
    return bamio.BamData(["c0"], np.asarray([10 * n + 1000], np.int64), z, (10 * i).astype(np.int32), flag, np.full(n, 30, np.uint8),
                         np.where(three, 102, 100).astype(np.int32), nm, np.ones(n, np.uint8), coff, cigar, z, z, z,
                         [b"q%d" % (n + k if a else p) for k, (p, a) in enumerate(zip(pair, alone))], "")


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_the_scan_blocks_of_4096_records(tmp_path, n):
    """The device-wide scan takes 4 096 items per workgroup, and the pair filter's items are the records: one item short of a block, a whole
    block, one item into the second block (the kept pair 4 095 | 4 096 lies on both sides of the border), one item into the third."""
    b = _adjacent_pairs(n)
    p = str(tmp_path / "edge.bam")
    bamio.write_bam(p, b, level=1)
    ofp = O.FilterParameters(O.FlagFilter(True, True, False), min_percent_identity_pair=0.95)
    got, nprim = _device_selection(p, ofp, threads=2)
    order, prim = _expect(b, ofp)
    kept = (n - 1) // 2 - (n - 1) // 6                            # the pairs 1 .. (n - 1) / 2 but for every third
    assert len(order) == 2 * kept and (n < 4097 or {4095, 4096} <= set(order.tolist())) and (n < 8193 or {8191, 8192} <= set(order.tolist()))
    _compare(got, b, order)
    assert nprim == prim


def test_missing_nm_in_a_judged_pair_is_the_references_panic(tmp_path):
    b = _paired_sample(3_000, seed=5)
    ofp = O.FilterParameters(O.FlagFilter(True, True, False), min_percent_identity_pair=0.9)
    order, _ = _expect(b, ofp)
    b.nm_kind[order[len(order) // 2]] = bamio.NM_ABSENT
    p = str(tmp_path / "nonm.bam")
    bamio.write_bam(p, b, level=1)
    with pytest.raises(RuntimeError) as ei:
        _device_selection(p, ofp)
    assert "does not have an 'NM' auxiliary tag" in str(ei.value)


def test_pair_filter_needs_mate_columns(tmp_path):
    b = _paired_sample(500, seed=6)
    p = str(tmp_path / "x.bam")
    bamio.write_bam(p, b, level=1)
    with Session(0, FilterConfig(), 75) as s:
        cbam.gpu_ingest(s, p, threads=2)
        with pytest.raises(RuntimeError):
            cbam.pair_filter_apply(s, False, 255, pair=(1, 0.0, 0.0))
