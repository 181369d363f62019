"""The device pair filter (cov_pair_filter_apply: csrc/pair_kernels.hip.h and its driver) at its decision points: every sample of
tests/pair_cases.py goes through a written BAM, the device ingest with the mate columns and the filter, and must come out exactly as
oracle.reader_stage returns it — all fields, CIGAR offsets and words, the primary count; the error cases end with the oracle's status and
the reference's message.  The judgement and parking samples, concatenated, also come in as SAM text and as a shuffled BAM grouped on the
device.  tests/test_pair_cases.py proves on the CPU that every sample holds the property it is named for."""
import os

import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd.engine import FilterConfig, Session
from oracle import bamio
from oracle import oracle as O
from tests import binary, pair_cases as P, samtext
from tests.grouping import grouped_order, take_bamdata
from tests.knobs import set_knobs, with_knobs
from tests.test_gpu_pair_filter import _compare
from tests.test_gpu_sam_ingest import feed_text, session_for
from tests.test_sam_parse_core import header_names

pytestmark = pytest.mark.gpu

CASES = P.all_cases()
MESSAGES = {2: "Mapping record encountered that does not have an 'NM' auxiliary tag in the SAM/BAM format", 3: "Unexpected data type of NM aux tag"}


def apply(s, fp):
    fs, fpairs = O.filter_mode(fp)
    assert fpairs
    return cbam.pair_filter_apply(s, fs, fp.min_mapq, (fp.min_aligned_length_single, fp.min_percent_identity_single, fp.min_aligned_percent_single),
                                  (fp.min_aligned_length_pair, fp.min_percent_identity_pair, fp.min_aligned_percent_pair))


def expect(b, fp):
    """(order, primaries, None) or (None, None, the oracle's error code)."""
    try:
        order, prim = O.reader_stage(b, fp)
    except O.OracleError as e:
        return None, None, e.code
    return np.asarray(order, np.int64), prim, None


def check(s, records, oracle_records, fp):
    """The filter over the session's store against the oracle over oracle_records (the same records; other read names where keys were injected)."""
    order, prim, code = expect(oracle_records, fp)
    if code:
        with pytest.raises(RuntimeError) as ei:
            apply(s, fp)
        assert not isinstance(ei.value, cbam.IngestFallback)
        assert str(ei.value) == "cov_pair_filter_apply: %d: %s" % (code, MESSAGES[code])
        return
    nsel, nprim = apply(s, fp)
    got = cbam.session_records(s)
    assert got.n_records == nsel
    _compare(got, records, order)
    assert nprim == prim


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_on_the_device(tmp_path, monkeypatch, case):
    if case.knobs:
        set_knobs(monkeypatch, **case.knobs)
    b = case.bam
    p = str(tmp_path / "s.bam")
    bamio.write_bam(p, b, level=1)
    with Session(0, FilterConfig(), 75) as s:
        assert cbam.gpu_ingest(s, p, threads=2, want_mates=True)[2] == b.n_records
        if case.keys is not None:
            mtid, qh1, qh2 = cbam.session_mates(s, b.n_records)
            np.testing.assert_array_equal(mtid, b.mtid)
            hs = [P._hash(q) for q in b.qname]
            np.testing.assert_array_equal(qh1, np.asarray([h[0] for h in hs], np.uint64))
            cbam.set_mates(s, mtid, case.keys[0], case.keys[1])
            back = cbam.session_mates(s, b.n_records)
            np.testing.assert_array_equal(back[1], case.keys[0])
            np.testing.assert_array_equal(back[2], case.keys[1])
        if case.declined:
            with pytest.raises(cbam.IngestFallback) as ei:
                apply(s, case.fp)
            assert "handing the file to the CPU reader" in str(ei.value)
            _compare(cbam.session_records(s), b, np.arange(b.n_records))          # the decline left the store as the ingest filled it
            return
        check(s, b, case.oracle_bam(), case.fp)
        if case.error is not None:
            assert expect(case.oracle_bam(), case.fp)[2] == case.error


def test_set_mates_states(tmp_path):
    """cov_set_mates has cov_copy_mates' state checks: no mate columns, no hook."""
    b = P.case("parking_abcd").bam
    p = str(tmp_path / "s.bam")
    bamio.write_bam(p, b, level=1)
    n = b.n_records
    z = np.zeros(n, np.int32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    with Session(0, FilterConfig(), 75) as s:
        cbam.gpu_ingest(s, p, threads=2)
        with pytest.raises(RuntimeError) as ei:
            cbam.set_mates(s, *z)
        assert "cov_set_mates: the records were not ingested with cov_ingest_want_mates" in str(ei.value)
        with pytest.raises(RuntimeError):
            cbam.session_mates(s, n)
        with pytest.raises(ValueError):
            cbam.set_mates(s, z[0][:-1], z[1][:-1], z[2][:-1])
    with Session(0, FilterConfig(), 75) as s:
        cbam.gpu_ingest(s, p, threads=2, want_mates=True)
        cbam.set_mates(s, *cbam.session_mates(s, n))                              # what is there, written back: allowed, and nothing changes
        case = P.case("parking_abcd")
        nsel, _ = apply(s, case.fp)
        assert nsel == len(case.order)
        with pytest.raises(RuntimeError) as ei:                                   # the filter has spent the mate columns
            cbam.set_mates(s, z[0][:nsel], z[1][:nsel], z[2][:nsel])
        assert "cov_set_mates: the store holds records without mate columns" in str(ei.value)


@pytest.mark.parametrize("id", ["list_cap_64", "list_cap_66", "list_cap_floor_16", "list_cap_floor_19"])
def test_list_cap_in_the_binary(tmp_path, id):
    """pair_multi_cap = 64: with 64 listed records the device filters, with 66 the file goes to the CPU reader; pair_multi_cap = 1 is taken
    as 16: 16 listed records stay, 19 go.  The table is the oracle's every time."""
    case = P.case(id)
    over = case.declined
    p = str(tmp_path / "s.bam")
    bamio.write_bam(p, case.bam, level=1)
    kw = dict(methods=["mean", "covered_fraction", "count"], min_covered_fraction=0, min_read_percent_identity_pair=0.9)
    r = binary.run_full("contig", [p], env=with_knobs(dict(os.environ, COVERM_CLI_TIMING="1"), **case.knobs), timeout=300, **kw)
    assert r.stdout == O.run_cli("contig", [p], bams=[case.bam], **kw)
    assert r.stdout.count("\n") == 2
    assert ("pair filter on the device" not in r.stderr) == over, r.stderr[-2000:]
    if over:
        assert "more than %d records carry a read name that occurs more than twice" % max(16, case.knobs["pair_multi_cap"]) in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- the other routes into the store
ROUTED = [c for c in CASES if c.group in ("judge", "park")]
FPS = []
for _c in ROUTED:
    if _c.fp not in [f for _, f in FPS]:
        FPS.append((_c.id, _c.fp))


@pytest.fixture(scope="module")
def routed(tmp_path_factory):
    """The judgement and parking samples as one sample (a run of references per case): its SAM text with what the oracle reads from it, and
    the same records shuffled in a BAM with what grouping makes of them."""
    d = tmp_path_factory.mktemp("routed")
    b, _ = P.concatenated(ROUTED)
    text = samtext.render(b, seed=3)
    sam = str(d / "s.sam")
    with open(sam, "wb") as f:
        f.write(text)
    from_sam = bamio.read_sam(sam)
    assert from_sam.n_records == b.n_records and from_sam.qname == b.qname
    sh = take_bamdata(b, np.random.default_rng(4).permutation(b.n_records))
    shuffled = str(d / "shuffled.bam")
    bamio.write_bam(shuffled, sh, level=1)
    return dict(text=text, from_sam=from_sam, shuffled=shuffled, grouped=take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens))))


@pytest.mark.parametrize("fp", [f for _, f in FPS], ids=[i for i, _ in FPS])
def test_sam_text_route(routed, fp):
    want = routed["from_sam"]
    with session_for(want.ref_lens) as s:
        s._check(s._lib.cov_ingest_want_mates(s._h, 1))
        rc, msg, n, _ = feed_text(s, routed["text"], header_names(routed["text"]))
        assert rc == 0 and n == want.n_records, msg
        check(s, want, want, fp)


@pytest.mark.parametrize("fp", [f for _, f in FPS], ids=[i for i, _ in FPS])
def test_grouped_route(routed, fp):
    want = routed["grouped"]
    with Session(0, FilterConfig(), 75) as s:
        assert cbam.gpu_ingest(s, routed["shuffled"], threads=2, want_mates=True, group=True)[2] == want.n_records
        check(s, want, want, fp)


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "nm"], ids=lambda c: c.id)
def test_nm_cases_as_sam_text(tmp_path, case):
    """SAM text has no NM of a signed BAM type: the expected side is the oracle over what it reads from the text."""
    text = samtext.render(case.bam, seed=5)
    p = str(tmp_path / "s.sam")
    with open(p, "wb") as f:
        f.write(text)
    want = bamio.read_sam(p)
    with session_for(want.ref_lens) as s:
        s._check(s._lib.cov_ingest_want_mates(s._h, 1))
        rc, msg, n, _ = feed_text(s, text, header_names(text))
        assert rc == 0 and n == want.n_records, msg
        check(s, want, want, case.fp)
