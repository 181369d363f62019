"""What the device SAM decode keeps for the pair filter, looked at directly (cov_copy_mates): the mate's reference equals
oracle.bamio.read_sam's mtid and the 96-bit read-name hash equals the hash written out in tests/namehash.py over the oracle's QNAMEs —
and equals what the BGZF extraction keeps for the same reads in a BAM.  Also here: the bounded record store's spill under cov_sam_feed,
and the Python face (Session.sam_ingest, bam.gpu_ingest dispatching on the format, a pipe's read end)."""
import glob
import os
import threading

import numpy as np
import pytest

from coverm_amd import bam, synth
from coverm_amd.engine import FilterConfig, Session
from oracle import bamio
from tests import namehash, samtext
from tests.knobs import set_knobs
from tests.test_gpu_sam_ingest import assert_store_equals, feed_text, session_for
from tests.test_host_golden import _paired_sample
from tests.test_sam_parse_core import header_names

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RAW_SAM = sorted(glob.glob(os.path.join(HERE, "golden", "raw_sam", "*.sam")))
RAW_BAM = sorted(glob.glob(os.path.join(HERE, "golden", "raw", "*.bam")))


def check_mates(text, tmp_path, monkeypatch):
    p = str(tmp_path / "t.sam")
    with open(p, "wb") as f:
        f.write(text)
    want = bamio.read_sam(p)
    k1, k2 = namehash.name_hashes(want.qname)
    longest = max(len(l) for l in text.split(b"\n")) + 2
    for window in (None, max(longest, len(text) // 5, 256)):
        if window:
            monkeypatch.setenv("COVERM_KNOBS", "sam_window_bytes=%d" % window)
        else:
            monkeypatch.delenv("COVERM_KNOBS", raising=False)
        with session_for(want.ref_lens) as s:
            s._check(s._lib.cov_ingest_want_mates(s._h, 1))
            rc, msg, n, _ = feed_text(s, text, header_names(text))
            assert rc == 0 and n == want.n_records, msg
            assert_store_equals(s, want)
            mtid, qh1, qh2 = bam.session_mates(s, n)
            np.testing.assert_array_equal(mtid, np.asarray(want.mtid))
            np.testing.assert_array_equal(qh1, k1)
            np.testing.assert_array_equal(qh2, k2)
    return want


@pytest.mark.parametrize("path", RAW_SAM, ids=os.path.basename)
def test_sam_fixtures(tmp_path, monkeypatch, path):
    with open(path, "rb") as f:
        check_mates(f.read(), tmp_path, monkeypatch)


def test_paired_sample(tmp_path, monkeypatch):
    b = _paired_sample(20_000, seed=33)
    want = check_mates(samtext.render(b, seed=5), tmp_path, monkeypatch)
    assert want.qname == b.qname and len(set(want.qname)) > 5_000


def test_same_hashes_as_the_bam_extraction(tmp_path, monkeypatch):
    """The same reads as a BAM (BGZF ingest) and as SAM text: the two device routes keep the same mate columns."""
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    compared = 0
    for path in RAW_BAM:
        b = bamio.read_bam(path)
        if not b.qname or b.n_records == 0:
            continue
        with Session(0, FilterConfig(), 75) as s:
            try:
                _, _, n, _ = bam.gpu_ingest(s, path, threads=2, want_mates=True)
            except bam.IngestFallback:
                continue                                                  # (a file the BGZF route hands back with mates wanted: nothing to compare)
            from_bam = bam.session_mates(s, n)
        text = samtext.render(b, seed=6)
        with session_for(b.ref_lens) as s:
            s._check(s._lib.cov_ingest_want_mates(s._h, 1))
            rc, msg, n2, _ = feed_text(s, text, header_names(text))
            assert rc == 0 and n2 == n, msg
            from_sam = bam.session_mates(s, n)
        for x, y, k in zip(from_bam, from_sam, ("mtid", "qh1", "qh2")):
            np.testing.assert_array_equal(x, y, err_msg="%s %s" % (os.path.basename(path), k))
        compared += 1
    assert compared >= 1


def test_spill_of_the_bounded_store(tmp_path, monkeypatch):
    """A store cap of 20 000 records under 150 000 reads in windows of 2 MB: cov_sam_feed spills the complete contigs as cov_push_batch
    does, and the statistics equal those of the same records pushed into a session without a cap."""
    ref = synth.make_reference(200, 20_000_000, seed=91, min_len=1500, max_len=400_000)
    batch = synth.make_reads(ref, 150_000, seed=92)
    from tests.test_gpu_abi_parity import to_bamdata
    text = samtext.render(to_bamdata(batch, ref.lengths, ref.names), seed=12)
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref.lengths)
        s.push(batch)
        want_st, want_summ = s.finish()
    set_knobs(monkeypatch, store_cap_records=20000, store_cap_cigar=200000, sam_window_bytes=2_000_000)
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(ref.lengths)
        rc, msg, n, pieces = feed_text(s, text, header_names(text))
        assert rc == 0 and n == batch.n_records and pieces >= 5, (msg, n, pieces)
        st, summ = s.finish()
        assert s.store_spills() >= 3
        assert int(summ.n_records) == batch.n_records
        for k in st.dtype.names:
            np.testing.assert_array_equal(st[k], want_st[k], err_msg=k)


def test_python_face(tmp_path, monkeypatch):
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    b = _paired_sample(5_000, seed=35)
    p = str(tmp_path / "s.sam")
    samtext.write(p, b, seed=13)
    want = bamio.read_sam(p)
    with Session(0, FilterConfig(), 75) as s:
        names, lens, n, t = s.sam_ingest(p, mates=True)
        assert names == list(want.ref_names) and list(lens) == list(want.ref_lens) and n == want.n_records and t["total"] > 0
        assert_store_equals(s, want)
        np.testing.assert_array_equal(bam.session_mates(s, n)[0], np.asarray(want.mtid))
        s.reset()
        assert bam.gpu_ingest(s, p, threads=2)[2] == want.n_records          # not BGZF: dispatched to the SAM decode
        assert_store_equals(s, want)
        s.reset()
        rd, wr = os.pipe()
        with open(p, "rb") as f:
            text = f.read()

        def writer():
            with os.fdopen(wr, "wb", buffering=0) as w:
                for at in range(0, len(text), 4096):
                    w.write(text[at:at + 4096])

        th = threading.Thread(target=writer)
        th.start()
        try:
            with os.fdopen(rd, "rb") as r:
                assert s.sam_ingest(r)[2] == want.n_records
        finally:
            th.join()
        assert_store_equals(s, want)
