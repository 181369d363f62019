"""cov_sam_* through the C ABI: SAM text fed in whole-line pieces, decoded on the device into the session's store; cov_copy_records must
equal oracle.bamio.read_sam of the same text column for column — for the SAM fixtures, the SAM rendering of every BAM fixture, generated
special lines and a 2 M-record synthetic sample; with the default window and with windows so small that every input crosses at least three
of them.  Errors name the first offending line in file order and leave the session usable."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from coverm_amd import bam, native, synth
from coverm_amd.engine import FilterConfig, RecordBatch, Session
from oracle import bamio
from tests import samtext
from tests.test_gpu_abi_parity import to_bamdata
from tests.test_sam_parse_core import HDR, blob_of, header_names, rec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RAW_SAM = sorted(glob.glob(os.path.join(HERE, "golden", "raw_sam", "*.sam")))
RAW_BAM = sorted(glob.glob(os.path.join(HERE, "golden", "raw", "*.bam")))
COV_ERR_INVALID_ARG, COV_ERR_STATE, COV_ERR_INGEST_FALLBACK = 16, 18, 19


def lib():
    L = native.lib()
    L.cov_sam_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint64]
    L.cov_sam_window_bytes.argtypes = [C.c_void_p]
    L.cov_sam_window_bytes.restype = C.c_uint64
    L.cov_sam_slot_wait.argtypes = [C.c_void_p, C.c_int]
    L.cov_sam_feed.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_uint64]
    L.cov_sam_end.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.cov_last_error.restype = C.c_char_p
    L.cov_last_error.argtypes = [C.c_void_p]
    L.cov_ingest_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
    L.cov_ingest_abort.argtypes = [C.c_void_p]
    return L


def feed_text(s, text, names, expected=None):
    """(status, message, records, pieces): the text through cov_sam_begin / cov_sam_feed / cov_sam_end, cut as a host driver cuts it."""
    L = lib()
    blob, off = blob_of(names)
    rc = L.cov_sam_begin(s._h, blob, off.ctypes.data, len(names), len(text) if expected is None else expected)
    assert rc == 0, L.cov_last_error(s._h)
    W = int(L.cov_sam_window_bytes(s._h))
    at, k, keep = 0, 0, []
    while at < len(text):
        end = min(len(text), at + W)
        cut = end
        if end < len(text):
            nl = text.rfind(b"\n", at, end)
            cut = nl + 1 if nl >= at else end
        piece = text[at:cut]
        keep.append(piece)                      # (alive until the slot's upload is over)
        assert L.cov_sam_slot_wait(s._h, k % 4) == 0
        rc = L.cov_sam_feed(s._h, k % 4, piece, len(piece))
        if rc:
            return rc, L.cov_last_error(s._h).decode(), 0, k
        at, k = cut, k + 1
    n = C.c_uint64(0)
    rc = L.cov_sam_end(s._h, C.byref(n))
    for j in range(4):
        L.cov_sam_slot_wait(s._h, j)
    return rc, L.cov_last_error(s._h).decode(), int(n.value), k


def session_for(lens):
    s = Session(0, FilterConfig(), 75)
    s.set_targets(np.asarray(lens, np.int64))
    return s


def assert_store_equals(s, want):
    got = bam.session_records(s)
    assert len(got.tid) == want.n_records
    for k in ("tid", "pos", "flag", "mapq", "nm", "nm_kind"):
        np.testing.assert_array_equal(getattr(got, k), np.asarray(getattr(want, k)), err_msg=k)
    np.testing.assert_array_equal(got.l_seq, np.asarray(want.l_seq).astype(np.uint32))
    np.testing.assert_array_equal(got.cigar_off, want.cigar_off)
    np.testing.assert_array_equal(got.cigar, want.cigar)


def check_text(text, tmp_path, monkeypatch, small_windows=True):
    p = str(tmp_path / "t.sam")
    with open(p, "wb") as f:
        f.write(text)
    want = bamio.read_sam(p)
    names = header_names(text)
    longest = max(len(l) for l in text.split(b"\n")) + 2
    for window in ([None, max(longest, len(text) // 5, 256)] if small_windows else [None]):
        if window:
            monkeypatch.setenv("COVERM_KNOBS", "sam_window_bytes=%d" % window)
        else:
            monkeypatch.delenv("COVERM_KNOBS", raising=False)
        with session_for(want.ref_lens) as s:
            rc, msg, n, pieces = feed_text(s, text, names)
            assert rc == 0, msg
            assert n == want.n_records
            if window and window < len(text) // 3:
                assert pieces >= 3, (pieces, window, len(text))          # the input crossed at least three windows, lines carried over their ends
            assert_store_equals(s, want)
            ms, launches = s.sam_kernel_ms()
            assert ms > 0 and launches > 0
    return want


@pytest.mark.parametrize("path", RAW_SAM, ids=os.path.basename)
def test_sam_fixtures(tmp_path, monkeypatch, path):
    with open(path, "rb") as f:
        check_text(f.read(), tmp_path, monkeypatch)


@pytest.mark.parametrize("path", RAW_BAM, ids=os.path.basename)
def test_rendered_bam_fixtures(tmp_path, monkeypatch, path):
    b = bamio.read_bam(path)
    want = check_text(samtext.render(b, seed=3), tmp_path, monkeypatch)
    np.testing.assert_array_equal(want.tid, b.tid)


def test_generated_lines_and_mates(tmp_path, monkeypatch):
    body = b"\n".join([rec(rname=b"*", cigar=b"*", seq=b"*"), rec(rnext=b"="), rec(rname=b"c2", rnext=b"c1"), rec(tags=(b"NM:i:3", b"XS:i:2", b"NM:i:9")),
                       rec(tags=()), rec(cigar=b"3S4M2I1D5=6X7N8H9P"), rec(qn=b"a-rather-longer-read-name/1", flag=99, rnext=b"=")])
    hdr = b"@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:2000\n"      # (no duplicate SN here: the oracle's reader keeps the last of two, the engine's readers the first)
    for text in (hdr + body + b"\n", hdr + body, hdr.replace(b"\n", b"\r\n") + b"\r\n" + body.replace(b"\n", b"\r\n\r\n")):
        check_text(text, tmp_path, monkeypatch)
    # lines the oracle's reader does not take: the values parse_sam's rules give (tests/test_sam_parse_core.py states them)
    odd = b"\n".join([rec(rname=b"nope", rnext=b"="), rec(tags=(b"NM:i:-1",)), rec(tags=(b"NM:Z:x",)), rec(tags=(b"NM:i:",)), rec(tags=(b"NM:i:3", b"NM:Z:x")), rec(cigar=b"4M1Q")]) + b"\n"
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    with session_for([1000, 2000, 77]) as s:
        s._check(s._lib.cov_ingest_want_mates(s._h, 1))
        rc, msg, n, _ = feed_text(s, HDR + odd, [b"c1", b"c2", b"c1"])
        assert rc == 0 and n == 6, msg
        got = bam.session_records(s)
        np.testing.assert_array_equal(got.tid, [-1, 0, 0, 0, 0, 0])
        np.testing.assert_array_equal(got.nm_kind, [1, 2, 2, 0, 2, 1])
        np.testing.assert_array_equal(got.nm, [1, 0, 0, 0, 3, 1])
        np.testing.assert_array_equal(got.cigar[-2:], [4 << 4, 1 << 4 | 15])
        s._check(s._lib.cov_ingest_want_mates(s._h, 0))


def test_errors_and_states(monkeypatch):
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    L = lib()
    good = rec()
    nine = b"\t".join(good.split(b"\t")[:9])
    names = [b"c1", b"c2", b"c1"]
    batch = RecordBatch(np.asarray([0], np.int32), np.asarray([4], np.int32), np.asarray([0], np.uint16), np.asarray([30], np.uint8), np.asarray([0], np.uint32),
                        np.asarray([1], np.uint8), np.asarray([10], np.uint32), np.asarray([0, 1], np.uint32), np.asarray([10 << 4], np.uint32))
    with session_for([1000, 2000, 77]) as s:
        for text, word, line in [(HDR + good + b"\n" + good + b"\n" + nine + b"\n" + nine + b"\n", "malformed SAM line", 7),
                                 (HDR + good + b"\n" + rec(cigar=b"1M1I" * 35_000, seq=b"*") + b"\n" + nine + b"\n", "65535", 6)]:
            rc, msg, _, _ = feed_text(s, text, names)
            assert rc == COV_ERR_INVALID_ARG and word in msg and "line %d)" % line in msg, msg
            s.push(batch)                                                   # the session is usable: nothing of the failed ingest is in the store
            st, summ = s.finish()
            assert summ.n_records == 1 and st["n_pass"][0] == 1
            s.reset()
        rc, msg, _, _ = feed_text(s, HDR + good + b"\n@CO\tlate\n" + good + b"\n", names)
        assert rc == COV_ERR_INGEST_FALLBACK and "line 6)" in msg, msg
        s.reset()
        monkeypatch.setenv("COVERM_KNOBS", "sam_window_bytes=256")
        rc, msg, _, _ = feed_text(s, HDR + good + b"\n" + rec(seq=b"ACGT" * 100) + b"\n" + good + b"\n", names)
        assert rc == COV_ERR_INVALID_ARG and "longer than the decode window" in msg and "line 6)" in msg, msg
        monkeypatch.delenv("COVERM_KNOBS", raising=False)
        s.reset()
        # state errors
        assert L.cov_sam_feed(s._h, 0, good, len(good)) == COV_ERR_STATE
        assert L.cov_sam_end(s._h, None) == COV_ERR_STATE
        assert L.cov_ingest_begin(s._h, 1 << 20, 0, 1) == 0
        assert L.cov_sam_begin(s._h, b"", None, 0, 0) == COV_ERR_STATE
        assert L.cov_ingest_abort(s._h) == 0
        rc, msg, n, _ = feed_text(s, HDR + good + b"\n", names)
        assert rc == 0 and n == 1, msg


def test_two_million_records(tmp_path, monkeypatch):
    """A synthetic sample of 2 M records over 400 contigs, default window (several windows of 32 MiB), the size announced and not (a pipe's
    expected_bytes = 0: the store grows as records arrive).  The expectation is read_sam of the same text, read in ten parts."""
    monkeypatch.delenv("COVERM_KNOBS", raising=False)
    ref = synth.make_reference(400, 40_000_000, seed=11, min_len=1500, max_len=400_000)
    b = to_bamdata(synth.make_reads(ref, 2_000_000, seed=12), ref.lengths, ref.names)
    b.l_seq = np.minimum(np.asarray(b.l_seq), 24).astype(b.l_seq.dtype)      # (a short SEQ keeps the text near 200 MB)
    n = b.n_records
    parts, wants, header = [], [], None
    for k in range(10):
        text = samtext.render(b.select(np.arange(k * n // 10, (k + 1) * n // 10)), seed=20 + k)
        p = str(tmp_path / "part.sam")
        with open(p, "wb") as f:
            f.write(text)
        wants.append(bamio.read_sam(p))
        first = 0
        while text[first:first + 1] == b"@":                 # the header: the lines in front of the first alignment line
            first = text.index(b"\n", first) + 1
        header = text[:first]
        parts.append(text[first:])
    text = header + b"".join(parts)
    cat = lambda k: np.concatenate([np.asarray(getattr(w, k)) for w in wants])
    ncig = np.concatenate([np.diff(w.cigar_off.astype(np.int64)) for w in wants])
    for expected in (None, 0):
        with session_for(ref.lengths) as s:
            rc, msg, got_n, pieces = feed_text(s, text, header_names(header), expected=expected)
            assert rc == 0 and got_n == n and pieces >= 3, (msg, got_n, pieces)
            got = bam.session_records(s)
            for k in ("tid", "pos", "flag", "mapq", "nm", "nm_kind"):
                np.testing.assert_array_equal(getattr(got, k), cat(k), err_msg=k)
            np.testing.assert_array_equal(got.l_seq, cat("l_seq").astype(np.uint32))
            np.testing.assert_array_equal(np.diff(got.cigar_off.astype(np.int64)), ncig)
            np.testing.assert_array_equal(got.cigar, cat("cigar"))
