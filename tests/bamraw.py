"""A small BAM writer over raw bytes, and the comparison of a device ingest with the CPU reader: shared by the GPU tests that build their
files byte by byte (test_gpu_ingest_long_records.py, test_gpu_inflate_edges.py)."""
import struct
import zlib

import numpy as np

from coverm_amd import bam as cbam
from coverm_amd.engine import FilterConfig, Session
from oracle import bamio

FIELDS = ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq", "cigar_off", "cigar")


def rec(tid, pos, cigar, l_seq, aux, name=b"q"):
    cigar = np.asarray(cigar, np.uint32)
    placeholder = None
    if len(cigar) > 65535:        # SAM spec 4.2.2: `<l_seq>S<ref span>N` in the CIGAR field, the real one in CG:B,I behind the other tags
        span = int((cigar >> 4)[np.isin(cigar & 15, (0, 2, 3, 7, 8))].sum())
        placeholder, aux = cigar, aux + b"CGBI" + struct.pack("<I", len(cigar)) + cigar.tobytes()
        cigar = np.array([(l_seq << 4) | 4, (span << 4) | 3], np.uint32)
    core = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 30, 4680, len(cigar), 0, l_seq, -1, -1, 0)
    body = core + name + b"\0" + cigar.tobytes() + b"\x11" * ((l_seq + 1) // 2) + b"\xff" * l_seq + aux
    words = len(placeholder) if placeholder is not None else len(cigar)
    return struct.pack("<i", len(body)) + body, words, len(aux)


def header(refs):
    h = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", len(refs))
    for name, length in refs:
        h += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return h


def bgzf(data, block=0xff00):
    out = []
    for s0 in range(0, len(data), block):
        chunk = data[s0:s0 + block]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    return b"".join(out)


def ingest_and_compare(path, session_kw=None, **kw):
    """The device ingest's nine columns equal the CPU reader's, finish() statistics and histogram equal those of a session that was pushed
    the same records.  Returns the CPU reader's file and the ingest's stats."""
    whole = cbam.read_alignment_file(path, threads=2, want_names=False)
    ob = bamio.read_bam(path)
    assert ob.n_records == whole.records.n_records
    np.testing.assert_array_equal(np.asarray(ob.pos), whole.records.pos)
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        names, lens, n, _ = cbam.gpu_ingest(s, path, threads=2, **kw)
        stats = cbam.ingest_stats(s)
        assert names == whole.ref_names and n == whole.records.n_records
        got = cbam.session_records(s)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(got, f), getattr(whole.records, f), err_msg=f)
        st_gpu, su_gpu = s.finish()
        h_gpu = s.hist()
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        s.set_targets(whole.ref_lens)
        s.push(whole.records)
        st, su = s.finish()
        h = s.hist()
    assert st_gpu.tobytes() == st.tobytes() and (h_gpu == h).all()
    assert su_gpu.num_detected_primary_alignments == su.num_detected_primary_alignments
    assert stats["records"] == n
    return whole, stats
