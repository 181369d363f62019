"""Runs in its own process (the window size of the device ingest is read once per process): tests/test_gpu_ingest_long_records.py sets
COVERM_KNOBS ingest_round_blocks / ingest_carry_kb so that a file of long reads is parsed in many small windows — nearly every window ends
inside a record, and the long records (MD:Z, ML:B,C, thousands of CIGAR words, NM last) come out of the carry area.
argv: a scratch directory."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coverm_amd import bam as cbam, synth  # noqa: E402
from coverm_amd.engine import FilterConfig, Session  # noqa: E402
from tests import namehash  # noqa: E402
from tests.bamraw import FIELDS, rec  # noqa: E402
from tests.test_gpu_ingest_long_records import text, write  # noqa: E402

tmp = sys.argv[1]
ref = synth.make_reference(40, 6_000_000, seed=18, min_len=5000, max_len=800_000)
b = synth.make_long_reads(ref, 300, seed=29, mean_len=20_000)
records, names = [], []
for i in range(b.n_records):
    l_seq = int(b.l_seq[i])
    aux = b"MDZ" + text(l_seq // 10, i) + b"\0" + b"MLBC" + struct.pack("<I", l_seq // 10) + bytes([i % 251]) * (l_seq // 10) + b"NMS" + struct.pack("<H", int(b.nm[i]) % 65_536)
    names.append(b"read/%d" % i)
    records.append(rec(int(b.tid[i]), int(b.pos[i]), b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])], l_seq, aux, names[-1]))
p = os.path.join(tmp, "s.bam")
meta = write(p, [(n.encode(), int(x)) for n, x in zip(ref.names, ref.lengths)], records)
whole = cbam.read_alignment_file(p, threads=2, want_names=False)
R = whole.records.n_records
assert R == 300 and meta["long"] == 300
with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
    for rep in range(2):        # the second file goes behind the first in the same store
        _, _, n, _ = cbam.gpu_ingest(s, p, threads=4)
        assert n == R, (n, R)
        st = cbam.ingest_stats(s)
        assert st["windows"] >= 4 and st["long_records"] == 300 and st["repaired_starts"] == 0, st
    got = cbam.session_records(s)
    assert got.n_records == 2 * R
    for f in FIELDS[:7]:
        a = getattr(got, f)
        np.testing.assert_array_equal(a[:R], getattr(whole.records, f), err_msg=f)
        np.testing.assert_array_equal(a[R:], getattr(whole.records, f), err_msg=f + " (second file)")
    C = int(whole.records.cigar_off[-1])
    np.testing.assert_array_equal(got.cigar_off[:R + 1], whole.records.cigar_off)
    np.testing.assert_array_equal(got.cigar_off[R:] - C, whole.records.cigar_off)
    np.testing.assert_array_equal(got.cigar[:C], whole.records.cigar)
    np.testing.assert_array_equal(got.cigar[C:], whole.records.cigar)
k1, k2 = namehash.name_hashes(names)
with Session(0, FilterConfig(), 75) as s:       # mate columns stay where k_bam_extract writes them
    _, _, n, _ = cbam.gpu_ingest(s, p, threads=4, want_mates=True)
    assert n == R
    got = cbam.session_records(s)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(whole.records, f), err_msg=f)
    mtid, qh1, qh2 = cbam.session_mates(s, n)
    np.testing.assert_array_equal(mtid, whole.mtid)
    np.testing.assert_array_equal(qh1, k1)
    np.testing.assert_array_equal(qh2, k2)
print("LONG_WINDOWS_OK windows=%d records=%d" % (st["windows"], R))
