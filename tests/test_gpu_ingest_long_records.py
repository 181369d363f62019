"""Device ingest of long-read BAM files (csrc/bam_record_core.h, k_bam_find / k_bam_extract_long / the repair in k_bam_verify): records
with multi-kilobyte tags, dozens of tags, thousands of CIGAR words and record-shaped bytes inside a B array go through the device ingest
field for field like the CPU reader's, the search still cuts the stream at every 32 KiB segment (cov_ingest_last_stats), and a false start
is dropped on the device instead of costing the whole file."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from coverm_amd import bam as cbam
from coverm_amd.engine import FilterConfig, Session
from oracle import bamio
from oracle import oracle as O
from tests import binary
from tests.bamraw import bgzf, header, ingest_and_compare, rec
from tests.knobs import with_knobs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_core = open(os.path.join(ROOT, "coverm_amd", "csrc", "bam_record_core.h")).read()
T_WORDS = int(re.search(r"LONG_CIGAR_WORDS = (\d+)u", _core).group(1))
T_AUX = int(re.search(r"LONG_AUX_BYTES = (\d+)u", _core).group(1))
SEG = 32768
REPAIR_BUDGET = int(re.search(r"REPAIR_BUDGET = (\d+)", open(os.path.join(ROOT, "coverm_amd", "csrc", "ingest_kernels.hip.h")).read()).group(1))
ELEM = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


# ------------------------------------------------------------------------------------------------ a small BAM writer (tests/bamraw.py)
def write(path, refs, records):
    """records: the triples rec() returns.  Returns what the file holds: long records by the core header's rule, the smallest record."""
    open(path, "wb").write(bgzf(header(refs) + b"".join(r[0] for r in records)))
    return dict(n=len(records), long=sum(1 for _, w, a in records if w > T_WORDS or a > T_AUX), smallest=min(len(r[0]) for r in records))


def cigar_of(n_words):
    """n words: 2M 1I 2M 1I ... — an even count ends in a soft clip instead of an insertion"""
    c = np.empty(n_words, np.uint32)
    c[0::2] = (2 << 4) | 0
    c[1::2] = (1 << 4) | 1
    if n_words % 2 == 0:
        c[-1] = (1 << 4) | 4
    return c


def shape(c):
    c = np.asarray(c, np.uint32)
    return int((c >> 4)[np.isin(c & 15, (0, 1, 4, 7, 8))].sum()), int((c >> 4)[np.isin(c & 15, (0, 2, 3, 7, 8))].sum())      # l_seq, reference span


def text(n, seed):
    """n bytes of tag text that no record image hides in and that does not deflate to nothing"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 10, n, dtype=np.uint8) + 48).tobytes()


def binary_run(paths, extra=(), **kw):
    r = subprocess.run(binary.argv("contig", paths, **kw) + list(extra), capture_output=True, text=True, timeout=300, env=dict(os.environ, COVERM_CLI_TIMING="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return r


# ------------------------------------------------------------------------------------------------ A: long tags
@pytest.fixture(scope="module")
def long_tags(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("long_tags") / "s.bam")
    lens = [4096, 4097, 9000, 40_000, 70_000]
    records = [rec(0, 1000 + 3000 * i, [100 << 4], 100, b"NMC" + bytes([i % 7]) + b"MMZ" + text(lens[i % 5], i) + b"\0", b"r%d" % i) for i in range(600)]
    return p, write(p, [(b"chr", 2_000_000)], records)


def test_long_tags(long_tags):
    """600 records whose MM:Z (4096 ... 70 000 bytes) crosses 32 KiB segments and BGZF blocks: every one is a long record, no start needs a
    repair, and the search still finds a start wherever a record starts.
    The bound on the longest hop, derived: with every start found, the lane of a segment hops the records that start in its own 32 KiB —
    at most ceil(32768 / smallest record) of them — and, in the last live segment in front of a window's end, the at most 8 records
    behind them that cannot head an 8-chain."""
    p, meta = long_tags
    _, stats = ingest_and_compare(p)
    assert meta["long"] == 600 and stats["long_records"] == meta["long"]
    assert stats["repaired_starts"] == 0
    bound = -(-SEG // meta["smallest"]) + 8
    print("max_hop_records", stats["max_hop_records"], "bound", bound, "segments", stats["segments"], "with start", stats["segments_with_start"])
    assert stats["max_hop_records"] <= bound


def test_long_tags_through_the_binary(long_tags):
    p, meta = long_tags
    kw = dict(methods=["mean", "variance", "count"])
    want = O.run_cli("contig", [p], bams=[bamio.read_alignment_file(p)], **kw)
    for extra in ([], ["--unsorted"]):
        r = binary_run([p], extra, **kw)
        assert r.stdout == want
        line = [x for x in r.stderr.splitlines() if "device ingest: first upload" in x]
        assert len(line) == 1 and "long records %d, repaired starts 0, longest hop " % meta["long"] in line[0], r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ B: many tags
def test_many_tags(tmp_path):
    """40 tags of every type per record, NM the 36th"""
    def aux(i):
        t = []
        kinds = [lambda k: b"X%dA" % (k % 10) + b"k", lambda k: b"X%dc" % (k % 10) + struct.pack("<b", -k), lambda k: b"X%dC" % (k % 10) + bytes([k]),
                 lambda k: b"X%ds" % (k % 10) + struct.pack("<h", -k), lambda k: b"X%dS" % (k % 10) + struct.pack("<H", k), lambda k: b"X%di" % (k % 10) + struct.pack("<i", -k),
                 lambda k: b"X%dI" % (k % 10) + struct.pack("<I", k), lambda k: b"X%df" % (k % 10) + struct.pack("<f", k), lambda k: b"X%dZ" % (k % 10) + b"z" * ((i + k) % 23) + b"\0",
                 lambda k: b"X%dH" % (k % 10) + b"1F" * (k % 4) + b"\0"]
        subs = [b"c", b"C", b"s", b"S", b"i", b"I", b"f"]
        for k in range(40):
            if k == 35:
                t.append(b"NMC" + bytes([i % 11]))
            elif k % 11 == 10:
                st = subs[(k // 11 + i) % 7]
                t.append(b"Y%dB" % (k % 10) + st + struct.pack("<I", (i + k) % 5) + b"\3" * (((i + k) % 5) * ELEM[st]))
            else:
                t.append(kinds[(k + i) % 10](k))
        return b"".join(t)
    records = [rec(i // 1000, 500 + 700 * (i % 1000), [60 << 4, (2 << 4) | 1, 38 << 4], 100, aux(i), b"m%d" % i) for i in range(2000)]
    p = str(tmp_path / "s.bam")
    meta = write(p, [(b"a", 1_000_000), (b"b", 1_000_000)], records)
    whole, stats = ingest_and_compare(p)
    assert (whole.records.nm_kind == 1).all()
    assert stats["long_records"] == meta["long"] and stats["repaired_starts"] == 0


# ------------------------------------------------------------------------------------------------ C: CIGAR thresholds
def test_cigar_thresholds(tmp_path):
    """CIGARs on both sides of every threshold of k_bam_extract (<= 4 words wait in LDS, more go out directly, more than T go to
    k_bam_extract_long), the longest the field holds, and one that only fits CG:B,I, behind an 8 kB string.  Ordinary records stand
    between them, so long and ordinary records interleave inside one lane's piece."""
    counts = [1, 4, 5, T_WORDS - 1, T_WORDS, T_WORDS + 1, 255, 4097, 65_535]
    records, pos = [], 1000
    for rep in range(2):
        for j, n in enumerate(counts + [70_001]):
            c = cigar_of(n)
            l_seq, span = shape(c)
            aux = b"NMC" + bytes([j + 1]) + (b"XZZ" + text(8000, j) + b"\0" if n == 70_001 else b"")
            records.append(rec(0, pos, c, l_seq, aux, b"c%d_%d" % (rep, n)))
            pos += 50
            for x in range(1 + j % 3):
                records.append(rec(0, pos, [80 << 4], 80, b"NMC\2", b"o%d" % pos))
                pos += 50
    p = str(tmp_path / "s.bam")
    meta = write(p, [(b"chr", 4_000_000)], records)
    assert meta["long"] == 2 * 5                 # T + 1, 255, 4097, 65 535 words and the CG record (T and fewer words with 4 tag bytes are ordinary)
    whole, stats = ingest_and_compare(p)
    assert int(np.diff(whole.records.cigar_off.astype(np.int64)).max()) == 70_001
    assert stats["long_records"] == meta["long"] and stats["repaired_starts"] == 0


# ------------------------------------------------------------------------------------------------ D: many windows
def test_long_reads_in_many_windows(tmp_path):
    """(its own process: the knobs are read once per process)"""
    env = with_knobs(os.environ, ingest_round_blocks=64, ingest_carry_kb=1024)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ingest_long_windows_worker.py"), str(tmp_path)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "LONG_WINDOWS_OK" in r.stdout


# ------------------------------------------------------------------------------------------------ E, F: false starts
def false_start_file(path, n_false):
    """One record whose XB:B,C array holds, at the beginning of each of the n_false 32 KiB segments behind the one the record starts in,
    eight well-formed record images (plausible against the header, their tags exact).  The file is one window, where buffer offset =
    carry area + inflated offset and the carry area is a multiple of 32 KiB: segment boundaries are the inflated offsets k * 32 KiB."""
    refs = [(b"chr", 3_000_000)]
    data = header(refs)
    records = [rec(0, 100 + 10 * i, [90 << 4], 90, b"NMC\1", b"a%d" % i) for i in range(40)]
    at = len(data) + sum(len(r[0]) for r in records)           # where the carrier starts
    images = b"".join(rec(0, 5000 + i, [50 << 4], 50, b"NMC\3ASi" + struct.pack("<i", i), b"img%d" % i)[0] for i in range(8))
    name = b"carrier"
    array_at = at + 4 + 32 + len(name) + 1 + 4 + 50 + 100 + 4 + 3 + 1 + 4         # ... CIGAR, seq, qual, NM:C, `XB` `B` `C` count
    first = (at // SEG + 1) * SEG
    assert array_at < first
    arr = bytearray((n_false + 1) * SEG + 16_384 if n_false > 1 else 80 << 10)
    for k in range(n_false):
        o = first + k * SEG - array_at + 24
        arr[o:o + len(images)] = images
    carrier = rec(0, 600, [100 << 4], 100, b"NMC\2" + b"XBBC" + struct.pack("<I", len(arr)) + bytes(arr), name)
    assert array_at == at + len(carrier[0]) - len(arr)
    records.append(carrier)
    records += [rec(0, 700 + 10 * i, [90 << 4], 90, b"NMC\1", b"b%d" % i) for i in range(50)]
    write(path, refs, records)
    return [(first + k * SEG + 24) // SEG for k in range(n_false)]


def test_a_false_start_is_dropped_on_the_device(tmp_path):
    p = str(tmp_path / "s.bam")
    segs = false_start_file(p, 1)
    whole, stats = ingest_and_compare(p)                           # (raises IngestFallback if the device gave up)
    assert whole.records.n_records == 91
    assert stats["repaired_starts"] >= 1, "the images missed their segment (%r): no false start was made" % segs
    kw = dict(methods=["mean", "variance", "count"])
    r = binary_run([p], **kw)
    assert r.stdout == O.run_cli("contig", [p], bams=[bamio.read_alignment_file(p)], **kw)
    assert "sample s: device ingest" in r.stderr and "streamed" not in r.stderr, r.stderr[-2000:]
    assert "repaired starts %d," % stats["repaired_starts"] in r.stderr


def test_false_starts_beyond_the_repair_budget_hand_the_file_back(tmp_path):
    p = str(tmp_path / "s.bam")
    false_start_file(p, REPAIR_BUDGET + 6)
    whole = cbam.read_alignment_file(p, threads=2, want_names=False)
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        with pytest.raises(cbam.IngestFallback) as ei:
            cbam.gpu_ingest(s, p, threads=2)
        assert "record boundaries did not verify" in str(ei.value)
        assert cbam.ingest_stats(s)["repaired_starts"] == REPAIR_BUDGET
        assert cbam.session_records(s).n_records == 0
        s.push(whole.records)
        st, su = s.finish()
        h = s.hist()
    with Session(0, FilterConfig(), 75, want_hist=True, want_identity=True) as s:
        s.set_targets(whole.ref_lens)
        s.push(whole.records)
        st2, su2 = s.finish()
        assert st.tobytes() == st2.tobytes() and (h == s.hist()).all() and su.n_records == su2.n_records == 91
