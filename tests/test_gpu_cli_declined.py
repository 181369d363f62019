"""The binary over files its device readers hand back.  A BAM whose second BGZF block carries a second (empty) extra subfield is declined
by the device ingest (tests/test_gpu_ingest.py shows the same block through the ABI); a SAM file with a header line behind its first
alignment line is declined by the device's SAM decode.  Whatever reader takes over, the table is the table of the regular file and the
oracle's; under COVERM_CLI_TIMING stderr names the reason and the reader that took the file.  From a pipe there is no second reader: the
run ends with a message."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import bamio
from oracle import oracle as O
from tests import binary
from tests.grouping import grouped_order, shuffles, take_bamdata
from tests.test_host_golden import _paired_sample
from tests.test_sam_parse_core import rec

pytestmark = pytest.mark.gpu

TIMING = {"COVERM_CLI_TIMING": "1"}
METHODS = dict(methods=["mean", "covered_fraction", "count"], min_covered_fraction=0)
PAIR = dict(min_read_percent_identity_pair=0.95, proper_pairs_only=True)


def with_extra_subfield(raw):
    """The file with its second BGZF block (the first behind the one that holds the header) given a second, empty subfield "XX":
    XLEN 6 -> 10, BSIZE + 4.  The same records."""
    q = int.from_bytes(raw[16:18], "little") + 1
    bs = int.from_bytes(raw[q + 16:q + 18], "little") + 1
    assert raw[q:q + 4] == b"\x1f\x8b\x08\x04" and raw[q + 12:q + 14] == b"BC" and q + bs < len(raw) - 28
    blk = raw[q:q + 10] + struct.pack("<H", 10) + b"BC\x02\0" + struct.pack("<H", bs + 4 - 1) + b"XX\0\0" + raw[q + 18:q + bs]
    return raw[:q] + blk + raw[q + bs:]


def write_pair(d, name, records):
    """good/s.bam and odd/s.bam under d/name (one file stem: one sample name in every table)."""
    paths = {}
    for kind in ("good", "odd"):
        os.makedirs(str(d / name / kind))
        paths[kind] = str(d / name / kind / "s.bam")
    bamio.write_bam(paths["good"], records, level=1)
    with open(paths["good"], "rb") as f:
        raw = f.read()
    with open(paths["odd"], "wb") as f:
        f.write(with_extra_subfield(raw))
    assert bamio.read_bam(paths["odd"]).n_records == records.n_records
    return paths


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("declined")
    b = _paired_sample(10_000, seed=53)                     # about 20 000 reads over its five contigs
    assert 19_000 < b.n_records < 20_001
    sh = take_bamdata(b, shuffles(len(b.tid), 54, b.qname)["name"])
    lines = ["##gff-version 3"]
    rng = np.random.default_rng(55)
    for t, (n, l) in enumerate(zip(b.ref_names, b.ref_lens)):
        for k in range(3):
            a = int(rng.integers(1, max(2, l - 600)))
            lines.append("%s\tx\tCDS\t%d\t%d\t.\t+\t0\tID=g%d_%d" % (n, a, min(int(l), a + int(rng.integers(50, 500))), t, k))
    gff = d / "s.gff"
    gff.write_text("\n".join(lines) + "\n")
    return {"sorted": (write_pair(d, "sorted", b), b), "shuffled": (write_pair(d, "shuffled", sh), take_bamdata(sh, grouped_order(sh.tid, len(sh.ref_lens)))),
            "gff": str(gff)}


def run(path, extra=(), stdin=None, **kw):
    return subprocess.run(binary.argv("contig", [path], **kw) + list(extra), capture_output=True, text=True, timeout=300, env=dict(os.environ, **TIMING),
                          stdin=stdin if stdin is not None else subprocess.DEVNULL)


def check_declined(paths, records, took_over, extra=(), **kw):
    good, odd = run(paths["good"], extra, **kw), run(paths["odd"], extra, **kw)
    assert good.returncode == 0 and odd.returncode == 0, (good.stderr[-2000:], odd.stderr[-2000:])
    assert "sample s: device ingest" in good.stderr and "subfield" not in good.stderr, good.stderr[-2000:]
    assert odd.stdout == good.stdout
    assert odd.stdout == O.run_cli("contig", [paths["odd"]], bams=[records], **kw)
    assert odd.stdout.count("\n") > 3
    assert "subfield" in odd.stderr and "sample s: %s" % took_over in odd.stderr, odd.stderr[-2000:]
    return odd


def test_plain_run_goes_to_the_streamed_reader(files):
    paths, b = files["sorted"]
    check_declined(paths, b, "streamed", **METHODS)


def test_pair_mode_filter_goes_to_the_whole_file_reader(files):
    paths, b = files["sorted"]
    odd = check_declined(paths, b, "whole file", **METHODS, **PAIR)
    assert "pair filter on the device" not in odd.stderr


def test_gff_goes_to_the_whole_file_reader(files):
    paths, b = files["sorted"]
    odd = check_declined(paths, b, "whole file", **METHODS, gff=files["gff"])
    assert "records came back" not in odd.stderr


def test_unsorted_goes_to_the_streamed_reader(files):
    paths, grouped = files["shuffled"]
    check_declined(paths, grouped, "streamed", extra=["--unsorted"], **METHODS)


def test_declined_sam_text_file_and_pipe(tmp_path):
    """A header line behind the first alignment line: the device decode hands the text back (COV_ERR_INGEST_FALLBACK).  A file is read
    again on the host; standard input cannot be."""
    hdr = b"@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:2000\n"
    text = hdr + rec() + b"\n@CO\tlate\n" + rec(rname=b"c2", pos=40) + b"\n"
    p = str(tmp_path / "s.sam")
    with open(p, "wb") as f:
        f.write(text)
    kw = dict(methods=["mean", "count"], min_covered_fraction=0)
    r = run(p, **kw)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "handed to the host route" in r.stderr and "sample s: whole file" in r.stderr, r.stderr[-2000:]
    assert r.stdout == O.run_cli("contig", [p], bams=[bamio.read_sam(p)], **kw)
    assert r.stdout.count("\n") == 3                       # the header line and the two contigs
    with open(p, "rb") as f:
        r = run("-", stdin=f, **kw)
    assert r.returncode != 0 and "a pipe cannot be read again" in r.stderr and "\n" not in r.stdout.strip(), (r.stdout, r.stderr[-2000:])
