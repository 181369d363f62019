"""`coverm-amd depth --bin-size` end to end: over a fixture BAM for every --bin-value, with --no-zeros, with forced small chunks, over the same
records as SAM text on a pipe with --unsorted, and over two BAM files, the bedGraph equals Python's rendering of the oracle's depth reduced by
numpy; without --bin-size the output is the run track it was."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio
from oracle import oracle as O
from tests import binary, samtext
from tests import depth_bins_ref as B
from tests import depth_runs_ref as R
from tests.grouping import grouped_order, take_bamdata
from tests.knobs import with_knobs

pytestmark = pytest.mark.gpu

RAW = os.path.join(binary.ROOT, "tests", "golden", "raw")
A, A2 = "7seqs.reads_for_seq1_and_seq2.bam", "2seqs.bad_read.1.with_supplementary.bam"


def oracle_depths(b, ff=(True, True, False), fp=None):
    off = O.FlagFilter(*ff)
    ofp = O.FilterParameters(off, **fp) if fp else None
    order, _ = O.reader_stage(b, ofp)
    return [np.cumsum(O.contig_deltas(b, off, t, order), dtype=np.int64).astype(np.int32) for t in range(len(b.ref_lens))]


def want(b, sample, bs, value="mean", no_zeros=False, **kw):
    off, bins = B.bins_of(oracle_depths(b, **kw), bs)
    return 'track type=bedGraph name="%s"\n' % sample + B.bedgraph(b.ref_names, b.ref_lens, off, bins, bs, value, no_zeros)


def depth(paths, extra=(), env=None):
    r = subprocess.run([binary.BIN, "depth", "-b"] + list(paths) + ["-t", "4"] + list(extra), capture_output=True, text=True, timeout=300,
                       env=env or dict(os.environ), stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_fixture_bam_every_value(tmp_path):
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    full = want(b, A[:-4], 100)
    assert depth([p], ["--bin-size", "100"]) == full and full.count("\n") > 10
    for value in B.VALUES:
        assert depth([p], ["--bin-size", "100", "--bin-value", value]) == want(b, A[:-4], 100, value)
        assert depth([p], ["--bin-value", value, "--no-zeros", "--bin-size", "100"]) == want(b, A[:-4], 100, value, no_zeros=True)
    assert want(b, A[:-4], 100, no_zeros=True) != full
    assert depth([p], ["--bin-size", "100"], env=with_knobs(os.environ, depth_chunk_bases=2048)) == full
    assert depth([p], ["--bin-size", "7", "--bin-value", "sum"]) == want(b, A[:-4], 7, "sum")
    out = str(tmp_path / "a.bedgraph")
    assert depth([p], ["--bin-size", "100", "-o", out]) == ""
    with open(out) as fh:
        assert fh.read() == full
    assert depth([p], ["--bin-size", "100", "--min-read-percent-identity", "0.99", "--include-secondary"]) == \
        want(b, A[:-4], 100, ff=(True, True, True), fp=dict(min_percent_identity_single=0.99))


def test_sam_on_a_pipe_unsorted():
    b = bamio.read_bam(os.path.join(RAW, A))
    rev = take_bamdata(b, np.arange(len(b.tid))[::-1])      # the last reference's records first
    text = samtext.render(rev, seed=5)
    grouped = take_bamdata(rev, grouped_order(rev.tid, len(rev.ref_lens)))
    for extra, nz in ((["--unsorted"], False), (["--unsorted", "--no-zeros"], True)):
        r = subprocess.run([binary.BIN, "depth", "-b", "-", "-t", "4", "--bin-size", "100", "--bin-value", "max"] + extra, input=text, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.decode() == want(grouped, "stdin", 100, "max", no_zeros=nz)


def test_two_bams_two_tracks():
    pa, pb = os.path.join(RAW, A), os.path.join(RAW, A2)
    got = depth([pa, pb], ["--bin-size", "100"])
    assert got == want(bamio.read_bam(pa), A[:-4], 100) + want(bamio.read_bam(pb), A2[:-4], 100)
    assert got.count("track type=bedGraph") == 2


def test_without_bin_size_the_output_is_the_run_track():
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    ro, start, d = R.runs_of(oracle_depths(b))
    for extra, nz in (([], False), (["--no-zeros"], True)):
        assert depth([p], extra) == 'track type=bedGraph name="%s"\n' % A[:-4] + R.bedgraph(b.ref_names, b.ref_lens, ro, start, d, nz)


def test_the_timing_line_counts_the_bins():
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    r = subprocess.run([binary.BIN, "depth", "-b", p, "--bin-size", "100", "-o", os.devnull], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, COVERM_CLI_TIMING="1"), stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    n = sum((int(L) + 99) // 100 for L in b.ref_lens)
    assert "depth bins of 100: %d bins computed, fetched and written in" % n in r.stderr
