"""`coverm-amd depth` end to end: over a fixture BAM, over the same records as SAM text on a pipe with --unsorted, and over two BAM files,
the bedGraph equals Python's rendering of the oracle's depth runs, with and without --no-zeros and with forced small chunks."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio
from oracle import oracle as O
from tests import binary, samtext
from tests import depth_runs_ref as R
from tests.grouping import grouped_order, take_bamdata
from tests.knobs import with_knobs

pytestmark = pytest.mark.gpu

RAW = os.path.join(binary.ROOT, "tests", "golden", "raw")
A, B = "7seqs.reads_for_seq1_and_seq2.bam", "2seqs.bad_read.1.with_supplementary.bam"


def want(b, sample, ff=(True, True, False), fp=None, no_zeros=False):
    off = O.FlagFilter(*ff)
    ofp = O.FilterParameters(off, **fp) if fp else None
    order, _ = O.reader_stage(b, ofp)
    depths = [np.cumsum(O.contig_deltas(b, off, t, order), dtype=np.int64).astype(np.int32) for t in range(len(b.ref_lens))]
    ro, start, depth = R.runs_of(depths)
    return 'track type=bedGraph name="%s"\n' % sample + R.bedgraph(b.ref_names, b.ref_lens, ro, start, depth, no_zeros)


def depth(paths, extra=(), env=None, stdin=None):
    r = subprocess.run([binary.BIN, "depth", "-b"] + list(paths) + ["-t", "4"] + list(extra), capture_output=True, text=True, timeout=300,
                       env=env or dict(os.environ), stdin=stdin if stdin is not None else subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_fixture_bam(tmp_path):
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    full = want(b, A[:-4])
    assert depth([p]) == full and full.count("\n") > 10
    assert depth([p], ["--no-zeros"]) == want(b, A[:-4], no_zeros=True)
    assert depth([p], env=with_knobs(os.environ, depth_chunk_bases=2048)) == full
    assert depth([p], ["--no-stream"]) == full
    out = str(tmp_path / "a.bedgraph")
    assert depth([p], ["-o", out]) == ""
    with open(out) as fh:
        assert fh.read() == full
    assert depth([p], ["--min-read-percent-identity", "0.99", "--include-secondary"]) == want(b, A[:-4], ff=(True, True, True), fp=dict(min_percent_identity_single=0.99))
    assert depth([p], ["--proper-pairs-only", "--exclude-supplementary"]) == want(b, A[:-4], ff=(False, False, False))


def test_sam_on_a_pipe_unsorted():
    b = bamio.read_bam(os.path.join(RAW, A))
    rev = take_bamdata(b, np.arange(len(b.tid))[::-1])      # the last reference's records first
    text = samtext.render(rev, seed=5)
    grouped = take_bamdata(rev, grouped_order(rev.tid, len(rev.ref_lens)))
    for extra, nz in ((["--unsorted"], False), (["--unsorted", "--no-zeros"], True)):
        r = subprocess.run([binary.BIN, "depth", "-b", "-", "-t", "4"] + extra, input=text, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.decode() == want(grouped, "stdin", no_zeros=nz)


def test_two_bams_two_tracks():
    pa, pb = os.path.join(RAW, A), os.path.join(RAW, B)
    got = depth([pa, pb])
    assert got == want(bamio.read_bam(pa), A[:-4]) + want(bamio.read_bam(pb), B[:-4])
    assert got.count("track type=bedGraph") == 2
    assert depth([pa, pb], ["--no-zeros"]) == want(bamio.read_bam(pa), A[:-4], no_zeros=True) + want(bamio.read_bam(pb), B[:-4], no_zeros=True)


def test_a_spilled_sample_ends_the_run():
    from coverm_amd import synth
    import tempfile
    ref = synth.make_reference(12, 200_000, seed=3, min_len=1500, max_len=40_000)
    batch = synth.make_reads(ref, 30_000, seed=4)
    from tests.test_gpu_abi_parity import to_bamdata
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "big.bam")
        bamio.write_bam(p, to_bamdata(batch, ref.lengths, ref.names), level=1)
        # (the streamed CPU reader pushes a window of the file at a time: the store passes its cap between two pushes)
        r = subprocess.run([binary.BIN, "depth", "-b", p], capture_output=True, text=True, timeout=300,
                           env=with_knobs(dict(os.environ, COVERM_NO_GPU_INGEST="1"), store_cap_records=10000, store_cap_cigar=100000, stream_window_kb=64))
    assert r.returncode == 1 and r.stdout.count("\n") <= 1 and "cov_depth_runs_compute: part of the sample's records already left the bounded record store" in r.stderr
