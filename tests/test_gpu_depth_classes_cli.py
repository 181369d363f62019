"""`coverm-amd depth --quantize / --thresholds` end to end: over a fixture BAM and over the same records as SAM text on a pipe, the output
equals the renderers of tests/depth_classes_ref.py over the oracle's depth, byte for byte: the quantised track, the threshold counts of a BED
file's regions in the file's order, and the threshold counts of fixed windows."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio
from tests import binary, samtext
from tests import depth_classes_ref as K
from tests import depth_regions_ref as G
from tests.grouping import grouped_order, take_bamdata
from tests.knobs import with_knobs
from tests.test_gpu_depth_bins_cli import oracle_depths
from tests.test_gpu_depth_regions_cli import RAW, A, bed_file, regions_for

pytestmark = pytest.mark.gpu


def want_classes(b, sample, spec):
    cuts, open_end = K.parse_quantize(spec)
    off, start, cls = K.class_runs_of(oracle_depths(b), cuts)
    return 'track name="%s" description="depth classes %s"\n' % (sample, spec) + K.render_classes(b.ref_names, b.ref_lens, off, start, cls, cuts, open_end)


def want_regions(b, sample, regs, names, thr, no_zeros=False):
    depths = oracle_depths(b)
    res = G.reduce(depths, regs)
    return 'track type=bedGraph name="%s"\n#thresholds\t%s\n' % (sample, "\t".join(map(str, thr))) + K.render_counts(b.ref_names, regs, K.counts(depths, regs, thr), res["max"], no_zeros, names)


def want_windows(b, sample, bs, thr, no_zeros=False):
    regs = [(t, j * bs, min((j + 1) * bs, int(n))) for t, n in enumerate(b.ref_lens) for j in range((int(n) + bs - 1) // bs)]
    return want_regions(b, sample, regs, None, thr, no_zeros)


def depth(paths, extra=(), env=None, stdin_bytes=None):
    r = subprocess.run([binary.BIN, "depth", "-b"] + list(paths) + ["-t", "4"] + list(extra), capture_output=True, timeout=300, env=env or dict(os.environ),
                       **(dict(input=stdin_bytes) if stdin_bytes is not None else dict(stdin=subprocess.DEVNULL)))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.decode()


def test_fixture_bam(tmp_path):
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    sample = A[:-4]
    for spec in ("0:1:5:", "1:2", ":"):
        full = want_classes(b, sample, spec)
        assert depth([p], ["--quantize", spec]) == full
    full = want_classes(b, sample, "0:1:5:")
    assert "\t0:1\n" in full and "\t1:5\n" in full and full.count("\n") > 8
    assert depth([p], ["--quantize", "0:1:5:"], env=with_knobs(os.environ, depth_chunk_bases=2048)) == full
    regs, names = regions_for(b)
    bed = bed_file(tmp_path, b, regs, names)
    got = depth([p], ["--regions", bed, "--thresholds", "1,2,4"])
    assert got == want_regions(b, sample, regs, names, (1, 2, 4)) and got.count("\n") == len(regs) + 2 and "\tgene 3;x\t" in got
    assert depth([p], ["--thresholds", "1,2,4", "--no-zeros", "--regions", bed]) == want_regions(b, sample, regs, names, (1, 2, 4), no_zeros=True)
    assert depth([p], ["--regions", bed, "--thresholds", "1,2,4"], env=with_knobs(os.environ, depth_chunk_bases=2048)) == got
    for bs in (100, 7):
        assert depth([p], ["--bin-size", str(bs), "--thresholds", "1,2"]) == want_windows(b, sample, bs, (1, 2))
    assert depth([p], ["--bin-size", "100", "--thresholds", "1,2", "--no-zeros"]) == want_windows(b, sample, 100, (1, 2), no_zeros=True)
    # the plain tracks behind them, in one process each, are what they were
    out = str(tmp_path / "q.txt")
    assert depth([p], ["--quantize", "0:1:5:", "-o", out]) == ""
    with open(out) as fh:
        assert fh.read() == full


def test_sam_on_a_pipe_unsorted(tmp_path):
    b = bamio.read_bam(os.path.join(RAW, A))
    rev = take_bamdata(b, np.arange(len(b.tid))[::-1])      # the last reference's records first
    text = samtext.render(rev, seed=5)
    grouped = take_bamdata(rev, grouped_order(rev.tid, len(rev.ref_lens)))
    regs, names = regions_for(b, 4)
    bed = bed_file(tmp_path, b, regs, names)
    assert depth(["-"], ["--unsorted", "--quantize", "0:1:5:"], stdin_bytes=text) == want_classes(grouped, "stdin", "0:1:5:")
    assert depth(["-"], ["--unsorted", "--regions", bed, "--thresholds", "1,2,4"], stdin_bytes=text) == want_regions(grouped, "stdin", regs, names, (1, 2, 4))
    assert depth(["-"], ["--unsorted", "--bin-size", "100", "--thresholds", "1,2"], stdin_bytes=text) == want_windows(grouped, "stdin", 100, (1, 2))


def test_two_samples_two_tracks(tmp_path):
    """The thresholds are set per sample and cleared behind it: the second sample's plain session state is the first one's."""
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    got = depth([p, p], ["--bin-size", "100", "--thresholds", "1,2"])
    assert got == want_windows(b, A[:-4], 100, (1, 2)) * 2
