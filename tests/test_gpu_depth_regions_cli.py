"""`coverm-amd depth --regions` end to end: over a fixture BAM for every --bin-value, with --no-zeros, with forced small chunks, with -o, under
a read filter, over the same records as SAM text on a pipe with --unsorted, and over two BAM files (each resolved against its own header), the
output equals Python's rendering of the oracle's depth sliced by numpy, in the BED file's order, names echoed; the refusals exit non-zero with
their message."""
import os
import subprocess

import numpy as np
import pytest

from oracle import bamio
from tests import binary, samtext
from tests import depth_regions_ref as G
from tests.grouping import grouped_order, take_bamdata
from tests.knobs import with_knobs
from tests.test_gpu_depth_bins_cli import oracle_depths

pytestmark = pytest.mark.gpu

RAW = os.path.join(binary.ROOT, "tests", "golden", "raw")
A, A2 = "7seqs.reads_for_seq1_and_seq2.bam", "shard1.bam"      # (shard1: the last four references of the seven, so at other tids)


def regions_for(b, seed=3):
    """The edge and random sets over the file's references, shuffled so that the file's order is not the target order; every third has a name."""
    sets = G.region_sets([int(L) for L in b.ref_lens], seed)
    regs = sets["edges"] + sets["random"]
    order = np.random.default_rng(seed).permutation(len(regs))
    regs = [regs[i] for i in order]
    return regs, [None if i % 3 else "gene %d;x" % i for i in range(len(regs))]


def bed_file(tmp_path, b, regs, names, name="r.bed"):
    p = str(tmp_path / name)
    with open(p, "w") as fh:
        fh.write("# targets\ntrack name=t\n" + G.bed_lines(b.ref_names, regs, names))
    return p


def want(b, sample, regs, names, value="mean", no_zeros=False, **kw):
    res = G.reduce(oracle_depths(b, **kw), regs)
    return 'track type=bedGraph name="%s"\n' % sample + G.render(b.ref_names, regs, res, value, no_zeros, names)


def depth(paths, extra=(), env=None):
    r = subprocess.run([binary.BIN, "depth", "-b"] + list(paths) + ["-t", "4"] + list(extra), capture_output=True, text=True, timeout=300,
                       env=env or dict(os.environ), stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def refused(argv):
    r = subprocess.run([binary.BIN, "depth"] + argv, capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert r.returncode != 0
    return r.stderr


def test_fixture_bam_every_value(tmp_path):
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    regs, names = regions_for(b)
    bed = bed_file(tmp_path, b, regs, names)
    full = want(b, A[:-4], regs, names)
    assert depth([p], ["--regions", bed]) == full and full.count("\n") == len(regs) + 1 and "\tgene 3;x\t" in full
    for value in G.VALUES:
        assert depth([p], ["--regions", bed, "--bin-value", value]) == want(b, A[:-4], regs, names, value)
        assert depth([p], ["--bin-value", value, "--no-zeros", "--regions", bed]) == want(b, A[:-4], regs, names, value, no_zeros=True)
    assert want(b, A[:-4], regs, names, no_zeros=True) != full
    assert depth([p], ["--regions", bed], env=with_knobs(os.environ, depth_chunk_bases=2048)) == full
    out = str(tmp_path / "a.bed")
    assert depth([p], ["--regions", bed, "-o", out]) == ""
    with open(out) as fh:
        assert fh.read() == full
    assert depth([p], ["--regions", bed, "--min-read-percent-identity", "0.99", "--include-secondary"]) == \
        want(b, A[:-4], regs, names, ff=(True, True, True), fp=dict(min_percent_identity_single=0.99))


def test_sam_on_a_pipe_unsorted(tmp_path):
    b = bamio.read_bam(os.path.join(RAW, A))
    rev = take_bamdata(b, np.arange(len(b.tid))[::-1])      # the last reference's records first
    text = samtext.render(rev, seed=5)
    grouped = take_bamdata(rev, grouped_order(rev.tid, len(rev.ref_lens)))
    regs, names = regions_for(b, 4)
    bed = bed_file(tmp_path, b, regs, names)
    for extra, nz in ((["--unsorted"], False), (["--unsorted", "--no-zeros"], True)):
        r = subprocess.run([binary.BIN, "depth", "-b", "-", "-t", "4", "--regions", bed, "--bin-value", "max"] + extra, input=text, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.decode() == want(grouped, "stdin", regs, names, "max", no_zeros=nz)


def test_two_bams_two_tracks_each_against_its_own_header(tmp_path):
    pa, pb = os.path.join(RAW, A), os.path.join(RAW, A2)
    ba, bb = bamio.read_bam(pa), bamio.read_bam(pb)
    shared = [n for n in ba.ref_names if n in bb.ref_names]
    assert shared and list(ba.ref_names) != list(bb.ref_names)      # the same names at different tids
    lim = {n: min(int(ba.ref_lens[list(ba.ref_names).index(n)]), int(bb.ref_lens[list(bb.ref_names).index(n)])) for n in shared}
    rows = [(n, a, e) for n in reversed(shared) for a, e in ((0, lim[n]), (1, 2), (lim[n] - 1, lim[n]), (0, lim[n]))]
    bed = str(tmp_path / "two.bed")
    with open(bed, "w") as fh:
        fh.write("".join("%s\t%d\t%d\n" % r for r in rows))
    got = depth([pa, pb], ["--regions", bed, "--bin-value", "sum"])
    per = []
    for b, stem in ((ba, A[:-4]), (bb, A2[:-4])):
        regs = [(list(b.ref_names).index(n), a, e) for n, a, e in rows]
        per.append(want(b, stem, regs, None, "sum"))
    assert got == per[0] + per[1] and got.count("track type=bedGraph") == 2


def test_refusals(tmp_path):
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    name, L = b.ref_names[0], int(b.ref_lens[0])
    good = str(tmp_path / "good.bed")
    with open(good, "w") as fh:
        fh.write("%s\t0\t1\n" % name)
    err = refused(["-b", p, "--regions", good, "--bin-size", "100"])
    assert "'--regions' cannot be used with '--bin-size'" in err
    for text, what in (("%s\t0\t1\nno_such_reference\t0\t5\n" % name, "reference 'no_such_reference' is not in"),
                       ("%s\t0\t1\n%s\t0\t%d\n" % (name, name, L + 1), "end %d lies behind the length %d" % (L + 1, L)),
                       ("%s\t0\t1\n%s\t5\t5\n" % (name, name), "start 5 >= end 5")):
        bad = str(tmp_path / "bad.bed")
        with open(bad, "w") as fh:
            fh.write(text)
        err = refused(["-b", p, "--regions", bad])
        assert "%s:2: " % bad in err and what in err
    assert "absent.bed" in refused(["-b", p, "--regions", str(tmp_path / "absent.bed")])
    assert "missing value for --regions" in refused(["-b", p, "--regions"])
    r = subprocess.run([binary.BIN, "contig", "-b", p, "--regions", good], capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert r.returncode != 0 and "unknown argument --regions" in r.stderr
    r = subprocess.run([binary.BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--regions BED" in r.stderr


def test_the_timing_line_counts_the_regions(tmp_path):
    p = os.path.join(RAW, A)
    b = bamio.read_bam(p)
    regs, names = regions_for(b)
    bed = bed_file(tmp_path, b, regs, names)
    r = subprocess.run([binary.BIN, "depth", "-b", p, "--regions", bed, "-o", os.devnull], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, COVERM_CLI_TIMING="1"), stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "depth regions: %d regions computed, fetched and written in" % len(regs) in r.stderr
