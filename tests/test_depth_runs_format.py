"""covh_depth_runs_format — the bedGraph text of `coverm-amd depth` — fed runs without a device: the lines equal Python's rendering, with and
without --no-zeros, for a target range inside a larger header, for every thread count, and over more runs than one piece holds."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd import native
from tests import depth_runs_ref as R


class Header(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("names", C.c_char_p), ("name_off", C.c_void_p), ("target_len", C.c_void_p)]


def fmt(tmp_path, names, lens, tid_lo, n, run_off, start, depth, no_zeros, threads):
    L = native.lib()
    L.covh_depth_runs_format.argtypes = [C.POINTER(Header), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    blob = "".join(names).encode()
    noff = np.concatenate([[0], np.cumsum([len(x.encode()) for x in names])]).astype(np.uint32)
    tl = np.asarray(lens, np.uint64)
    h = Header(len(names), blob, noff.ctypes.data, tl.ctypes.data)
    runs = np.zeros(len(start), native.DEPTH_RUN_DTYPE)
    runs["start"], runs["depth"] = start, depth
    ro = np.ascontiguousarray(run_off, np.uint64)
    path = str(tmp_path / "out.bedgraph")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
    try:
        rc = L.covh_depth_runs_format(C.byref(h), tid_lo, n, ro.ctypes.data, runs.ctypes.data if len(runs) else None, int(no_zeros), threads, fd)
    finally:
        os.close(fd)
    assert rc == 0
    with open(path) as fh:
        return fh.read()


@pytest.mark.parametrize("no_zeros", [False, True])
@pytest.mark.parametrize("threads", [1, 3])
def test_lines_equal_python(tmp_path, no_zeros, threads):
    depths = R.shapes()["edge_lengths"] + R.shapes()["all_zero"] + R.shapes()["equal_across_boundaries"]
    names = ["contig_%d~x" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    off, start, depth = R.runs_of(depths)
    want = R.bedgraph(names, lens, off, start, depth, no_zeros)
    assert fmt(tmp_path, names, lens, 0, len(names), off, start, depth, no_zeros, threads) == want
    assert want.startswith("contig_1~x\t0\t1\t") or no_zeros
    # a chunk in the middle of the header: its offsets count from the chunk's first run
    lo, hi = 5, 17
    sub = slice(int(off[lo]), int(off[hi]))
    got = fmt(tmp_path, names, lens, lo, hi - lo, off[lo:hi + 1] - off[lo], start[sub], depth[sub], no_zeros, threads)
    assert got == R.bedgraph(names[lo:hi], lens[lo:hi], off[lo:hi + 1] - off[lo], start[sub], depth[sub], no_zeros)


def test_more_runs_than_a_piece_in_order(tmp_path):
    """400 000 runs (a piece is 2^17): the pieces formatted side by side come out in order, cut anywhere inside a target or between empty ones."""
    rng = np.random.default_rng(3)
    depths = [(np.arange(L) % 3).astype(np.int32) for L in (150_000, 0, 0, 131_072, 1, 118_927)] + [np.zeros(0, np.int32)]
    names = ["t%d" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    off, start, depth = R.runs_of(depths)
    assert len(start) == 400_000
    want = R.bedgraph(names, lens, off, start, depth)
    for threads in (1, 2, 5):
        assert fmt(tmp_path, names, lens, 0, len(names), off, start, depth, False, threads) == want
    assert fmt(tmp_path, names, lens, 0, len(names), off, start, depth, True, 4) == R.bedgraph(names, lens, off, start, depth, True)
    del rng


def test_no_runs(tmp_path):
    assert fmt(tmp_path, ["a", "b"], [0, 0], 0, 2, [0, 0, 0], [], [], False, 2) == ""
