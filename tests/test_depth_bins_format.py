"""covh_depth_bins_format — the bedGraph text of `coverm-amd depth --bin-size` — fed bins without a device: the lines equal Python's rendering
for the five value kinds, with and without --no-zeros, with a short last bin, with an empty target between two others, for a target range
inside a larger header, and for 1 and 4 threads over more bins than one piece holds."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd import native
from tests import depth_bins_ref as B
from tests import depth_runs_ref as R


class Header(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("names", C.c_char_p), ("name_off", C.c_void_p), ("target_len", C.c_void_p)]


def fmt(tmp_path, names, lens, tid_lo, n, bin_size, bin_off, bins, value, no_zeros, threads, want_rc=0):
    L = native.lib()
    L.covh_depth_bins_format.argtypes = [C.POINTER(Header), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    blob = "".join(names).encode()
    noff = np.concatenate([[0], np.cumsum([len(x.encode()) for x in names])]).astype(np.uint32)
    tl = np.asarray(lens, np.uint64)
    h = Header(len(names), blob, noff.ctypes.data, tl.ctypes.data)
    bins = np.ascontiguousarray(bins, native.DEPTH_BIN_DTYPE)
    bo = np.ascontiguousarray(bin_off, np.uint64)
    path = str(tmp_path / "out.bedgraph")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
    try:
        rc = L.covh_depth_bins_format(C.byref(h), tid_lo, n, bin_size, bo.ctypes.data, bins.ctypes.data if len(bins) else None, B.VALUES.index(value), int(no_zeros), threads, fd)
    finally:
        os.close(fd)
    assert rc == want_rc
    with open(path) as fh:
        return fh.read()


def test_the_mirror_is_the_reference_layout():
    assert native.DEPTH_BIN_DTYPE == B.BIN_DTYPE


@pytest.mark.parametrize("value", B.VALUES)
@pytest.mark.parametrize("no_zeros", [False, True])
def test_lines_equal_python(tmp_path, value, no_zeros):
    depths = R.shapes()["edge_lengths"] + R.shapes()["all_zero"] + R.shapes()["equal_across_boundaries"]
    names = ["contig_%d~x" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    for bs in (1, 7, 100, 1000):
        off, bins = B.bins_of(depths, bs)
        want = B.bedgraph(names, lens, off, bins, bs, value, no_zeros)
        for threads in (1, 3):
            assert fmt(tmp_path, names, lens, 0, len(names), bs, off, bins, value, no_zeros, threads) == want
        # a chunk in the middle of the header: its offsets count from the chunk's first bin
        lo, hi = 5, 17
        sub = slice(int(off[lo]), int(off[hi]))
        got = fmt(tmp_path, names, lens, lo, hi - lo, bs, off[lo:hi + 1] - off[lo], bins[sub], value, no_zeros, 2)
        assert got == B.bedgraph(names[lo:hi], lens[lo:hi], off[lo:hi + 1] - off[lo], bins[sub], bs, value, no_zeros)


def test_short_last_bin_and_an_empty_target_between_two(tmp_path):
    depths = [np.asarray([1, 2, 3, 4, 5, 6, 7], np.int32), np.zeros(0, np.int32), np.asarray([0, 0, 0, 9], np.int32)]
    off, bins = B.bins_of(depths, 3)
    assert off.tolist() == [0, 3, 3, 5]
    got = fmt(tmp_path, ["a", "gap", "b"], [7, 0, 4], 0, 3, 3, off, bins, "mean", False, 1)
    assert got == "a\t0\t3\t2.000\na\t3\t6\t5.000\na\t6\t7\t7.000\nb\t0\t3\t0.000\nb\t3\t4\t9.000\n"
    assert fmt(tmp_path, ["a", "gap", "b"], [7, 0, 4], 0, 3, 3, off, bins, "sum", True, 1) == "a\t0\t3\t6\na\t3\t6\t15\na\t6\t7\t7\nb\t3\t4\t9\n"
    assert fmt(tmp_path, ["a", "gap", "b"], [7, 0, 4], 0, 3, 3, off, bins, "min", False, 1).split("\n")[3] == "b\t0\t3\t0"
    assert fmt(tmp_path, ["a", "gap", "b"], [7, 0, 4], 0, 3, 3, off, bins, "covered", False, 4).endswith("b\t0\t3\t0\nb\t3\t4\t1\n")


def test_the_mean_is_the_quotient_of_the_two_integers(tmp_path):
    """Sums and lengths whose quotient falls on or next to a rounding edge of three decimals: C's %.3f of the double equals Python's."""
    sums = [1, 2, 5, 7, 1001, 2 ** 31 - 1, 3 * (2 ** 31 - 1), 12345678901, 2 ** 52 + 1]
    for bs in (3, 7, 16, 2000, 3000):
        bins = np.zeros(len(sums), native.DEPTH_BIN_DTYPE)
        bins["sum"] = sums
        bins["max"] = 1
        lens = [bs] * len(sums)
        off = np.arange(len(sums) + 1, dtype=np.uint64)
        names = ["t%d" % i for i in range(len(sums))]
        got = fmt(tmp_path, names, lens, 0, len(sums), bs, off, bins, "mean", False, 1)
        assert got == "".join("t%d\t0\t%d\t%s\n" % (i, bs, "%.3f" % (s / bs)) for i, s in enumerate(sums))


def test_more_bins_than_a_piece_in_order(tmp_path):
    """300 000 bins (a piece is 2^17): the pieces formatted side by side come out in order, cut anywhere inside a target or between empty ones."""
    depths = [(np.arange(L) % 3).astype(np.int32) for L in (300_000, 0, 0, 262_144, 1, 37_853)] + [np.zeros(0, np.int32)]
    names = ["t%d" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    off, bins = B.bins_of(depths, 2)
    assert len(bins) == 300_000
    want = B.bedgraph(names, lens, off, bins, 2)
    for threads in (1, 4):
        assert fmt(tmp_path, names, lens, 0, len(names), 2, off, bins, "mean", False, threads) == want
    assert fmt(tmp_path, names, lens, 0, len(names), 2, off, bins, "max", True, 4) == B.bedgraph(names, lens, off, bins, 2, "max", True)


def test_no_bins_and_refusals(tmp_path):
    none = np.zeros(0, native.DEPTH_BIN_DTYPE)
    assert fmt(tmp_path, ["a", "b"], [0, 0], 0, 2, 10, [0, 0, 0], none, "mean", False, 2) == ""
    assert fmt(tmp_path, ["a", "b"], [0, 0], 0, 2, 0, [0, 0, 0], none, "mean", False, 2, want_rc=native.ERR_INVALID_ARG) == ""
    assert fmt(tmp_path, ["a", "b"], [0, 0], 1, 2, 10, [0, 0, 0], none, "mean", False, 2, want_rc=native.ERR_INVALID_ARG) == ""
