"""The host side of `coverm-amd depth --quantize / --thresholds` through ctypes, without a device: the spec parsers, and the formatters
covh_depth_class_runs_format, covh_depth_regions_counts_format and covh_depth_bins_counts_format against the renderers of
tests/depth_classes_ref.py, byte for byte, for every thread count."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd import native
from tests import depth_classes_ref as K
from tests import depth_regions_ref as G
from tests import depth_runs_ref as R
from tests.test_depth_runs_format import Header

ERR_INVALID_ARG = native.ERR_INVALID_ARG


def lib():
    L = native.lib()
    L.covh_last_error.restype = C.c_char_p
    L.covh_depth_quantize_parse.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    L.covh_depth_thresholds_parse.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.covh_depth_class_runs_format.argtypes = [C.POINTER(Header), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int]
    L.covh_depth_regions_counts_format.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int]
    L.covh_depth_bins_counts_format.argtypes = [C.POINTER(Header), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int]
    L.covh_bed_read.restype = C.c_void_p
    L.covh_bed_read.argtypes = [C.c_char_p]
    L.covh_bed_free.argtypes = [C.c_void_p]
    L.covh_bed_free.restype = None
    return L


def parse(spec):
    L = lib()
    cuts, n, oe = np.full(16, -7, np.int32), C.c_uint32(99), C.c_int(-1)
    rc = L.covh_depth_quantize_parse(spec.encode(), cuts.ctypes.data, C.byref(n), C.byref(oe))
    return (rc, tuple(int(c) for c in cuts[:n.value]), bool(oe.value)) if rc == 0 else (rc, L.covh_last_error().decode(), None)


@pytest.mark.parametrize("spec,cuts,open_end", [("0:1:", (0, 1), True), (":1:5", (0, 1, 5), False), ("1:5:", (1, 5), True), (":", (0,), True),
                                                ("0:1:5:150:", (0, 1, 5, 150), True), ("5:", (5,), True), ("0:2147483647", (0, 2147483647), False),
                                                (":".join(map(str, range(16))) + ":", tuple(range(16)), True)])
def test_good_specs(spec, cuts, open_end):
    assert parse(spec) == (0, cuts, open_end)
    assert K.parse_quantize(spec) == (cuts, open_end)


@pytest.mark.parametrize("spec", ["5", "1:1", "5:1", "a:b", "1::2", "-1:2", ":".join(map(str, range(17))), "0:2147483648", "", "1: 2", "1:2::", "::", "0x1:2", "+1:2"])
def test_bad_specs(spec):
    rc, msg, _ = parse(spec)
    assert rc == ERR_INVALID_ARG and "covh_depth_quantize_parse" in msg and ("'%s'" % spec) in msg
    with pytest.raises(ValueError):
        K.parse_quantize(spec)


def test_thresholds_list():
    L = lib()
    thr, n = np.zeros(16, np.int32), C.c_uint32(0)
    assert L.covh_depth_thresholds_parse(b"1,10,30", thr.ctypes.data, C.byref(n)) == 0 and thr[:n.value].tolist() == [1, 10, 30]
    assert L.covh_depth_thresholds_parse(b"0", thr.ctypes.data, C.byref(n)) == 0 and thr[:n.value].tolist() == [0]
    for bad, what in ((b"", "empty"), (b"1,,2", "empty"), (b"3,2", "value 1"), (b"1,1", "value 1"), (b"1;2", "not a decimal"), (b"-1", "not a decimal"),
                      (b"2147483648", "not a decimal"), (",".join(map(str, range(17))).encode(), "more than 16"), (b"1,2,", "empty")):
        assert L.covh_depth_thresholds_parse(bad, thr.ctypes.data, C.byref(n)) == ERR_INVALID_ARG, bad
        assert what in L.covh_last_error().decode(), (bad, L.covh_last_error())


def header(names, lens):
    blob = "".join(names).encode()
    noff = np.concatenate([[0], np.cumsum([len(x.encode()) for x in names])]).astype(np.uint32)
    tl = np.asarray(lens, np.uint64)
    return Header(len(names), blob, noff.ctypes.data, tl.ctypes.data), (blob, noff, tl)


def to_file(tmp_path, call):
    path = str(tmp_path / "out.txt")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
    try:
        rc = call(fd)
    finally:
        os.close(fd)
    assert rc == 0, lib().covh_last_error()
    with open(path) as fh:
        return fh.read()


def fmt_runs(tmp_path, names, lens, tid_lo, n, run_off, start, cls, cuts, open_end, threads):
    L = lib()
    h, keep = header(names, lens)
    runs = np.zeros(len(start), native.DEPTH_RUN_DTYPE)
    runs["start"], runs["depth"] = start, cls
    ro = np.ascontiguousarray(run_off, np.uint64)
    c = np.asarray(cuts, np.int32)
    return to_file(tmp_path, lambda fd: L.covh_depth_class_runs_format(C.byref(h), tid_lo, n, ro.ctypes.data, runs.ctypes.data if len(runs) else None, c.ctypes.data, len(c),
                                                                      int(open_end), threads, fd))


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("spec", ["0:1:5:", "1:2:4:16", "1:2:4:16:", ":", "3:", "0:1"])
def test_class_lines_equal_python(tmp_path, spec, threads):
    cuts, open_end = K.parse_quantize(spec)
    depths = K.shapes()["edge_lengths"] + K.shapes()["runs_cross_boundaries"] + K.shapes()["alternating_in_class"] + K.shapes()["all_zero"]
    names = ["contig_%d~x" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    off, start, cls = K.class_runs_of(depths, cuts)
    want = K.render_classes(names, lens, off, start, cls, cuts, open_end)
    assert fmt_runs(tmp_path, names, lens, 0, len(names), off, start, cls, cuts, open_end, threads) == want
    lo, hi = 5, 14      # a chunk in the middle of the header: its offsets count from the chunk's first run
    sub = slice(int(off[lo]), int(off[hi]))
    got = fmt_runs(tmp_path, names, lens, lo, hi - lo, off[lo:hi + 1] - off[lo], start[sub], cls[sub], cuts, open_end, threads)
    assert got == K.render_classes(names[lo:hi], lens[lo:hi], off[lo:hi + 1] - off[lo], start[sub], cls[sub], cuts, open_end)


def test_the_printing_rules(tmp_path):
    """A closed spec prints neither class 0 nor class n; an open one prints class n as lo:inf; `end` comes from the next run, printed or not."""
    depth = [np.asarray([0, 0, 1, 1, 7, 7, 7, 2, 0, 9], np.int32), np.asarray([3], np.int32)]
    names, lens = ["a", "b"], [10, 1]
    off, start, cls = K.class_runs_of(depth, (1, 5))
    assert cls.tolist() == [0, 1, 2, 1, 0, 2, 1]
    closed = fmt_runs(tmp_path, names, lens, 0, 2, off, start, cls, (1, 5), False, 2)
    assert closed == "a\t2\t4\t1:5\na\t7\t8\t1:5\nb\t0\t1\t1:5\n"      # 2..4 ends where the unprinted class-2 run starts
    opened = fmt_runs(tmp_path, names, lens, 0, 2, off, start, cls, (1, 5), True, 2)
    assert opened == "a\t2\t4\t1:5\na\t4\t7\t5:inf\na\t7\t8\t1:5\na\t9\t10\t5:inf\nb\t0\t1\t1:5\n"
    assert "0:" not in closed and fmt_runs(tmp_path, names, lens, 0, 2, [0, 0, 0], [], [], (1, 5), True, 1) == ""


def test_more_class_runs_than_a_piece_in_order(tmp_path):
    depths = [(np.arange(L) % 3).astype(np.int32) for L in (150_000, 0, 131_072, 1)]
    names, lens = ["t%d" % i for i in range(4)], [len(d) for d in depths]
    off, start, cls = K.class_runs_of(depths, (0, 1, 2))
    assert len(start) > 2 * (1 << 17)
    want = K.render_classes(names, lens, off, start, cls, (0, 1, 2), True)
    for threads in (1, 4):
        assert fmt_runs(tmp_path, names, lens, 0, 4, off, start, cls, (0, 1, 2), True, threads) == want


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("no_zeros", [False, True])
def test_region_count_lines_equal_python(tmp_path, threads, no_zeros):
    L = lib()
    depths = R.shapes()["runs_cross_boundaries"] + R.shapes()["all_zero"]
    names = ["c%d" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    sets = G.region_sets(lens)
    regs = sets["edges"] + sets["random"] + sets["overlap"]
    rnames = [None if i % 3 == 0 else "gene %d" % i for i in range(len(regs))]      # the name column: only where the line had one
    bed = tmp_path / "r.bed"
    bed.write_text(G.bed_lines(names, regs, rnames))
    res = G.reduce(depths, regs)
    assert (res["max"] == 0).any() and (res["max"] > 0).any()
    thr = K.MIXED
    cnt = np.ascontiguousarray(K.counts(depths, regs, thr))
    b = L.covh_bed_read(str(bed).encode())
    assert b
    try:
        got = to_file(tmp_path, lambda fd: L.covh_depth_regions_counts_format(b, res.ctypes.data, cnt.ctypes.data, len(thr), int(no_zeros), threads, fd))
    finally:
        L.covh_bed_free(b)
    want = K.render_counts(names, regs, cnt, res["max"], no_zeros, rnames)
    assert got == want and ("\tgene 2\t" in got) and got.count("\n") == (int((res["max"] > 0).sum()) if no_zeros else len(regs))


@pytest.mark.parametrize("threads", [1, 4])
def test_window_count_lines_equal_python(tmp_path, threads):
    L = lib()
    depths = R.shapes()["edge_lengths"] + R.shapes()["all_zero"]
    names = ["w%d" % i for i in range(len(depths))]
    lens = [len(d) for d in depths]
    for bs in (1, 100, 5000):
        regs = [(t, j * bs, min((j + 1) * bs, n)) for t, n in enumerate(lens) for j in range((n + bs - 1) // bs)]
        boff = np.concatenate([[0], np.cumsum([(n + bs - 1) // bs for n in lens])]).astype(np.uint64)
        res = G.reduce(depths, regs)
        cnt = np.ascontiguousarray(K.counts(depths, regs, (1, 2)))
        h, keep = header(names, lens)
        for no_zeros in (False, True):
            got = to_file(tmp_path, lambda fd: L.covh_depth_bins_counts_format(C.byref(h), 0, len(names), bs, boff.ctypes.data, res.ctypes.data, cnt.ctypes.data, 2, int(no_zeros),
                                                                               threads, fd))
            assert got == K.render_counts(names, regs, cnt, res["max"], no_zeros), (bs, no_zeros)
