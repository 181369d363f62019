"""The BED reader, its resolution against a header and covh_depth_regions_format — the host side of `coverm-amd depth --regions` — through
ctypes, without a device: a good file round-trips (comment, `track` and `browser` lines, CRLF endings, lines with and without a name), every
error names <path>:<line>, and the formatter's bytes equal a Python rendering for every value kind, with no_zeros, for 1 and 4 threads."""
import ctypes as C
import os

import numpy as np
import pytest

from coverm_amd import native
from tests import depth_regions_ref as G


class Header(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("names", C.c_char_p), ("name_off", C.c_void_p), ("target_len", C.c_void_p)]


NAMES = ["chr1", "chr 2 with spaces", "chr10", "empty", "chrM~x"]
LENS = [1000, 50, 2 ** 31 - 1, 0, 16569]


def lib():
    L = native.lib()
    L.covh_last_error.restype = C.c_char_p
    L.covh_bed_read.restype = C.c_void_p
    L.covh_bed_read.argtypes = [C.c_char_p]
    L.covh_bed_free.argtypes = [C.c_void_p]
    L.covh_bed_free.restype = None
    L.covh_bed_count.restype = C.c_uint64
    L.covh_bed_count.argtypes = [C.c_void_p]
    L.covh_bed_line.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.covh_bed_resolve.argtypes = [C.c_void_p, C.POINTER(Header), C.c_void_p]
    L.covh_depth_regions_format.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    return L


class Bed:
    def __init__(self, path):
        self.L = lib()
        self.h = self.L.covh_bed_read(str(path).encode())
        self.error = None if self.h else self.L.covh_last_error().decode()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.h:
            self.L.covh_bed_free(self.h)

    def lines(self):
        out = []
        for i in range(self.L.covh_bed_count(self.h)):
            chrom, name = C.c_void_p(), C.c_void_p()
            cl, nl, a, e, ln = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
            assert self.L.covh_bed_line(self.h, i, C.byref(chrom), C.byref(cl), C.byref(a), C.byref(e), C.byref(name), C.byref(nl), C.byref(ln)) == 0
            out.append((C.string_at(chrom.value, cl.value).decode(), a.value, e.value, C.string_at(name.value, nl.value).decode() if name.value else None, ln.value))
        return out

    def resolve(self, names=NAMES, lens=LENS):
        blob = "".join(names).encode()
        noff = np.concatenate([[0], np.cumsum([len(x.encode()) for x in names])]).astype(np.uint32)
        tl = np.asarray(lens, np.uint64)
        h = Header(len(names), blob, noff.ctypes.data, tl.ctypes.data)
        out = np.zeros(self.L.covh_bed_count(self.h), native.DEPTH_REGION_DTYPE)
        rc = self.L.covh_bed_resolve(self.h, C.byref(h), out.ctypes.data if len(out) else None)
        return rc, out, (self.L.covh_last_error().decode() if rc else None)

    def format(self, tmp_path, res, value, no_zeros, threads, want_rc=0):
        res = np.ascontiguousarray(res, native.DEPTH_BIN_DTYPE)
        path = str(tmp_path / "out.bed")
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
        try:
            rc = self.L.covh_depth_regions_format(self.h, res.ctypes.data if len(res) else None, value if isinstance(value, int) else G.VALUES.index(value), int(no_zeros), threads, fd)
        finally:
            os.close(fd)
        assert rc == want_rc
        with open(path, newline="") as fh:
            return fh.read()


GOOD = ("# a comment\n"
        "track name=targets description=\"x\"\n"
        "browser position chr1:1-100\r\n"
        "chr1\t0\t1000\twhole chr1\n"
        "\n"
        "chr10\t2147483646\t2147483647\r\n"
        "chrM~x\t5\t6\tgene\twith\ttabs\tbehind\r\n"
        "chr 2 with spaces\t49\t50\t\n"
        "\r\n"
        "#chr1\t1\t2\n"
        "chr1\t10\t20\tdup\n"
        "chr1\t10\t20")      # (no newline at the end of the file)
GOOD_LINES = [("chr1", 0, 1000, "whole chr1", 4), ("chr10", 2 ** 31 - 2, 2 ** 31 - 1, None, 6), ("chrM~x", 5, 6, "gene", 7), ("chr 2 with spaces", 49, 50, "", 8),
              ("chr1", 10, 20, "dup", 11), ("chr1", 10, 20, None, 12)]


def write(tmp_path, text, name="r.bed"):
    p = tmp_path / name
    with open(p, "w", newline="") as fh:
        fh.write(text)
    return p


def test_the_mirror_is_sixteen_bytes():
    assert native.DEPTH_REGION_DTYPE.itemsize == 16 and native.DEPTH_REGION_DTYPE.names == ("tid", "start", "end", "reserved")
    assert C.sizeof(native.CovDepthRegionsInfo) == 48 and native.K_DEPTH_REGIONS == 14 and native.K_COUNT == 15


def test_a_good_file_round_trips(tmp_path):
    with Bed(write(tmp_path, GOOD)) as b:
        assert b.error is None and b.lines() == GOOD_LINES
        rc, reg, _ = b.resolve()
        assert rc == 0
        assert reg["tid"].tolist() == [0, 2, 4, 1, 0, 0] and reg["start"].tolist() == [l[1] for l in GOOD_LINES] and reg["end"].tolist() == [l[2] for l in GOOD_LINES]
        assert (reg["reserved"] == 0).all()
    with Bed(write(tmp_path, "# nothing\n\ntrack x\n", "none.bed")) as b:
        assert b.error is None and b.lines() == [] and b.resolve()[0] == 0


@pytest.mark.parametrize("bad, what", [("chr1\t5\n", "found 2 fields"), ("chr1 5 9\n", "found 1 field"), ("chr1\tx5\t9\n", "start 'x5'"), ("chr1\t\t9\n", "start ''"),
                                       ("chr1\t-1\t9\n", "start '-1'"), ("chr1\t5\t9.0\n", "end '9.0'"), ("chr1\t1\t2147483648\n", "end '2147483648'"),
                                       ("chr1\t99999999999999999999\t5\n", "start '99999999999999999999'"), ("chr1\t7\t7\n", "start 7 >= end 7"),
                                       ("chr1\t8\t7\tname\n", "start 8 >= end 7"), ("\t1\t2\n", "reference name is empty")])
def test_syntax_errors_name_path_and_line(tmp_path, bad, what):
    p = write(tmp_path, "# one\nchr1\t0\t5\n\r\n" + bad + "chr1\tnot\treached\n")
    with Bed(p) as b:
        assert b.h is None and b.error.startswith("%s:4: " % p) and what in b.error


def test_a_missing_file_is_an_error(tmp_path):
    with Bed(tmp_path / "absent.bed") as b:
        assert b.h is None and "absent.bed" in b.error


@pytest.mark.parametrize("bad, what", [("chr3\t0\t5\n", "reference 'chr3' is not in"), ("chr\t0\t5\n", "reference 'chr' is not in"), ("CHR1\t0\t5\n", "reference 'CHR1'"),
                                       ("chr1\t0\t1001\n", "end 1001 lies behind the length 1000 of reference 'chr1'"), ("empty\t0\t1\n", "length 0 of reference 'empty'")])
def test_resolution_errors_name_path_and_line(tmp_path, bad, what):
    p = write(tmp_path, "chr1\t0\t1000\n#\n" + bad)
    with Bed(p) as b:
        assert b.error is None
        rc, _, err = b.resolve()
        assert rc == native.ERR_INVALID_ARG and err.startswith("%s:3: " % p) and what in err


@pytest.mark.parametrize("value", G.VALUES)
@pytest.mark.parametrize("no_zeros", [False, True])
def test_the_formatter_equals_python(tmp_path, value, no_zeros):
    with Bed(write(tmp_path, GOOD)) as b:
        regs = [(NAMES.index(c), a, e) for c, a, e, _, _ in GOOD_LINES]
        names = [l[3] for l in GOOD_LINES]
        res = np.zeros(len(regs), native.DEPTH_BIN_DTYPE)
        res["sum"] = [123457, 2 ** 31 - 1, 0, 7, 25, 2 ** 52 + 1]
        res["min"] = [0, 2 ** 31 - 1, 0, 7, 1, 3]
        res["max"] = [900, 2 ** 31 - 1, 0, 7, 4, 2 ** 31 - 1]
        res["covered"] = [999, 1, 0, 1, 10, 10]
        want = G.render(NAMES, regs, res, value, no_zeros, names)
        assert ("gene\t" in want) != no_zeros and "chr 2 with spaces\t49\t50\t\t" in want      # the empty name is a name
        for threads in (1, 4):
            assert b.format(tmp_path, res, value, no_zeros, threads) == want
        assert b.format(tmp_path, res, 5, no_zeros, 1, want_rc=native.ERR_INVALID_ARG) == ""


def test_more_regions_than_a_piece_in_the_files_order(tmp_path):
    """300 000 regions (a piece of the formatter is 2^17): 1 and 4 threads give the same bytes, in the file's order."""
    n = 300_000
    rng = np.random.default_rng(5)
    t = rng.integers(0, 2, n) * 4      # chr1 or chrM~x
    a = rng.integers(0, 900, n)
    e = a + rng.integers(1, 100, n)
    regs = list(zip(t.tolist(), a.tolist(), e.tolist()))
    names = [None if i % 3 else "n%d" % i for i in range(n)]
    res = np.zeros(n, native.DEPTH_BIN_DTYPE)
    res["sum"] = rng.integers(0, 10 ** 6, n)
    res["max"] = rng.integers(0, 3, n)
    with Bed(write(tmp_path, G.bed_lines(NAMES, regs, names), "many.bed")) as b:
        assert b.error is None
        want = G.render(NAMES, regs, res, "mean", False, names)
        for threads in (1, 4):
            assert b.format(tmp_path, res, "mean", False, threads) == want
        assert b.format(tmp_path, res, "sum", True, 4) == G.render(NAMES, regs, res, "sum", True, names)
