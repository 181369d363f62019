"""csrc/bgzf_walk_core.h (the BGZF header test, the per-chunk hop and the serial header chain of the device ingest's host driver) against
one pass over the whole byte string, and against the code the driver carried before the header existed, frozen in
tests/c/bgzf_walk_host.cpp: files made here with zlib are handed over piece by piece, as the driver's reader thread hands them over.
The program form of the same file walks files of stored blocks built with -fsanitize=address,undefined."""
import ctypes as C
import itertools
import os
import random
import struct
import subprocess
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "bgzf_walk_host.cpp")
OK, NOT_BGZF, EXTRA_SUBFIELDS, MALFORMED, ISIZE_ABOVE_64K, TRUNCATED = range(6)
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
PIECES = range(64, 201)
CHUNKS = (32, 47, 64)


class Block(C.Structure):      # cov_bgzf_block
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("in_len", C.c_uint32), ("isize", C.c_uint32), ("crc", C.c_uint32), ("pad", C.c_uint32)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bgzfw") / "bgzf_walk_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.bgzfw_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(Block), C.c_uint64] + [C.POINTER(C.c_uint64)] * 4
    L.bgzfw_classify.argtypes = [C.c_char_p, C.c_int]
    L.bgzfw_frozen_find_test.argtypes = [C.c_char_p]
    return L


def block(payload, level=6, crc=None, isize=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize))


def make_file(n_blocks, lo, hi, seed, level=6):
    """-> (bytes, offsets of the block headers, the end-of-file block's included)"""
    rng = random.Random(seed)
    raw, starts = b"", []
    for _ in range(n_blocks):
        starts.append(len(raw))
        raw += block(rng.randbytes(rng.randint(lo, hi)), level)
    starts.append(len(raw))
    return raw + EOF_BLOCK, starts


def single_pass(raw):
    table, q, out = [], 0, 0
    while q < len(raw):
        bs = int.from_bytes(raw[q + 16:q + 18], "little") + 1
        crc, isize = struct.unpack("<II", raw[q + bs - 8:q + bs])
        table.append((q + 18, bs - 26, crc, isize, out))
        out += isize
        q += bs
    assert q == len(raw)
    return table


def walk(host, raw, piece, chunk, which=0, cap=4096):
    out = (Block * cap)()
    n, nxt, pre, taken = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    st = host.bgzfw_walk(raw, len(raw), piece, chunk, which, out, cap, C.byref(n), C.byref(nxt), C.byref(pre), C.byref(taken))
    assert n.value <= cap
    return st, nxt.value, [(b.in_off, b.in_len, b.crc, b.isize, b.out_off) for b in out[:n.value]], pre.value, taken.value


def both(host, raw, piece, chunk):
    """The walk of bgzf_walk_core.h, which must equal the frozen code's in every respect -> (status, next_blk, table, lists taken over)"""
    a, b = walk(host, raw, piece, chunk, 0), walk(host, raw, piece, chunk, 1)
    assert a[:4] == b[:4], (piece, chunk, a[:2], b[:2])
    return a[0], a[1], a[2], b[4]


def test_every_split_of_a_header_and_of_a_trailer(host):
    """Blocks of 40-90 payload bytes, pieces of 64-200 bytes, chunks of 32-64 bytes: a piece boundary falls behind each of the first 1..17
    bytes of some header and behind each of the first 1..7 bytes of some trailer (counted from the offsets, all must occur), and the table
    is the single pass's every time.  Such a block is at most 90 + 5 + 26 bytes long, so with pieces of 64 bytes or more it ends at most
    two pieces after the one its header began in; a second file of 200-300 payload bytes supplies the blocks completed three and more
    pieces after their header."""
    hdr_split, trl_split, later = [0] * 18, [0] * 8, 0
    for raw, starts in (make_file(40, 40, 90, 5), make_file(12, 200, 300, 6)):
        want = single_pass(raw)
        ends = starts[1:] + [len(raw)]
        for piece in PIECES:
            for h, e in zip(starts, ends):
                for s in range(1, 18):
                    hdr_split[s] += (h + s) % piece == 0
                for s in range(1, 8):
                    trl_split[s] += (e - 8 + s) % piece == 0
                later += (e - 1) // piece - h // piece >= 3
            for chunk in CHUNKS:
                st, nxt, table, _ = both(host, raw, piece, chunk)
                assert (st, nxt) == (OK, len(raw)) and table == want, (piece, chunk)
    assert all(hdr_split[1:]) and all(trl_split[1:]) and later, (hdr_split, trl_split, later)


def test_chunks_that_hold_whole_blocks_hand_their_lists_over(host):
    """Chunks larger than the blocks: the chain takes the per-chunk lists over where it arrives at their first header, and hops the blocks
    that straddle chunks and pieces itself."""
    raw, _ = make_file(60, 40, 90, 7)
    want = single_pass(raw)
    for piece, chunk in itertools.product((500, 777, 1024), (128, 200, 256)):
        st, nxt, table, taken = both(host, raw, piece, chunk)
        assert (st, nxt) == (OK, len(raw)) and table == want and taken > 0, (piece, chunk, taken)


def test_a_header_inside_a_stored_block_is_not_a_block(host):
    """A stored (level 0) block whose payload holds a complete header and a complete block (two end-of-file blocks back to back, so that
    find_block_start's look at the following header would pass as well), with chunks that start inside that payload: the per-chunk hop
    finds the fake and lists it, the chain never arrives there."""
    rng = random.Random(11)
    fake = block(rng.randbytes(20), 0) + EOF_BLOCK + EOF_BLOCK
    raw = block(rng.randbytes(50)) + block(rng.randbytes(37) + fake + rng.randbytes(9), 0) + block(rng.randbytes(60)) + EOF_BLOCK
    want = single_pass(raw)
    assert len(want) == 4
    listed = 0
    for piece, chunk in itertools.product(PIECES, CHUNKS):
        st, nxt, table, _ = both(host, raw, piece, chunk)
        assert (st, nxt) == (OK, len(raw)) and table == want, (piece, chunk)
        listed += walk(host, raw, piece, chunk)[3] >= 2
    assert listed      # the hop did list the blocks inside the payload: of the file's own blocks only the last fits into such a chunk


def _irregular(kind):
    """-> (bytes, status, offset of the block the walk stops at; the table when the file is taken after all)"""
    raw, starts = make_file(30, 40, 90, 13)
    k = 17
    at, end = starts[k], starts[k + 1]
    if kind == "flg_extra_bit":       # FLG = FEXTRA | FTEXT with XLEN == 6: the chain takes it
        raw = raw[:at + 3] + b"\x05" + raw[at + 4:]
        return raw, OK, len(raw), single_pass(raw)
    if kind == "second_subfield":     # XLEN 6 -> 10, BSIZE + 4 (a block every BGZF reader accepts)
        blk = raw[at:at + 10] + struct.pack("<H", 10) + b"BC\x02\0" + struct.pack("<H", end - at + 4 - 1) + b"XX\0\0" + raw[at + 18:end]
        return raw[:at] + blk + raw[end:], EXTRA_SUBFIELDS, at, None
    if kind == "bsize_below_26":
        return raw[:at + 16] + struct.pack("<H", 24) + raw[at + 18:], MALFORMED, at, None
    if kind == "isize_above_64k":
        return raw[:end - 4] + struct.pack("<I", 65537) + raw[end:], ISIZE_ABOVE_64K, at, None
    if kind == "last_block_cut_short":
        return raw[:-5], TRUNCATED, starts[-1], None
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["flg_extra_bit", "second_subfield", "bsize_below_26", "isize_above_64k", "last_block_cut_short"])
def test_irregular_files_end_where_they_ended_before(host, kind):
    """Status and point of failure are the frozen loop's (asserted inside both()), for every piece size and with chunks below and above
    the block size, and they are the ones written down here."""
    raw, status, stop, table = _irregular(kind)
    for piece, chunk in itertools.product(PIECES, CHUNKS + (256,)):
        st, nxt, got, _ = both(host, raw, piece, chunk)
        assert (st, nxt) == (status, stop), (piece, chunk)
        if table is not None:
            assert got == table


def test_end_of_file_block_alone_and_empty_input(host):
    for piece, chunk in ((64, 32), (200, 64), (64, 64), (100, 47)):
        assert both(host, EOF_BLOCK, piece, chunk)[:3] == (OK, 28, [(18, 2, 0, 0, 0)])
        assert both(host, b"", piece, chunk)[:3] == (OK, 0, [])


def test_header_test_equals_the_one_of_find_block_start(host):
    """Every combination of the nine fields of an ordinary header left alone or perturbed (2^9, with two ways to perturb each field): the
    strict form says ORDINARY exactly where find_block_start's test passed; the outcomes name the first field that fails, in the order
    signature, subfield, BSIZE; the chain's form differs from the strict one in FLG alone."""
    good = bytearray(EOF_BLOCK[:16] + struct.pack("<H", 99))
    fields = [(0, 1), (1, 1), (2, 1), (3, 1), (10, 2), (12, 1), (13, 1), (14, 2), (16, 2)]       # ID1 ID2 CM FLG XLEN SI1 SI2 SLEN BSIZE
    variants = [[b"\x1e", b"\x8a", b"\x09", b"\x05", b"\x0a\0", b"C", b"B", b"\x03\0", b"\x18\0"],
                [b"\0", b"\0", b"\0", b"\0", b"\x06\x01", b"\0", b"\0", b"\x02\x01", b"\0\0"]]
    n = 0
    for var in variants:
        for mask in range(1 << len(fields)):
            h = bytearray(good)
            for i, (off, ln) in enumerate(fields):
                if mask >> i & 1:
                    h[off:off + ln] = var[i]
            strict, loose, old = host.bgzfw_classify(bytes(h), 0), host.bgzfw_classify(bytes(h), 1), host.bgzfw_frozen_find_test(bytes(h))
            assert (strict == 0) == bool(old), (mask, var)
            want = 1 if mask & 0b1111 else 2 if mask & 0b11110000 else 3 if mask >> 8 else 0
            assert strict == want, (mask, strict)
            want = 1 if mask & 0b0111 or not h[3] & 4 else 2 if mask & 0b11110000 else 3 if mask >> 8 else 0
            assert loose == want, (mask, loose)
            n += 1
    assert n == 2 * 512


def test_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bgzf_walk_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.strip() == "%d cases, 0 bad" % (2 * 6 * 137 * 3 + 9 + 2)
