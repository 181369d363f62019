"""csrc/ingest_plan_core.h (the device ingest's driver as arithmetic: which bytes of a fed piece go to which round's compressed buffer, the
sizes of a window's buffers, the store's first-window scale, the verdict of a finished ingest, the rings the rounds turn in) against the
loop of cov_ingest_feed and the expressions of launch_round_, ingest_drain_ and ingest_end_ as they stood before, frozen in
tests/c/ingest_plan_host.cpp, and against properties stated here that do not depend on the frozen copy.
The program form of the same file walks the same grids built with -fsanitize=address,undefined."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "ingest_plan_host.cpp")

SIZES = {0: "90 B", 1: "700 B", 2: "0xFF00 B", 3: "mixed"}
PIECES = (64 * 1024, 200 * 1024, 0)      # 0: the whole file in one piece
ROUND_BLOCKS = (64, 128, 4096)
CORRUPT = {1: "out of order", 2: "payload beyond the piece", 3: "isize > 64 KiB", 4: "payload > 64 KiB", 5: "not contiguous when inflated"}
BROKEN = {1: "steps differ from the frozen loop", 2: "one of the two rejected, the other did not", 4: "a byte not copied exactly once", 8: "a copy outside its round's buffer",
          16: "a block's bytes in another round's buffer", 32: "launches do not add up to the blocks fed", 64: "a round longer than round_blocks",
          128: "steps out of order", 256: "state differs from the frozen loop", 512: "a bad table accepted"}
KEY_END = 0x80000000


def ccap_of(round_blocks, bytes_rule):
    return 256 * 1024 if bytes_rule else round_blocks * 65536 * 2      # the rounds close on bytes / on the block count


def feed_grid():
    for sizes, piece, rb, bytes_rule, mid in itertools.product(SIZES, PIECES, ROUND_BLOCKS, (0, 1), (0, 1)):
        yield sizes, piece, rb, ccap_of(rb, bytes_rule), mid


def why(bits):
    return [t for b, t in BROKEN.items() if bits & b]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ingplan") / "ingest_plan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    L.ingplan_feed_case.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.ingplan_feed_case.restype = C.c_uint32
    L.ingplan_geometry_differs.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    for f in (L.ingplan_scale, L.ingplan_scale_frozen):
        f.argtypes = [C.c_uint64] * 3
        f.restype = C.c_double
    L.ingplan_end.argtypes = [C.c_uint32] * 3 + [C.c_longlong] * 2 + [C.c_int] * 2 + [C.c_uint64] * 2 + [C.c_int] * 2
    L.ingplan_end.restype = C.c_uint32
    L.ingplan_is_span.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int]
    L.ingplan_slot.argtypes = [C.c_int, C.c_uint32]
    L.ingplan_slot.restype = C.c_uint32
    L.ingplan_reused.argtypes = [C.c_int, C.c_uint32]
    L.ingplan_extracted_before_launch.argtypes = [C.c_uint32]
    L.ingplan_extracted_before_launch.restype = C.c_longlong
    return L


def test_feed_plan_equals_the_frozen_loop_and_keeps_its_properties(host):
    """Every case: the same steps and the same state as the frozen loop, and — from the planner's steps alone — every fed byte copied exactly
    once, every copy inside its round's buffer (b - origin <= ccap + 2 * 65536 + 256), a block's bytes in the buffer of the round whose
    launch contains the block, the launches' blocks adding up to the blocks fed, no round longer than round_blocks."""
    out = (C.c_uint64 * 6)()
    n = straddles = on_count = on_bytes = 0
    for sizes, piece, rb, ccap, mid in feed_grid():
        bits = host.ingplan_feed_case(sizes, piece, rb, ccap, mid, 0, out)
        assert bits == 0, (SIZES[sizes], piece, rb, ccap, mid, why(bits))
        steps, launches, blocks, fed, cut, rejected = list(out)
        n_blocks = 3 * rb + 17 - (rb // 2 + 3 if mid else 0)
        assert (blocks, rejected) == (n_blocks, 0) and launches >= 2 and steps > launches
        straddles += cut
        closes_on_count = launches == (n_blocks - 1) // rb      # every launched round was full (the open one holds the rest)
        on_count += closes_on_count
        on_bytes += not closes_on_count
        n += 1
    assert n == 4 * 3 * 3 * 2 * 2
    assert straddles > 100          # pieces did end inside the block that opens the next round
    assert on_count and on_bytes    # both closing rules fired on the grid


def test_feed_plan_rejects_what_the_frozen_loop_rejects(host):
    out = (C.c_uint64 * 6)()
    n = 0
    for (sizes, piece, rb, ccap, mid), corrupt in itertools.product(feed_grid(), CORRUPT):
        if rb == 4096 or mid:
            continue      # (the rejections need no large case)
        bits = host.ingplan_feed_case(sizes, piece, rb, ccap, mid, corrupt, out)
        assert bits == 0 and out[5] == 1, (SIZES[sizes], piece, rb, ccap, CORRUPT[corrupt], why(bits))
        assert out[2] <= (3 * rb + 17) // 2 + 1      # nothing behind the offending entry was accepted
        n += 1
    assert n == 4 * 3 * 2 * 2 * 5


SPANS = ((0, 1000), (0, 3 << 20), (0, 200 << 20), (5 << 30, 25 << 30), (7, 7))      # small files, a 200 MB-class file, a 20 GB-class span, an empty span


def test_window_geometry_equals_the_frozen_expressions(host):
    out = (C.c_uint64 * 6)()
    for (lo, hi), rb, carry in itertools.product(SPANS + ((9, 3),), (64, 4096, 61440), (65536, 16 << 20)):
        for n in (0, 1, rb - 1, rb, rb + 1):
            assert host.ingplan_geometry_differs(lo, hi, n, rb, carry, 2048, 16384, out) == 0, (lo, hi, rb, carry, n)
            est, full, win_bytes, seg_cap, scratch, tok = list(out)
            # sized for the blocks of this round at least, and for a full round unless the file is too small to have one
            assert full >= n and full <= max(n, rb) and (full == max(n, rb) or full == max(n, est))
            assert win_bytes == carry + full * 65536 + 64 and seg_cap * 32768 >= win_bytes > (seg_cap - 1) * 32768
            assert scratch >= full * 2048 and tok == full * 16384


def test_first_window_scale_equals_the_frozen_expression(host):
    seen_zero = seen_scaled = 0
    for lo, hi in SPANS:
        for comp_end in (0, 1, lo, lo + 70000, max(hi - 65536, 0), max(hi - 65537, 0), hi):
            got = host.ingplan_scale(comp_end, lo, hi)
            assert got == host.ingplan_scale_frozen(comp_end, lo, hi), (lo, hi, comp_end)
            seen_zero += got == 0
            seen_scaled += got > 1.1
    assert seen_zero and seen_scaled


def test_header_left(host):
    """Window 0 is told the whole header, as ever; a window behind the header's end nothing; one the header runs into, the rest of it."""
    host.ingplan_header_left.argtypes = [C.c_uint64] * 2
    host.ingplan_header_left.restype = C.c_uint64
    for first_record in (0, 40, 716_800, 4_974_980):
        assert host.ingplan_header_left(first_record, 0) == first_record
        for out_off0 in (1, 716_800, 4_974_979, 4_974_980, 1 << 40):
            assert host.ingplan_header_left(first_record, out_off0) == max(first_record - out_off0, 0)


def test_verdict_equals_the_frozen_if_chain(host):
    """Every combination of the seven status bits, both failure counters zero and not, whole file and span (each of the four ways to be one),
    open end, the tail key absent / inside / beyond the span, the previous key absent / inside / beyond, spilled or not."""
    tails = (2 ** 64 - 1, 50, KEY_END)
    prevs = (99, 1 << 63 | 50, 1 << 63 | KEY_END)
    n = 0
    texts = set()
    for fail in range(128):
        for inf, ext, key_lo, key_hi, sf, oe, tail, prev, spilled in itertools.product((0, 5), (0, 7), (0, 5), (KEY_END, 100), (0, 1), (0, 1), tails, prevs, (0, 1)):
            args = (fail, inf, ext, key_lo, key_hi, sf, oe, tail, prev, spilled)
            got = host.ingplan_end(*args, 0)
            assert got == host.ingplan_end(*args, 1), args
            texts.add(got)
            n += 1
    assert n == 128 * 2 * 2 * 16 * 3 * 3 * 2
    assert {t & 0xff for t in texts} == set(range(13))         # every outcome occurs
    assert {t >> 8 for t in texts} == {0, 1, 2, 3, 4}          # and every ending
    for key_lo, key_hi, sf, oe in itertools.product((0, 1), (KEY_END, KEY_END - 1), (0, 1), (0, 1)):
        assert bool(host.ingplan_is_span(key_lo, key_hi, sf, oe)) == (key_lo > 0 or key_hi < KEY_END or bool(sf) or bool(oe))


def test_rings(host):
    """Slots cycle with their ring's depth; a slot is waited for exactly when an earlier window used it; between the launch of window w and
    the forced extraction of window w no other window takes its parse slot."""
    r = (C.c_uint32 * 6)()
    host.ingplan_rings(r)
    cwin, win, parse, tok, g_words, win_words = list(r)
    assert parse > win and g_words == 8 + parse * win_words
    for ring, depth in enumerate((cwin, win, parse, tok)):
        for w in range(40):
            assert host.ingplan_slot(ring, w) == w % depth
            if ring != 2:
                assert bool(host.ingplan_reused(ring, w)) == any(host.ingplan_slot(ring, v) == host.ingplan_slot(ring, w) for v in range(w))
    for w in range(40):
        upto = host.ingplan_extracted_before_launch(w)
        assert upto == (w - win if w >= win else -1)
        # windows not yet forced out when w is launched: none of them shares w's window buffer or parse slot
        for v in range(upto + 1, w):
            assert host.ingplan_slot(1, v) != host.ingplan_slot(1, w) and host.ingplan_slot(2, v) != host.ingplan_slot(2, w)


def test_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ingest_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.strip() == "%d cases, 0 bad" % (144 + 48 * 5 + 6 * 3 * 5 * 2 + 128 * 1152)
