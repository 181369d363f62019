"""csrc/cli_route.h (which reader takes a sample, and which one takes it after a decline) against the route conditions ingest() held before
they were gathered there, frozen in tests/c/cli_route_host.cpp: equal route and equal refusal text for every combination of the nine
switches and span_count 1 / 2 that can reach ingest() — a pipe is never BGZF (is_bgzf) and never comes with --no-stream (run_cli refuses
that pair before any sample is opened).  Rows of the table in DESIGN.md section 1 are stated literally as well, so that a mistake made on
both sides of the comparison still shows."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("bgzf", "piped", "no_stream", "per_gene", "pair_filter", "no_gpu_ingest", "pair_on_host", "sam_on_host", "genes_decode_on_host")
DEVICE_BGZF, CPU_STREAM, DEVICE_SAM, HOST_WHOLE = 0, 1, 2, 3
SPANS = "--devices with fewer BAM files than devices needs streamable input (BAM, no --gff)"
PIPE_ONLY = "a pipe ('-b -', a FIFO) is decoded on the device only: COVERM_SAM_ON_HOST / COVERM_PAIR_ON_HOST need a file"
SPAN_PAIR = "--devices with fewer BAM files than devices and a pair-mode filter needs the device ingest, which declined this file: why"
PIPE_AGAIN = "smp: why — a pipe cannot be read again: write the stream to a file"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("route") / "cli_route_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "c", "cli_route_host.cpp")])
    L = C.CDLL(so)
    for f in (L.route_first, L.route_first_frozen):
        f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    for f in (L.route_after, L.route_after_frozen):
        f.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    return L


def facts(span_count=1, **on):
    assert set(on) <= set(NAMES)
    return (C.c_int32 * 10)(*[int(bool(on.get(n))) for n in NAMES], span_count)


def first(fn, f):
    msg = C.create_string_buffer(512)
    r = fn(f, msg, 512)
    return r if r >= 0 else msg.value.decode()


def after(fn, declined, f):
    msg = C.create_string_buffer(512)
    r = fn(declined, f, b"smp", b"why", msg, 512)
    return r if r >= 0 else msg.value.decode()


def test_every_combination_equals_the_frozen_conditions(host):
    n = n_declines = 0
    seen = set()
    for bits in itertools.product((0, 1), repeat=9):
        on = dict(zip(NAMES, bits))
        if on["piped"] and (on["bgzf"] or on["no_stream"]):
            continue
        for span_count in (1, 2):
            f = facts(span_count, **on)
            got = first(host.route_first, f)
            assert got == first(host.route_first_frozen, f), (on, span_count)
            seen.add(got)
            n += 1
            if got in (DEVICE_BGZF, DEVICE_SAM):
                nxt = after(host.route_after, got, f)
                assert nxt == after(host.route_after_frozen, got, f), (on, span_count)
                assert nxt not in (DEVICE_BGZF, DEVICE_SAM)             # a second decline cannot happen: the routes that take over never decline
                seen.add(("after", got, nxt))
                n_declines += 1
    assert n == 2 * (512 - 128 - 128 + 64) and n_declines == 28 + 36      # (counted by hand: DeviceBgzf 24 + 4 with --gff, DeviceSam 4 x 3 x 3)
    # every outcome of both tables occurred
    assert seen >= {DEVICE_BGZF, CPU_STREAM, DEVICE_SAM, HOST_WHOLE, SPANS, PIPE_ONLY, ("after", DEVICE_BGZF, CPU_STREAM), ("after", DEVICE_BGZF, HOST_WHOLE),
                    ("after", DEVICE_BGZF, SPAN_PAIR), ("after", DEVICE_SAM, HOST_WHOLE), ("after", DEVICE_SAM, PIPE_AGAIN)}


FIRST_ROWS = [
    (dict(bgzf=1), 1, DEVICE_BGZF),
    (dict(bgzf=1), 2, DEVICE_BGZF),
    (dict(bgzf=1, pair_filter=1), 2, DEVICE_BGZF),
    (dict(bgzf=1, per_gene=1, pair_filter=1), 1, DEVICE_BGZF),
    (dict(bgzf=1, per_gene=1), 2, SPANS),
    (dict(bgzf=1, per_gene=1, genes_decode_on_host=1), 1, HOST_WHOLE),
    (dict(bgzf=1, per_gene=1, pair_on_host=1), 1, HOST_WHOLE),                 # (--gff: the switch alone keeps the file on the host)
    (dict(bgzf=1, pair_on_host=1), 1, DEVICE_BGZF),                            # (without a pair-mode filter the switch says nothing)
    (dict(bgzf=1, pair_filter=1, pair_on_host=1), 1, HOST_WHOLE),
    (dict(bgzf=1, pair_filter=1, pair_on_host=1), 2, SPANS),
    (dict(bgzf=1, no_gpu_ingest=1), 2, CPU_STREAM),
    (dict(bgzf=1, no_gpu_ingest=1, pair_filter=1), 1, HOST_WHOLE),
    (dict(bgzf=1, no_stream=1), 1, HOST_WHOLE),
    (dict(), 1, DEVICE_SAM),
    (dict(), 2, SPANS),
    (dict(per_gene=1, pair_filter=1), 1, DEVICE_SAM),
    (dict(no_gpu_ingest=1), 1, HOST_WHOLE),
    (dict(piped=1, no_gpu_ingest=1), 1, DEVICE_SAM),                           # a pipe has no other reader
    (dict(sam_on_host=1), 1, HOST_WHOLE),
    (dict(piped=1, sam_on_host=1), 1, PIPE_ONLY),
    (dict(piped=1, pair_filter=1, pair_on_host=1), 1, PIPE_ONLY),
    (dict(no_stream=1), 1, HOST_WHOLE),
]

AFTER_ROWS = [
    (DEVICE_BGZF, dict(bgzf=1), 1, CPU_STREAM),
    (DEVICE_BGZF, dict(bgzf=1), 2, CPU_STREAM),
    (DEVICE_BGZF, dict(bgzf=1, pair_filter=1), 1, HOST_WHOLE),
    (DEVICE_BGZF, dict(bgzf=1, pair_filter=1), 2, SPAN_PAIR),
    (DEVICE_BGZF, dict(bgzf=1, per_gene=1), 1, HOST_WHOLE),
    (DEVICE_BGZF, dict(bgzf=1, per_gene=1, pair_filter=1), 1, HOST_WHOLE),
    (DEVICE_SAM, dict(), 1, HOST_WHOLE),
    (DEVICE_SAM, dict(per_gene=1), 1, HOST_WHOLE),
    (DEVICE_SAM, dict(piped=1), 1, PIPE_AGAIN),
    (DEVICE_SAM, dict(piped=1, pair_filter=1), 1, PIPE_AGAIN),
]


def test_rows_of_the_route_table(host):
    for on, span_count, want in FIRST_ROWS:
        assert first(host.route_first, facts(span_count, **on)) == want, (on, span_count)
    for declined, on, span_count, want in AFTER_ROWS:
        f = facts(span_count, **on)
        assert first(host.route_first, f) == declined, (on, span_count)      # the row starts from the route these facts take first
        assert after(host.route_after, declined, f) == want, (declined, on, span_count)
