"""csrc/slot_ring.h (the producer / consumer handshake over the staging slots that both device ingest feeders use): the stand-alone program
tests/c/slot_ring_host.cpp, built once with the thread sanitizer and once with the address and undefined-behaviour sanitizers.  It runs
under a time limit: a handshake that leaves one side waiting is a failure, not a wait."""
import os
import platform
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "slot_ring_host.cpp")


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_both_threads_return_in_every_case(tmp_path, sanitize):
    exe = str(tmp_path / "slot_ring_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC,
                           "-lpthread"])
    run = lambda pre: subprocess.run(pre + ["timeout", "-k", "5", "60", exe], capture_output=True, text=True, timeout=90)
    r = run([])
    if r.returncode == 66 and "unexpected memory mapping" in r.stderr and shutil.which("setarch"):
        # the thread sanitizer's runtime gave up before main: its shadow memory does not fit the address-space randomisation of this
        # kernel.  The same program with the randomisation off for this one process.
        r = run(["setarch", platform.machine(), "-R"])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip() == "%d cases, 0 bad" % (8 * (5 * 2 + 4 * 2 * 5))
