"""csrc/pileup_schedule_core.h (which tiles each wave of k_pileup_fast visits: the deep-tile list first, one tile per visit, then its chunks)
on the CPU.  tests/c/pileup_schedule_host.cpp enumerates every wave's visits over a grid of tile counts, chunk sizes, wave counts and list
lengths, with the listed tiles at the front, at the back and scattered, and checks that together they cover every list entry and every
unflagged tile exactly once, no flagged tile in the chunk phase, no index past either end.  Built twice, plainly and with
-fsanitize=address,undefined, and run as a program."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pileup_schedule_host(tmp_path, flags):
    exe = str(tmp_path / "pileup_schedule_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "c", "pileup_schedule_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and lines[0].startswith("cells: ") and int(lines[0].split()[1]) > 500, lines
