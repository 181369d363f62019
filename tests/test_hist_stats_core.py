"""csrc/hist_stats_core.h (a contig's window statistics read off its depth histogram: what k_estimate / k_hist_stats run per contig) on the CPU.
tests/c/hist_stats_host.cpp checks it against a loop over positions — an empty histogram, bin 0 only, a single bin at 0 / 511 / 512, a sum
of squares that passes 2^64, random histograms — and is built twice, plainly and with -fsanitize=address,undefined, and run as a program."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_hist_stats_host(tmp_path, flags):
    exe = str(tmp_path / "hist_stats_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "c", "hist_stats_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines() == ["constructed: ok", "random: ok", "ok"]
