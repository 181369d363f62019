"""csrc/depth_bins_core.h — the bin geometry, a word's partials and their merge, as the device's lanes run them — emulated on the CPU
(tests/c/depth_bins_host.cpp, plain and under AddressSanitizer + UBSan) against numpy's reduceat: the arena's words are merged in a shuffled
order, and the result must not depend on it."""
import os
import subprocess

import numpy as np
import pytest

from tests import depth_bins_ref as B
from tests import depth_runs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = B.stretch_bases()
BIN_SIZES = [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1000, 1024, W - 1, W, W + 1, 16384, 50000, 2 ** 31 - 1]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_bins")
    src = os.path.join(ROOT, "tests", "c", "depth_bins_host.cpp")
    plain, san = str(d / "plain"), str(d / "san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", san, src])
    return d, (plain, san)


def run(programs, text, tag):
    d, exes = programs
    path = str(d / (tag + ".txt"))
    with open(path, "w") as fh:
        fh.write(text)
    outs = []
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return outs[0].splitlines()


def test_the_stretch_is_a_whole_number_of_wave_loads():
    assert W % 256 == 0 and W >= 256


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_bins_equal_numpy(programs, name):
    depths = R.shapes()[name]
    lens = [len(d) for d in depths]
    flat = " ".join(str(int(v)) for d in depths for v in d)
    cases = [(bs, seed) for bs in BIN_SIZES for seed in (0, 1 + bs)]      # ascending, and shuffled
    text = "".join("B %d %d %d %s\n%s\n" % (len(depths), bs, seed, " ".join(map(str, lens)), flat) for bs, seed in cases)
    lines = run(programs, text, name)
    assert len(lines) == 7 * len(cases)
    ints = lambda l: [int(x) for x in l.split()[1:]]
    for i, (bs, seed) in enumerate(cases):
        got = lines[7 * i:7 * i + 7]
        assert [l[0] for l in got] == list("NOLSIAC")
        off, bins = B.bins_of(depths, bs)
        msg = "%s B=%d seed=%d" % (name, bs, seed)
        assert ints(got[0]) == [len(bins), sum(max(1, (L + 3) // 4) for L in lens), W], msg
        assert ints(got[1]) == off.tolist(), msg
        assert ints(got[2]) == B.bin_lengths(lens, bs), msg
        assert ints(got[3]) == bins["sum"].tolist(), msg
        assert ints(got[4]) == bins["min"].tolist(), msg
        assert ints(got[5]) == bins["max"].tolist(), msg
        assert ints(got[6]) == bins["covered"].tolist(), msg
        # an empty target repeats its neighbour's offset; the bins of a target tile [0, L)
        for t, L in enumerate(lens):
            assert int(off[t + 1] - off[t]) == (L + bs - 1) // bs, msg
        assert sum(B.bin_lengths(lens, bs)) == sum(lens), msg
    if name == "empty_targets_only":
        assert all(l == "N 0 %d %d" % (len(depths), W) for l in lines[0::7])


def test_large_depths_do_not_wrap(programs):
    """Depths near 2^31: a bin's sum needs its 64 bits, min and max their sign."""
    big = 2 ** 31 - 1
    depths = [np.full(9, big, np.int64), np.asarray([big, 0, big - 1, 5, 1], np.int64)]
    lens = [len(d) for d in depths]
    for bs in (1, 3, 4, 7, 1000):
        text = "B 2 %d 7 %s\n%s\n" % (bs, " ".join(map(str, lens)), " ".join(str(int(v)) for d in depths for v in d))
        lines = run(programs, text, "large_%d" % bs)
        off, bins = B.bins_of(depths, bs)
        ints = lambda l: [int(x) for x in l.split()[1:]]
        assert ints(lines[3]) == bins["sum"].tolist() and ints(lines[4]) == bins["min"].tolist() and ints(lines[5]) == bins["max"].tolist()
