"""csrc/depth_regions_core.h — a region's descriptor, its pieces, the search a wave runs and a word as a lane sees it — emulated on the CPU
(tests/c/depth_regions_host.cpp, plain and under AddressSanitizer + UBSan) against numpy slices of the depth: the pieces are merged in a
shuffled order, and the result must not depend on it."""
import os
import subprocess

import numpy as np
import pytest

from tests import depth_regions_ref as G
from tests import depth_runs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = G.W


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_regions")
    src = os.path.join(ROOT, "tests", "c", "depth_regions_host.cpp")
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


def case(depths, regions, seed):
    lens = [len(d) for d in depths]
    return "G %d %d %d %s\n%s\n%s\n" % (len(depths), len(regions), seed, " ".join(map(str, lens)), " ".join(str(int(v)) for d in depths for v in d),
                                      " ".join("%d %d %d" % r for r in regions))


ints = lambda l: [int(x) for x in l.split()[1:]]


def test_the_sets_are_what_the_tests_rely_on():
    """The largest shape has a region of 13 pieces; the piece set holds the one-piece / two-piece pair at skip 3."""
    depths = R.shapes()["runs_cross_boundaries"]
    lens = [len(d) for d in depths]
    sets = G.region_sets(lens)
    assert max(lens) == 49229 and G.pieces_of(0, 49229) == 13 and (0, 0, 49229) in sets["pieces"] and sets["overlap"].count((0, 0, 49229)) >= 6
    assert G.pieces_of(3, 3 + W - 3) == 1 and G.pieces_of(3, 3 + W - 2) == 2 and (0, 3, W) in sets["pieces"] and (0, 3, W + 1) in sets["pieces"]
    assert len(sets["random"]) == 300 and sets["steps"] and sets["edges"]
    for regs in sets.values():
        assert all(0 <= a < e <= lens[t] for t, a, e in regs)
    tids = [t for t, _, _ in sets["overlap"]]
    assert tids != sorted(tids)      # interleaved: the stable order by tid has work to do


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_regions_equal_numpy(programs, name):
    depths = R.shapes()[name]
    lens = [len(d) for d in depths]
    sets = G.region_sets(lens)
    cases = [(k, seed) for k in sorted(sets) for seed in (0, 7 + len(sets[k]))]      # ascending, and shuffled
    lines = run(programs, "".join(case(depths, sets[k], seed) for k, seed in cases), name)
    assert len(lines) == 6 * len(cases)
    for i, (k, seed) in enumerate(cases):
        got = lines[6 * i:6 * i + 6]
        assert [l[0] for l in got] == list("NPSIAC")
        regs = sets[k]
        want = G.reduce(depths, regs)
        msg = "%s %s seed=%d" % (name, k, seed)
        pieces = [G.pieces_of(a, e) for _, a, e in regs]
        assert ints(got[0]) == [len(regs), sum(pieces), sum(max(1, (L + 3) // 4) for L in lens), W], msg
        assert ints(got[1]) == pieces, msg
        assert ints(got[2]) == want["sum"].tolist(), msg
        assert ints(got[3]) == want["min"].tolist(), msg
        assert ints(got[4]) == want["max"].tolist(), msg
        assert ints(got[5]) == want["covered"].tolist(), msg
        if i % 2:      # the shuffled order gives the ascending order's output
            assert got == lines[6 * (i - 1):6 * i], msg
    if name == "empty_targets_only":
        assert all(not regs for regs in sets.values())
        assert all(l == "N 0 0 %d %d" % (len(depths), W) for l in lines[0::6])


def test_large_depths_do_not_wrap(programs):
    """Depths near 2^31 - 1: a region's sum needs its 64 bits, min and max their sign."""
    big = 2 ** 31 - 1
    depths = [np.full(2 * W + 9, big, np.int64), np.asarray([big, 0, big - 1, 5, 1], np.int64)]
    regs = [(0, 0, 2 * W + 9), (0, 3, W + 1), (1, 0, 5), (1, 1, 3), (0, 5, 6), (1, 2, 5)]
    for seed in (0, 11):
        lines = run(programs, case(depths, regs, seed), "large_%d" % seed)
        want = G.reduce(depths, regs)
        assert int(want["sum"][0]) == (2 * W + 9) * big > 2 ** 32
        assert ints(lines[2]) == want["sum"].tolist() and ints(lines[3]) == want["min"].tolist() and ints(lines[4]) == want["max"].tolist()
        assert ints(lines[5]) == want["covered"].tolist()


def test_a_neighbours_depth_and_the_pad_are_never_added(programs):
    """A region that ends one base in front of its target's end, beside a neighbour of large depth: the entries behind the region in its last
    word (the target's last base, PAD, and in the next word the neighbour) stay out."""
    depths = [np.asarray([1, 2, 3, 4, 5, 6], np.int64), np.full(9, 1000, np.int64), np.asarray([7], np.int64)]
    regs = [(0, 0, 5), (0, 1, 5), (0, 4, 5), (0, 5, 6), (1, 0, 9), (1, 3, 4), (2, 0, 1), (1, 8, 9)]
    lines = run(programs, case(depths, regs, 3), "neighbour")
    want = G.reduce(depths, regs)
    assert ints(lines[2]) == want["sum"].tolist() == [15, 14, 5, 6, 9000, 1000, 7, 1000]
    assert ints(lines[3]) == want["min"].tolist() and ints(lines[4]) == want["max"].tolist() and ints(lines[5]) == want["covered"].tolist()
