"""csrc/depth_class_core.h — the cut list's validator, class_of, the class view behind the run arithmetic of csrc/depth_runs_core.h and the
threshold counts of a region's word — emulated on the CPU (tests/c/depth_classes_host.cpp, plain and under AddressSanitizer + UBSan) against
numpy: searchsorted, the run-length encoding of the classes, and slices of the depth."""
import os
import subprocess

import numpy as np
import pytest

from tests import depth_classes_ref as K
from tests import depth_regions_ref as G
from tests import depth_runs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_classes")
    src = os.path.join(ROOT, "tests", "c", "depth_classes_host.cpp")
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


cut_text = lambda cuts: "%d %s" % (len(cuts), " ".join(map(str, cuts)))
ints = lambda l: [int(x) for x in l.split()[1:]]


def test_class_of_at_every_cut(programs):
    """cut - 1, cut and cut + 1 of every cut of every list, 0 and 2^31 - 1; n = 1 (ONE, TOP) and n = 16 (UNIT and a list that ends at the top)."""
    lists = dict(K.CUT_LISTS)
    lists["SIXTEEN_TO_THE_TOP"] = tuple(range(0, 15 * 1000, 1000)) + (K.TOP_DEPTH,)
    assert len(lists["UNIT"]) == 16 and len(lists["SIXTEEN_TO_THE_TOP"]) == 16 and len(lists["ONE"]) == 1
    cases = []
    for name, cuts in sorted(lists.items()):
        ds = sorted({0, K.TOP_DEPTH} | {d for c in cuts for d in (c - 1, c, c + 1) if 0 <= d <= K.TOP_DEPTH})
        cases.append((name, cuts, ds))
    lines = run(programs, "".join("C %s %d %s\n" % (cut_text(c), len(ds), " ".join(map(str, ds))) for _, c, ds in cases), "class_of")
    assert len(lines) == len(cases)
    for line, (name, cuts, ds) in zip(lines, cases):
        assert ints(line) == K.class_of(ds, cuts).tolist(), name
    # the top depth is in the last class of a list that holds it, and in class n of any other: no sentinel takes it
    assert K.class_of([K.TOP_DEPTH], K.TOP)[0] == 1 and K.class_of([K.TOP_DEPTH - 1], K.TOP)[0] == 0 and K.class_of([K.TOP_DEPTH], K.ONE)[0] == 1


def test_validator(programs):
    cases = [((), 0, "empty"), (tuple(range(17)), 16, "more than 16"), ((1, 5, 4, 9), 2, "ascending"), ((1, 5, 5, 9), 2, "ascending"),
             ((0, 3, -1), 2, "negative"), ((-5,), 0, "negative"), ((3, 2), 1, "ascending")]
    good = [K.MIXED, K.ZERO_ONE, K.UNIT, K.TOP, K.ONE, (0,), (0, K.TOP_DEPTH)]
    lines = run(programs, "".join("V %s\n" % cut_text(c) for c, _, _ in cases) + "".join("V %s\n" % cut_text(c) for c in good), "validate")
    assert len(lines) == len(cases) + len(good)
    for line, (cuts, at, what) in zip(lines, cases):
        f = line.split(" ", 2)
        assert f[0] == "V" and int(f[1]) == at and what in f[2], (cuts, line)
    assert lines[len(cases):] == ["V ok"] * len(good)


@pytest.mark.parametrize("name", sorted(K.shapes()))
def test_class_runs_equal_numpy(programs, name):
    """Every shape (PAD, empty targets, three targets in a word, the arena of exactly the promised size) under every cut list."""
    depths = K.shapes()[name]
    body = "%d %s\n%s\n" % (len(depths), " ".join(str(len(d)) for d in depths), " ".join(str(int(v)) for d in depths for v in d))
    lists = sorted(K.CUT_LISTS.items())
    lines = run(programs, "".join("Q %s %s" % (cut_text(c), body) for _, c in lists), name)
    assert len(lines) == 4 * len(lists)
    for i, (cname, cuts) in enumerate(lists):
        got = lines[4 * i:4 * i + 4]
        off, start, cls = K.class_runs_of(depths, cuts)
        msg = "%s %s" % (name, cname)
        assert ints(got[0]) == [len(start), sum(max(1, (len(d) + 3) // 4) for d in depths)], msg
        assert ints(got[1]) == off.tolist(), msg
        assert ints(got[2]) == start.tolist(), msg
        assert ints(got[3]) == cls.tolist(), msg
        if cname == "UNIT" and all(int(np.max(d, initial=0)) <= 14 for d in depths):      # the class runs are the depth runs
            doff, dstart, ddepth = R.runs_of(depths)
            assert off.tolist() == doff.tolist() and start.tolist() == dstart.tolist() and (cls == ddepth + 1).all(), msg


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_threshold_counts_equal_numpy(programs, name):
    """The five region sets, MIXED and UNIT, the pieces merged in ascending and in shuffled order."""
    depths = R.shapes()[name]
    lens = [len(d) for d in depths]
    sets = G.region_sets(lens)
    assert sorted(sets) == ["edges", "overlap", "pieces", "random", "steps"]
    head = lambda regs, seed: "%d %d %d %s\n%s\n%s\n" % (len(depths), len(regs), seed, " ".join(map(str, lens)), " ".join(str(int(v)) for d in depths for v in d),
                                                       " ".join("%d %d %d" % r for r in regs))
    cases = [(k, tn, seed) for k in sorted(sets) for tn in ("MIXED", "UNIT") for seed in (0, 7 + len(sets[k]))]
    lines = run(programs, "".join("T %s %s" % (cut_text(K.CUT_LISTS[tn]), head(sets[k], seed)) for k, tn, seed in cases), name)
    at = 0
    for k, tn, seed in cases:
        regs, thr = sets[k], K.CUT_LISTS[tn]
        assert lines[at] == "K %d %d" % (len(regs), len(thr))
        got = np.asarray([ints(l) for l in lines[at + 1:at + 1 + len(regs)]], np.int64).reshape(len(regs), len(thr))
        np.testing.assert_array_equal(got, K.counts(depths, regs, thr), err_msg="%s %s %s seed=%d" % (name, k, tn, seed))
        at += 1 + len(regs)
    assert at == len(lines)


def test_a_neighbours_depth_and_the_pad_are_never_counted(programs):
    """A region that ends in front of its target's end, beside a neighbour of large depth: the entries behind the region in its last word
    (the target's last base, PAD, and in the next word the neighbour) stay out, for a threshold of 0 too (PAD is below it)."""
    depths = [np.asarray([1, 2, 3, 4, 5, 6], np.int64), np.full(9, 1000, np.int64), np.asarray([7], np.int64)]
    regs = [(0, 0, 5), (0, 1, 5), (0, 4, 5), (0, 5, 6), (1, 0, 9), (1, 3, 4), (2, 0, 1), (1, 8, 9)]
    thr = (0, 1, 5, 7, 1000)
    text = "T %s 3 %d 3 6 9 1\n%s\n%s\n" % (cut_text(thr), len(regs), " ".join(str(int(v)) for d in depths for v in d), " ".join("%d %d %d" % r for r in regs))
    lines = run(programs, text, "neighbour")
    got = [ints(l) for l in lines[1:]]
    assert got == K.counts(depths, regs, thr).tolist()
    assert got[0] == [5, 5, 1, 0, 0] and got[4] == [9, 9, 9, 9, 9] and got[6] == [1, 1, 1, 1, 0]
