"""csrc/depth_runs_core.h — the chunk layout, the run-start rule, the target of a word from the start mask's rank, count / emit and the chunk
planner, as the device's functors run them — emulated on the CPU (tests/c/depth_runs_host.cpp, plain and under AddressSanitizer + UBSan)
against numpy: a target's runs start at 0 and behind every np.diff(depth) != 0."""
import os
import subprocess

import numpy as np
import pytest

from tests import depth_runs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_runs")
    src = os.path.join(ROOT, "tests", "c", "depth_runs_host.cpp")
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
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return outs[0].splitlines()


def words_of(L):
    return max(1, (L + 3) // 4)


@pytest.mark.parametrize("name", sorted(R.shapes()))
def test_runs_equal_numpy(programs, name):
    depths = R.shapes()[name]
    text = "R %d %s\n%s\n" % (len(depths), " ".join(str(len(d)) for d in depths), " ".join(str(int(v)) for d in depths for v in d))
    lines = run(programs, text, name)
    off, start, depth = R.runs_of(depths)
    ints = lambda l: [int(x) for x in l.split()[1:]]
    assert ints(lines[0]) == [len(start), sum(words_of(len(d)) for d in depths)]
    assert ints(lines[1]) == off.tolist()
    assert ints(lines[2]) == start.tolist()
    assert ints(lines[3]) == depth.tolist()
    # the runs of a target tile [0, L): first start 0, starts ascending, no run for an empty target
    for t, d in enumerate(depths):
        s = start[int(off[t]):int(off[t + 1])]
        assert (len(s) == 0) == (len(d) == 0)
        assert len(s) == 0 or (s[0] == 0 and (np.diff(s.astype(np.int64)) > 0).all() and s[-1] < len(d))


def plan_ref(lens, budget):
    """At least one target, then as many as still fit `budget` arena entries (a target takes its words of four)."""
    cuts, lo = [], 0
    while lo < len(lens):
        used, t = 4 * words_of(lens[lo]), lo + 1
        while t < len(lens) and used + 4 * words_of(lens[t]) <= budget:
            used += 4 * words_of(lens[t])
            t += 1
        cuts.append(t)
        lo = t
    return cuts


PLANS = [
    ("budget_below_one_target", [5000, 10, 7000, 3], 2048),
    ("exactly_one_target", [2048, 2048, 2048], 2048),
    ("one_target_and_a_base_more", [2048, 1, 2048], 2052),
    ("empty_targets_at_the_edges", [0, 0, 2040, 0, 0, 2044, 0, 4, 0], 2048),
    ("everything_fits", [1, 2, 3, 0, 1000], 1 << 28),
    ("all_empty", [0] * 9, 16),
    ("odd_lengths", list(R.EDGE_LENGTHS) * 3, 2048),
]


def test_planner(programs):
    text = "".join("P %d %d %s\n" % (len(lens), budget, " ".join(map(str, lens))) for _, lens, budget in PLANS)
    lines = run(programs, text, "plans")
    assert len(lines) == len(PLANS)
    for line, (name, lens, budget) in zip(lines, PLANS):
        got = [int(x) for x in line.split()[1:]]
        assert got == plan_ref(lens, budget), name
        assert got[-1] == len(lens) and all(b > a for a, b in zip([0] + got, got)), name
        for a, b in zip([0] + got, got):      # a chunk above the budget is one target
            assert sum(4 * words_of(L) for L in lens[a:b]) <= budget or b - a == 1, name
    assert plan_ref(PLANS[0][1], 2048) == [1, 2, 3, 4] and plan_ref(PLANS[1][1], 2048) == [1, 2, 3]
    assert plan_ref(PLANS[3][1], 2048) == [3, 5, 7, 9]
