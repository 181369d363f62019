"""csrc/sep_entry_core.h (which contigs form an entry of the separator / single-genome scan, and which contigs without a read count as its
unobserved lengths — written as prefix scans, the form the kernels of csrc/sep_kernels.hip.h run) against a serial walk written here that
mirrors covh_genome_coverage_separator's fill_backwards / fill_backwards_to_last / fill_forwards (genome.rs:448-499, 807-853).
tests/c/sep_entry_host.cpp is built twice, plainly and with -fsanitize=address,undefined, and run as a program over the same cases."""
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def walk(gid, obs):
    """The scan of host_coverage.cpp:791-866 over one sample: [(first_tid, gid, sorted member tids)], entries in the order they are printed."""
    n = len(gid)
    entries, cur, last_tid = [], None, None

    def fill_backwards(tid, g):
        members, first = [], 0
        if tid == 0:
            return members, 0
        my = tid - 1
        while gid[my] == g:
            members.append(my)
            if my == 0:
                return members, 0
            my -= 1
        return members, my + 1

    def fill_backwards_to_last(tid, last, g, members):
        for my in range(last + 1, tid):
            if gid[my] != g:
                break
            members.append(my)

    for tid in range(n):
        if not obs[tid]:
            continue
        g = gid[tid]
        if cur is None:
            m, first = fill_backwards(tid, g)
            cur = [first, g, m + [tid]]
        elif g == cur[1]:
            fill_backwards_to_last(tid, last_tid, g, cur[2])
            cur[2].append(tid)
        else:
            fill_backwards_to_last(tid, last_tid, cur[1], cur[2])
            entries.append(cur)
            m, first = fill_backwards(tid, g)
            cur = [first, g, m + [tid]]
        last_tid = tid
    if cur is not None:
        for my in range(last_tid + 1, n):          # fill_forwards
            if gid[my] != cur[1]:
                break
            cur[2].append(my)
        entries.append(cur)
    return [(f, g, sorted(m)) for f, g, m in entries]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sepc")
    src = os.path.join(HERE, "c", "sep_entry_host.cpp")
    plain, san = str(d / "sep_entry_host"), str(d / "sep_entry_host_san")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-Werror", "-o", plain, src])
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", san, src])
    return str(d), (plain, san)


def run_cases(programs, cases_, tag):
    """Every case through both builds; each output line against the walk."""
    d, exes = programs
    path = os.path.join(d, tag + ".txt")
    with open(path, "w") as f:
        for gid, obs in cases_:
            f.write("%d %s %s\n" % (len(gid), " ".join(str(int(g)) for g in gid), " ".join(str(int(o)) for o in obs)))
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (exe, r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases_)
        for (gid, obs), line in zip(cases_, lines):
            ne, row, tids, first, egid = [[int(x) for x in part.split()] for part in line.split(";")]
            want = walk(list(gid), list(obs))
            got = [(first[e], egid[e], tids[row[e]:row[e + 1]]) for e in range(ne[0])]
            assert got == want, (list(gid), list(obs), got, want)
            assert len(row) == ne[0] + 1 and row[0] == 0 and len(tids) == row[-1]
    return [walk(list(g), list(o)) for g, o in cases_]


def all_patterns(n_max, n_genomes):
    out = []
    for n in range(n_max + 1):
        for gid in itertools.product(range(n_genomes), repeat=n):
            for obs in itertools.product((0, 1), repeat=n):
                out.append((gid, obs))
    return out


def test_every_pattern_of_two_genomes(programs):
    cases_ = all_patterns(6, 2)
    assert len(cases_) == sum(4 ** n for n in range(7))
    run_cases(programs, cases_, "two")


def test_every_pattern_of_three_genomes(programs):
    run_cases(programs, all_patterns(5, 3), "three")


def test_single_genome_mode(programs):
    """gid all 0: one entry from the first target to the last whenever anything is observed."""
    cases_ = [((0,) * n, obs) for n in range(9) for obs in itertools.product((0, 1), repeat=n)]
    for (gid, obs), entries in zip(cases_, run_cases(programs, cases_, "single")):
        assert entries == ([(0, 0, list(range(len(gid))))] if any(obs) else [])


def test_cases_by_construction(programs):
    A, B = 0, 1
    cases_ = [((A, B, A, A), (1, 0, 0, 1)),      # the A behind B is counted nowhere
              ((A, A, B, B, A), (0, 0, 0, 0, 0)),      # nothing observed
              ((A, A, B, B, A), (1, 0, 0, 0, 1)),      # first and last observed
              ((A, A, B, B, A), (0, 1, 1, 0, 0)),      # first and last unobserved
              ((A, B, B, A), (0, 0, 1, 0)),
              ((A, A, B, A, A), (1, 0, 1, 0, 1))]      # a genome that recurs makes a second entry
    got = run_cases(programs, cases_, "constructed")
    assert got[0] == [(0, A, [0, 3])]
    assert got[1] == []
    assert got[2] == [(0, A, [0, 1, 4])]
    assert got[3] == [(0, A, [0, 1]), (2, B, [2, 3])]
    assert got[4] == [(1, B, [1, 2])]
    assert got[5] == [(0, A, [0, 1]), (2, B, [2]), (3, A, [3, 4])]


@pytest.mark.parametrize("frac", [0.02, 0.3, 0.9])
def test_random_blocks(programs, frac):
    """600 targets in blocks of random length over a small pool of genomes (genomes recur apart from each other)."""
    rng = np.random.default_rng(int(frac * 100))
    cases_ = []
    for _ in range(40):
        gid = []
        while len(gid) < 600:
            gid += [int(rng.integers(0, 5))] * int(rng.choice([1, 1, 2, 3, 7, 40]))
        gid = gid[:600]
        cases_.append((gid, (rng.random(600) < frac).astype(int).tolist()))
    got = run_cases(programs, cases_, "random%d" % int(frac * 100))
    assert any(len(e) > 3 for e in got)
