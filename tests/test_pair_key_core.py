"""csrc/pair_key_core.h — the pair filter's join key, the slot its probe run starts at and the table's size — run on the CPU
(tests/c/pair_key_host.cpp, built plainly and with -fsanitize=address,undefined, run as a program) against the second statement of the same
three rules in tests/pair_cases.py, with which the table cases place their keys."""
import os
import subprocess

import numpy as np
import pytest

from tests import pair_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair_key")
    src = os.path.join(ROOT, "tests", "c", "pair_key_host.cpp")
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
    return [[int(x) for x in l.split()[1:]] for l in outs[0].splitlines()]


def test_keys_and_slots(programs):
    """Random keys and the corner keys: qh1 0 and 1, tid -1, 0 and 2^31 - 1, every mask from one entry to 2^31."""
    rng = np.random.default_rng(5)
    keys = [(q1, q2, tid, mask) for q1 in (0, 1, 2, (1 << 64) - 1) for q2 in (0, 1, 0xFFFFFFFF) for tid in (-1, 0, 1, (1 << 31) - 1)
            for mask in (0, 1, 1023, 2047, (1 << 31) - 1)]
    for _ in range(20_000):
        keys.append((int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, 1 << 32)), int(rng.integers(-1, 1 << 31)),
                     (1 << int(rng.integers(0, 32))) - 1))
    got = run(programs, "".join("K %d %d %d %d\n" % k for k in keys), "keys")
    assert len(got) == len(keys)
    for (q1, q2, tid, mask), (k1, k2t, slot) in zip(keys, got):
        assert (k1, k2t, slot) == (P.key_k1(q1), P.key_k2t(q2, tid), P.slot_of(q1, q2, tid, mask)), (q1, q2, tid, mask)
        assert k1 != 0 and k2t != 0 and slot <= mask
    # the rules themselves, on the corners
    assert P.key_k1(0) == P.key_k1(1) == 1 and P.key_k1(2) == 2
    assert P.key_k2t(5, -1) == 5 | 1 << 32 and P.key_k2t(5, 0) == 5 | 2 << 32 and P.key_k2t(0, (1 << 31) - 1) == ((1 << 31) + 1) << 32
    assert len({P.key_k2t(9, t) for t in (-1, 0, 1, (1 << 31) - 1)}) == 4


def test_table_sizes(programs):
    sizes = [0, 1, 511, 512, 513, 1023, 1024, 1025, 4 << 20, (4 << 20) + 1, 1 << 30, (1 << 30) + 1, 0xFFFFFFFF]
    got = run(programs, "".join("Z %d\n" % n for n in sizes), "sizes")
    assert [g[0] for g in got] == [P.table_size(n) for n in sizes]
    assert [P.table_size(n) for n in (0, 1, 511, 512, 513)] == [1024, 1024, 1024, 1024, 2048]
    for n, (z,) in zip(sizes, got):
        assert z >= 1024 and z >= 2 * n and z & (z - 1) == 0 and (z == 1024 or z // 2 < 2 * n)
